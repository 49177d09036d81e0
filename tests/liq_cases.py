"""Seeded inputs for the liq_parm routines and what the order-faithful restatements (oracle/kmt_py.py, oracle/liq_py.py, oracle/rates_py.py) make of
them: the cases of tests/test_liq_cases.py (CPU: do the cases reach every branch and chunk edge? how far do the restatements move under last-place
freedom of exp / log?) and of tests/test_gpu_liq_synth.py (the device kernels against the same expected values).  Plain module, no GPU.  The captured
fixtures reach one ka, one kw vector, ifeed = 0, 281-288 K and no droplet bin; these cases are the smallest that reach the rest:

  fast_k_mt   7 calls (ka, ifeed, nkc_l, kw) of 3-4 layers on the table's 70 x 70 grid: empty, one-row, exact-multiple-of-56 and ragged bins
  cw_rc       grids from 1 x 1 to 5 x 2048, the ka boundary inside a chunk and on a chunk edge, humidities at every threshold of the on/off table
  dry_rates   1, 64, 65, 200 layers (one thread each, blocks of 64), rcd <= 0, 200-310 K
  henry, v_mean, equil_co, st_coeff   1 and 300 layers over the model's temperature range, bins without water, every switch setting

Every generator is seeded and cached: both test files see the same arrays, which nobody may write to (they are made read-only)."""
import functools
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle import kmt_py, liq_py, rates_py      # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
NKC = 4
KMT_CELLS = 56          # grid cells per chunk of fast_k_mt_kernel
CWRC_CHUNK = 2048       # grid cells per chunk of cw_rc_kernel
CWM, CWMD = 1.0e-1, 1.0e2


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


def poison(shape, base):
    """negative, finite, different in every entry: what a routine must leave alone can be read back from it"""
    return -(base + 0.5 * np.arange(int(np.prod(shape)), dtype=np.float64)).reshape(shape)


def _loguniform(rng, lo, hi, size=None):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), size))


def _signs(rng, size, values):
    """values > 0 kept in about 60 % of the entries, 0 in 20 %, negated in 20 %"""
    pick = rng.random(size)
    return np.where(pick < 0.6, values, np.where(pick < 0.8, 0.0, -values))


def nspec(mech):
    return liq_py.load(mech)["nspec"]


# ---------------------------------------------------------------------------------------------------------------- last-place freedom of libm
class MathShim:
    """the math module with exp, log, log10, pow and sqrt moved to the next double up (or down)"""

    def __init__(self, up):
        self._to = math.inf if up else -math.inf

    def __getattr__(self, name):
        return getattr(math, name)

    def exp(self, x): return math.nextafter(math.exp(x), self._to)
    def log(self, x): return math.nextafter(math.log(x), self._to)
    def log10(self, x): return math.nextafter(math.log10(x), self._to)
    def pow(self, a, b): return math.nextafter(math.pow(a, b), self._to)
    def sqrt(self, x): return math.nextafter(math.sqrt(x), self._to)


class shimmed_math:
    """with shimmed_math(up): the restatements' `math` is the shim"""

    def __init__(self, up):
        self.shim = MathShim(up)

    def __enter__(self):
        for m in (kmt_py, liq_py, rates_py):
            assert m.math is math
            m.math = self.shim

    def __exit__(self, *a):
        for m in (kmt_py, liq_py, rates_py):
            m.math = math


def movement(nominal, moved):
    """worst |moved - nominal| / |nominal| over the entries whose nominal value is not 0 (exp(0) = 1 and sqrt(0) = 0 are exact in every libm: an entry
    that is exactly 0 has no last place to move in, and the GPU tests hold the zero patterns equal)"""
    a, b = np.asarray(nominal, np.float64).ravel(), np.asarray(moved, np.float64).ravel()
    nz = a != 0.0
    return float((np.abs(b[nz] - a[nz]) / np.abs(a[nz])).max()) if nz.any() else 0.0


def spread(compute):
    """compute() -> tuple of arrays: the worst movement of any of them under the shim, up and down"""
    nominal = compute()
    worst = 0.0
    for up in (True, False):
        with shimmed_math(up):
            moved = compute()
        worst = max([worst] + [movement(a, b) for a, b in zip(nominal, moved)])
    return worst


def close(got, want, bound):
    """every entry within bound * |want| (an entry that is 0 in want is 0 in got): -> (all within, worst relative difference of the entries that
    differ at all or 0., number of entries bit-identical)"""
    got, want = np.asarray(got), np.asarray(want)
    d = np.abs(got - want)
    ok = bool(np.all(d <= bound * np.abs(want)))
    nz = want != 0.0
    worst = float((d[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
    return ok, worst, int((got == want).sum())


# ---------------------------------------------------------------------------------------------------------------- fast_k_mt
# (ka, ifeed, nkc_l, kw kind, layers, rotation of the (cm, cw) signs): tests/test_liq_cases.py holds what each reaches
KMT_CALLS = (
    (52, 0, 4, "captured", 4, 0),     # the model's split; bins 1/3 = 3640 cells = 65 chunks exactly, bins 2/4 = 1260 cells, ragged; layer 3 is Stokes-only
    (0, 0, 4, "seeded", 3, 1),        # bins 1/3 empty (ka = 0), bins 2/4 the whole grid (4900 cells, ragged)
    (1, 2, 4, "zeros", 3, 3),         # bins 1/3 empty (ifeed = 2: ia from 2 to ka = 1); kw = 0: bins 1/2 hold no cell in range, bins 3/4 all of theirs
    (1, 0, 2, "full", 3, 2),          # bins 1/3 one row = 70 cells = two chunks, the second ragged; kw = nkt: bin 3/4 ranges empty; nkc_l = 2
    (4, 0, 4, "seeded", 3, 2),        # bins 1/3 = 280 cells = 5 chunks exactly
    (69, 2, 4, "seeded", 3, 0),       # bins 1/3 = rows 2..69 = 4760 cells = 85 chunks exactly; bins 2/4 one row
    (70, 0, 4, "captured", 3, 1),     # bins 2/4 empty (ka = nka)
)
KMT_STOKES = (0, 3)                   # (call, layer) whose ff is non-zero only where rq <= 10 um


def _kw(rng, kind, nka, nkt, captured=None):
    if kind == "captured":
        assert captured is not None and len(captured) == nka
        return np.array(captured, np.int32)
    if kind == "zeros":
        return np.zeros(nka, np.int32)
    if kind == "full":
        return np.full(nka, nkt, np.int32)
    kw = rng.integers(0, nkt + 1, nka).astype(np.int32)
    kw[rng.integers(0, nka)] = 0          # both ends occur (they may fall on the same row in a one-row grid: the later one holds)
    kw[(int(np.argmin(kw)) + 1 + rng.integers(0, max(1, nka - 1))) % nka] = nkt
    return kw


@functools.lru_cache(maxsize=None)
def kmt_calls(mech):
    g = np.load(os.path.join(GOLD, "kmt_%s.npz" % mech))
    tab = kmt_py.load(mech)
    nka, nkt, ns = tab["nka"], tab["nkt"], nspec(mech)
    rq = np.array(g["rq"])
    rng = np.random.default_rng({"aer": 9501, "tot": 9502}[mech])
    calls = []
    for ci, (ka, ifeed, nkc_l, kind, nl, rot) in enumerate(KMT_CALLS):
        ff = rng.uniform(0.01, 5.0, (nl, nka, nkt)) * (rng.random((nl, nka, nkt)) < 0.7)
        stokes = np.zeros(nl, bool)
        if ci == KMT_STOKES[0]:
            ff[KMT_STOKES[1]] *= rq <= 10.0
            stokes[KMT_STOKES[1]] = True
        cw, cm = np.empty((nl, NKC)), np.empty((nl, NKC))
        for i in range(nl):
            for b in range(NKC):
                combo = (b + i + rot) % 4      # 0: cm > 0, cw > 0   1: cm > 0, cw <= 0   2: cm <= 0, cw > 0   3: both <= 0
                off = 0.0 if (i + b) % 2 else -1.0e-12
                cm[i, b] = _loguniform(rng, 1e-12, 1e-9) if combo in (0, 1) else off
                cw[i, b] = _loguniform(rng, 1e-12, 1e-9) if combo in (0, 2) else off
        alpha = _loguniform(rng, 1e-6, 1.0, (nl, ns))
        lex = np.array(tab["lex"]) - 1
        alpha[:, lex[::7]] = 0.0               # exchanged species without accommodation: x1 = 0
        calls.append(dict(ka=ka, ifeed=ifeed, nkc_l=nkc_l, kw=_kw(rng, kind, nka, nkt, g["kw"]), ff=ff, cw=cw, cm=cm, stokes=stokes,
                          freep=rng.uniform(5e-8, 1.5e-7, nl), alpha=alpha, vmean=rng.uniform(100.0, 1800.0, (nl, ns)),
                          t=rng.uniform(230.0, 300.0, nl), p=rng.uniform(5.0e4, 1.02e5, nl),
                          xkmt0=poison((nl, NKC, ns), 1000.0 + 10000.0 * ci), vt0=poison((nl, NKC), 7.0 + 100.0 * ci), rq=rq))
    return _freeze(calls)


def kmt_bin_cells(c, kc):
    """the [nka, nkt] mask of the grid cells that bin kc (1-based) of call c sums over, and the number of cells the kernel walks for it (rows x nkt)"""
    nka, nkt = c["rq"].shape
    ia0, ia1 = ((2 if c["ifeed"] == 2 else 1), c["ka"]) if kc in (1, 3) else (c["ka"] + 1, nka)
    rows = (np.arange(1, nka + 1) >= ia0) & (np.arange(1, nka + 1) <= ia1)
    jt = np.arange(1, nkt + 1)[None, :]
    cols = jt <= c["kw"][:, None] if kc in (1, 2) else jt > c["kw"][:, None]
    return rows[:, None] & cols, max(0, ia1 - ia0 + 1) * nkt


def kmt_xkmt(mech):
    tab = kmt_py.load(mech)
    return [np.stack([kmt_py.fast_k_mt_layer(tab, c["ff"][i], c["rq"], c["kw"], c["ka"], c["ifeed"], c["nkc_l"], c["cw"][i], c["cm"][i], float(c["freep"][i]),
                                             c["alpha"][i], c["vmean"][i], c["xkmt0"][i]) for i in range(len(c["t"]))]) for c in kmt_calls(mech)]


def kmt_vt(mech):
    tab = kmt_py.load(mech)
    return [np.stack([kmt_py.vt_layer(tab, c["ff"][i], c["rq"], c["kw"], c["ka"], c["ifeed"], c["nkc_l"], c["cw"][i], float(c["t"][i]), float(c["p"][i]),
                                      c["vt0"][i]) for i in range(len(c["t"]))]) for c in kmt_calls(mech)]


@functools.lru_cache(maxsize=None)
def kmt_expected(mech):
    """-> per call (xkmt [nl, nkc, NSPEC], vt [nl, nkc]) after the routine, from the poisoned start"""
    return _freeze(list(zip(kmt_xkmt(mech), kmt_vt(mech))))


# ---------------------------------------------------------------------------------------------------------------- cw_rc, dry_cw_rc
CRYS4 = (0.4, 0.42, 0.7, 0.75)                 # xcryssulf, xcrysss, xdelisulf, xdeliss as captured
CRYS4_SWAPPED = (0.42, 0.4, 0.75, 0.7)         # sea salt crystallising below sulfate: bin 1's "cloud but below its own point" needs it
# (nka, nkt), ka, ifeed, kw kind, crys4, sweep?      rows per chunk = 2048 // nkt
CWRC_CALLS = (
    ((70, 70), 52, 0, "captured", CRYS4, False),         # the model's grid: chunks of 29 rows, the ka boundary inside the second
    ((70, 70), 58, 2, "seeded", CRYS4, False),           # ... and on the edge between the second and the third
    ((1, 1), 0, 0, "zeros", CRYS4, False),               # the smallest grid: its cell in bin 4
    ((1, 1), 1, 0, "full", CRYS4, False),                # ... in bin 1
    ((1, 1), 1, 2, "full", CRYS4, False),                # ... in no bin (ifeed = 2 leaves row 1 out)
    ((64, 32), 32, 0, "seeded", CRYS4, True),            # exactly one chunk; the humidity sweep
    ((65, 32), 64, 2, "seeded", CRYS4, False),           # one row into a second chunk, the ka boundary on the chunk edge
    ((65, 32), 65, 0, "seeded", CRYS4, False),           # ka = nka
    ((37, 53), 0, 0, "seeded", CRYS4, False),            # one ragged chunk (38 rows would fit); ka = 0
    ((37, 53), 20, 2, "seeded", CRYS4_SWAPPED, True),    # the sweep with the crystallisation points swapped
    ((5, 2048), 2, 2, "seeded", CRYS4, False),           # one row per chunk
)


def cwrc_bin_mask(nka, nkt, ka, ifeed, kw, b):
    """[nka, nkt] mask of bin b (0-based; 0, 2: ia <= ka | 1, 3: ia > ka; 0, 1: jt <= kw(ia) | 2, 3: jt > kw(ia))"""
    ia = np.arange(1, nka + 1)
    rows = ((ia >= (2 if ifeed == 2 else 1)) & (ia <= ka)) if b in (0, 2) else (ia > ka)
    jt = np.arange(1, nkt + 1)[None, :]
    cols = jt <= kw[:, None] if b < 2 else jt > kw[:, None]
    return rows[:, None] & cols


def _sweep_feu(crys4):
    out = [0.3, 0.9]
    for th in crys4:
        out += [math.nextafter(th, -math.inf), th, math.nextafter(th, math.inf)]
    return sorted(out)


@functools.lru_cache(maxsize=None)
def cwrc_calls():
    g = np.load(os.path.join(GOLD, "cwrc.npz"))
    rng = np.random.default_rng(9510)
    calls = []
    for (nka, nkt), ka, ifeed, kind, crys4, sweep in CWRC_CALLS:
        model = (nka, nkt) == g["rq"].shape
        rq = np.array(g["rq"]) if model else _loguniform(rng, 0.01, 80.0, (nka, nkt))
        e = np.array(g["e"]) if model else _loguniform(rng, 1e-15, 1e-9, nkt)
        kw = _kw(rng, kind, nka, nkt, g["kw"] if model else None)
        # humidity, cloud flags and the size of each bin's sum, per layer.  kinds: 0 the bin's ff all 0, 1 sum below the threshold, 2 above
        if sweep:
            fs = _sweep_feu(crys4)
            feu = fs + fs + [0.9] * 4
            cloud01 = [(0, i % 2) for i in range(len(fs))] + [(1, (i + 1) % 2) for i in range(len(fs))] + [(1, 1), (1, 0), (0, 1), (0, 0)]
            kinds = [[2] * 4] * (2 * len(fs)) + [[(0, 1, 2, 2)[(i + b) % 4] for b in range(4)] for i in range(4)]
        else:
            feu = [0.3, 0.41, 0.72, 0.9]
            cloud01 = [(1, 1), (1, 0), (0, 1), (0, 0)]
            kinds = [[(0, 1, 2, 2)[(i + b) % 4] for b in range(4)] for i in range(4)]
        nl = len(feu)
        cloud = np.array([[c0, c1, int(rng.integers(0, 2)), int(rng.integers(0, 2))] for c0, c1 in cloud01], np.int32)
        ff = rng.uniform(0.1, 1.0, (nl, nka, nkt)) * (rng.random((nl, nka, nkt)) < 0.8)
        x0 = (4.0 / 3.0 * math.pi) * rq ** 3
        for i in range(nl):
            for b in range(4):
                m = cwrc_bin_mask(nka, nkt, ka, ifeed, kw, b)
                s = float((ff[i] * x0)[m].sum())
                if kinds[i][b] == 0 or s == 0.0:
                    ff[i][m] = 0.0
                else:
                    target = ((0.03, 3.0) if b < 2 else (30.0, 3000.0))[kinds[i][b] - 1]
                    ff[i][m] *= target / s
        calls.append(dict(nka=nka, nkt=nkt, ka=ka, ifeed=ifeed, kw=kw, rq=rq, e=e, crys4=np.array(crys4), ff=ff, feu=np.array(feu), cloud=cloud))
    return _freeze(calls)


@functools.lru_cache(maxsize=None)
def cwrc_expected():
    """-> per call ((rc, cw, cm, conv2 [nl, 4], below [nl]), (rcd, cwd [nl, 2]))"""
    out = []
    for c in cwrc_calls():
        a = (c["rq"], c["e"], c["kw"], c["ka"], c["ifeed"])
        wet = [liq_py.cw_rc_layer(c["ff"][i], *a, float(c["feu"][i]), c["cloud"][i], c["crys4"]) for i in range(len(c["feu"]))]
        dry = [liq_py.cw_rc_layer(c["ff"][i], *a, dry=True) for i in range(len(c["feu"]))]
        w = tuple(np.stack([x[j] for x in wet]) for j in range(4)) + (np.array([x[4] for x in wet], np.int32),)
        d = tuple(np.stack([x[j] for x in dry]) for j in range(2))
        out.append((w, d))
    return _freeze(out)


# ---------------------------------------------------------------------------------------------------------------- dry_rates
DRY_NLAYER = (1, 64, 65, 200)      # one thread per layer in blocks of 64: a single thread, a full block, one thread into a second, a ragged fourth


@functools.lru_cache(maxsize=None)
def dry_cases(mech):
    rng = np.random.default_rng({"gas": 9520, "aer": 9521, "tot": 9522}[mech])
    cases = []
    for nl in DRY_NLAYER:
        rcd = _loguniform(rng, 1e-8, 1e-5, (nl, 2))
        rcd = np.where(rng.random((nl, 2)) < 0.8, rcd, np.where(rng.random((nl, 2)) < 0.5, 0.0, -rcd))
        if nl == 1:
            rcd[0] = (0.0, 3.0e-7)
        cases.append(dict(tt=rng.uniform(200.0, 310.0, nl), freep=rng.uniform(5e-8, 2e-7, nl), rcd=rcd, vmean4=rng.uniform(150.0, 800.0, (nl, 4)),
                          henry4=_signs(rng, (nl, 4), _loguniform(rng, 1e-9, 1e3, (nl, 4)))))
    return _freeze(cases)


def dry_compute(mech):
    """-> flat tuple over the cases: xkmtd [nl, 2, 4], xeq [nl] (, henry4 [nl, 4] for gas)"""
    out = []
    for c in dry_cases(mech):
        rows = [liq_py.dry_rates_layer(float(c["tt"][i]), float(c["freep"][i]), c["rcd"][i], None if mech == "gas" else c["vmean4"][i],
                                       c["henry4"][i] if mech == "gas" else None) for i in range(len(c["tt"]))]
        out.append(tuple(np.stack([np.asarray(r[j]) for r in rows]) for j in range(len(rows[0]))))
    return out


@functools.lru_cache(maxsize=None)
def dry_expected(mech):
    return _freeze(dry_compute(mech))


# ---------------------------------------------------------------------------------------------------------------- henry, v_mean, equil_co
LIQ_NLAYER = (1, 300)
J6 = 55


@functools.lru_cache(maxsize=None)
def liq_cases(mech):
    rng = np.random.default_rng({"aer": 9531, "tot": 9532}[mech])
    ns = nspec(mech)
    cases = []
    for nl in LIQ_NLAYER:
        conv2 = _signs(rng, (nl, NKC), _loguniform(rng, 1e4, 1e8, (nl, NKC)))
        if nl == 1:
            conv2[0] = (3.0e7, 0.0, -2.0e5, 8.0e4)
        cases.append(dict(tt=rng.uniform(200.0, 320.0, nl), conv2=conv2, xgamma=rng.uniform(0.1, 3.0, (nl, NKC, J6)),
                          xkef0=poison((nl, NKC, ns), 2000.0), xkeb0=poison((nl, NKC, ns), 3000.0)))
    return _freeze(cases)


def henry_compute(mech):
    tab = liq_py.load(mech)
    return [np.stack([liq_py.henry_layer(tab, float(t)) for t in c["tt"]]) for c in liq_cases(mech)]


def vmean_compute(mech):
    tab = liq_py.load_vmean(mech)
    return [np.stack([liq_py.v_mean_layer(tab, float(t)) for t in c["tt"]]) for c in liq_cases(mech)]


def equil_compute(mech):
    """-> flat list: xkef, xkeb of case 0, xkef, xkeb of case 1"""
    tab = liq_py.load(mech)
    out = []
    for c in liq_cases(mech):
        rows = [liq_py.equil_co_layer(tab, float(c["tt"][i]), c["conv2"][i], c["xgamma"][i], c["xkef0"][i], c["xkeb0"][i]) for i in range(len(c["tt"]))]
        out += [np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])]
    return out


@functools.lru_cache(maxsize=None)
def liq_expected(mech):
    """-> per case dict(henry, vmean, xkef, xkeb)"""
    h, v, e = henry_compute(mech), vmean_compute(mech), equil_compute(mech)
    return _freeze([dict(henry=h[i], vmean=v[i], xkef=e[2 * i], xkeb=e[2 * i + 1]) for i in range(len(h))])


def henry_exp_species(mech):
    """0-based species whose Henry constant is a temperature law (exp), and those whose constant is a number"""
    ent = liq_py.load(mech)["henry"]["entries"]
    return np.array([j - 1 for j, _, b0 in ent if b0 is not None]), np.array([j - 1 for j, _, b0 in ent if b0 is None])


def equil_exp_species(mech):
    """-> (forward with exp, forward without, backward with, backward without): 0-based species of the routine's entries"""
    ent = liq_py.load(mech)["equil"]["entries"]
    has = lambda prog: any(f[0] == "funa" for f in prog)
    return (np.array([e[0] - 1 for e in ent if has(e[1])]), np.array([e[0] - 1 for e in ent if not has(e[1])]),
            np.array([e[0] - 1 for e in ent if has(e[2])]), np.array([e[0] - 1 for e in ent if not has(e[2])]))


# ---------------------------------------------------------------------------------------------------------------- st_coeff
STC_NLAYER = (1, 300)
STC_SWITCHES = ((False, False), (True, False), (False, True), (True, True))      # lpJoyce14bc, lpBuxmann15alph


def stc_table(mech):
    return json.load(open(os.path.join(REPO, "mistra_amd", "mech", mech + ".stcoeff.json")))


@functools.lru_cache(maxsize=None)
def stc_cases(mech):
    """env [nl, 5] = t, cw(1), cm(1), sion1(13,1), sion1(14,1).  cm(1) is 0 or 0.3 .. 1 of cw(1), the range of the captured layers:
    a_n2o5 forms 1.15e6 - 1.15e6*exp(-0.13*55.55*cm/cw), which cancels — and magnifies the last place of exp without bound — as the ratio goes to 0"""
    rng = np.random.default_rng({"aer": 9541, "tot": 9542}[mech])
    cases = []
    for nl in STC_NLAYER:
        cw1 = np.where(rng.random(nl) < 0.8, _loguniform(rng, 1e-17, 1.2e-9, nl), 0.0)
        cm1 = np.where(rng.random(nl) < 0.8, np.where(cw1 > 0, cw1, 1e-10) * rng.uniform(0.3, 1.0, nl), 0.0)
        s13 = np.where(rng.random(nl) < 0.8, rng.uniform(0.0, 4.5e-10, nl), 0.0)
        s14 = np.where(rng.random(nl) < 0.8, _loguniform(rng, 1e-30, 1.05e-10, nl), 0.0)
        env = np.stack([rng.uniform(230.0, 310.0, nl), cw1, cm1, s13, s14], axis=1)
        if nl == 1:
            env[0, 1:] = (6.0e-10, 4.5e-10, 2.0e-10, 5.0e-11)
        cases.append(env)
    return _freeze(cases)


def stc_compute(mech):
    """-> flat list over (switch setting, case): alpha [nl, NSPEC]"""
    tab = stc_table(mech)
    return [np.stack([rates_py.st_coeff_layer(tab, jo, bu, e) for e in env]) for jo, bu in STC_SWITCHES for env in stc_cases(mech)]


@functools.lru_cache(maxsize=None)
def stc_expected(mech):
    return _freeze(stc_compute(mech))


def stc_plain_species(mech, jo, bu):
    """0-based species whose coefficient involves no library function under that switch setting (min is a comparison)"""
    progs = stc_table(mech)["variants"][int(jo) + 2 * int(bu)]["programs"]
    return np.array([j for j, p in enumerate(progs) if not any(t[0] == "call" and t[1] != "min" for t in p)])
