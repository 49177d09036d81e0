"""Seeded and edge cases for the hand-over halves of the per-layer drivers (mistra_amd/csrc/pack.hip: pack_kernel, unpack_kernel, budgets_kernel), the
run-time species maps behind them (mistra_chem_set_species_maps) and the host gather / scatter of mistra_chem_drive_begin / _end, with the book-keeping
that proves each edge is reached.  The cases of tests/test_drive_cases.py (CPU: the restatement oracle/pack_py.py against the COMPILED bud_x / bud_s_x of the
reference, the order of every product, the edge table, the facts about the tables the kernels rely on) and of tests/test_gpu_drive_edges.py (the device).
Plain module, no GPU; everything is cached and read-only like tests/rates_cases.py.

BUDGET STATES  (budget_cases)  NB seeded states per mechanism — C = VAR || FIX, RCONST, the cumulative columns — and named edge states cut from one
  ordinary state.  A seeded value is (1 + m / 2^52) * 2^e with 52 random mantissa bits and e the sum of four uniform integers in [-12, 12]: bell-shaped
  over ~29 decades like a log-normal, every mantissa full so that products round, and made of integer draws only — no exp, no log: the same bytes on every
  machine (INPUT_SHA256 in the fixture holds them).  bud_x forms RCONST(i)*f1*f2*..; with full mantissas another order of the factors gives other bits on
  about every second state, so NB states tell EVERY other order of EVERY multi-factor reaction apart (condition (a) of tests/test_drive_cases.py).
PACK LAYERS    (pack_cases)    row 0 of tests/golden/drive_<mech>.npz with one edge set by name: every cvv bin on and around the `cvv > 0` select, air / h2o
  zero and negative, sl1 / sion1 under the clamps, a hand-over state with -0.0 / NaN / negative on every entry the hand-over list reads.
SPECIES MAPS   (map_sets, refusal_sets, refusal_of)  legal maps other than the capture's, and maps that differ from a legal one in ONE mapped species and
  must be refused, each with the text of its refusal; refusal_of restates the five checks of mistra_chem_set_species_maps in their order.

Expected values: oracle/pack_py.py for pack and hand-over (MAX(0.d0,x) and the cvv select as flang compiles them: NaN, -0.0 and negative cvv all take the
ELSE branch of `if (cvv1.gt.0)`, tot.f:229-248); the budgets from the compiled reference (tests/golden/drive_edges_<mech>.npz, written by
tests/golden/make_drive_edges_golden.py)."""
import functools
import hashlib
import itertools
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle import pack_py      # noqa: E402
from mistra_amd.mechtab import load as load_mech      # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MECHS = ("gas", "aer", "tot")
SEED = 20261018
NB = 24                   # seeded budget states per mechanism (condition (a) holds with this seed: tests/test_drive_cases.py)
NBGS = 122                # bgs(2,122,n), bud_s_g.f:63
NEG = -1.5e-9             # a concentration after a small undershoot of the integrator
# the unset slot: inside an accumulated range of bud_s_x but set by no term (bud_s_a.f, bud_s_t.f): it accumulates what the caller's bgs(1,slot) holds
UNSET_SLOTS = {"gas": (), "aer": (116,), "tot": (74,)}
CVV_KINDS = (("0.0", 0.0), ("-0.0", -0.0), ("-1e-3", -1.0e-3), ("NaN", math.nan), ("+Inf", math.inf), ("5e-324", 5.0e-324), ("1e-310", 1.0e-310))
# the refusals of mistra_chem_set_species_maps (mistra_amd/csrc/capi.cpp), in the order it checks
REFUSE_RANGE = "species map entry out of range"
REFUSE_TWICE = "a species is mapped twice"
REFUSE_INVERSE = "are not inverse to each other"
REFUSE_PACKED = "is also packed from sl1 / sion1"


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


@functools.lru_cache(maxsize=None)
def table(mech):
    return pack_py.load(mech)


@functools.lru_cache(maxsize=None)
def capture(mech):
    return _freeze(dict(np.load(os.path.join(GOLD, "drive_%s.npz" % mech))))


def same(a, b):
    """NaN in the same places, every other entry the same BITS, the sign of a zero included (the same() of tests/test_gpu_pack.py)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def where_differ(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return (na != nb) | (~na & ~nb & (a.view(np.uint64) != b.view(np.uint64)))


def seeded(rng, shape):
    """(1 + m/2^52) * 2^e, e the sum of four uniform integers in [-12, 12] (the module's docstring): integer draws only"""
    m = rng.integers(0, 1 << 52, size=shape, dtype=np.int64)
    e = rng.integers(-12, 13, size=(4,) + tuple(np.atleast_1d(shape)), dtype=np.int64).sum(axis=0)
    return np.ldexp(1.0 + m.astype(np.float64) / float(1 << 52), e.astype(np.int32))      # (m < 2^52: the quotient and the sum are exact)


def poison(shape, k=0):
    """a value of its own per entry, negative and far from anything a case computes: what an entry nobody may write must still hold afterwards"""
    n = int(np.prod(shape))
    return -(7.25 + 4096.0 * k + np.arange(n, dtype=np.float64)).reshape(shape)


def scalars(mech, args):
    """[6] = air, h2o, cvv1..4 and dt from a driver's argument list (gas.f:60-61 | aer.f:59-61 | tot.f:59-61)"""
    sc = np.zeros(6)
    if mech == "gas":
        sc[0], sc[1] = args[6], args[7]
    elif mech == "aer":
        sc[0], sc[1], sc[2:4] = args[10], args[11], args[2:4]
    else:
        sc[0], sc[1], sc[2:6] = args[14], args[15], args[2:6]
    return sc, float(args[1])


# ---------------------------------------------------------------------------------------------------------------- budget states
def factors(mech, r):
    """0-based indices into C || consts of reaction r's rate product, in the table's (= Fun_x's = bud_x's) order"""
    t = load_mech(mech)
    return [int(f) for f in t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]]]


@functools.lru_cache(maxsize=None)
def multi_factor_reactions(mech):
    """[(r, other orders)]: reactions with at least two DISTINCT factors and every order of them that is not the table's"""
    out = []
    for r in range(load_mech(mech).nreact):
        f = tuple(factors(mech, r))
        if len(set(f)) >= 2:
            out.append((r, tuple(sorted(set(itertools.permutations(f)) - {f}))))
    return out


@functools.lru_cache(maxsize=None)
def edge_species(mech):
    """what the named states override: `hot` the variable species in most rate products; (ra, a, b) a reaction of two distinct variable factors for the
    products that leave the number range in bg; (rs, sa, sb) the same for bgs: slot 1's term RCONST(rs)*C(sa)*C(sb).  All 0-based."""
    t, tab = load_mech(mech), table(mech)
    hot = int(np.bincount(t.a_fac[t.a_fac < t.nvar], minlength=t.nvar).argmax())
    slot, terms = tab["bud_s"][0]
    sign, rs, cs = terms[0]
    assert slot == 1 and sign > 0 and len(cs) == 2 and cs[0] != cs[1]
    avoid = {hot, cs[0] - 1, cs[1] - 1}
    ra = next(r for r in range(t.nreact) if len(factors(mech, r)) == 2 and len(set(factors(mech, r))) == 2 and max(factors(mech, r)) < t.nvar
              and not set(factors(mech, r)) & avoid and r != rs - 1)
    return dict(hot=hot, ra=ra, a=factors(mech, ra)[0], b=factors(mech, ra)[1], rs=rs - 1, sa=cs[0] - 1, sb=cs[1] - 1)


@functools.lru_cache(maxsize=None)
def budget_cases(mech):
    """-> dict(names [n], C [n, nvar+nfix], rconst [n, nreact], dt [n], bg_in [n, nreact, 2], bgs_in [n, 122, 2])"""
    t = load_mech(mech)
    nspec, nr = t.nvar + t.nfix, t.nreact
    rng = np.random.default_rng([SEED, MECHS.index(mech)])
    names, C, K, dt, bg, bgs = [], [], [], [], [], []

    def add(name, c, k, d, b, s):
        names.append(name); C.append(c); K.append(k); dt.append(d); bg.append(b); bgs.append(s)

    sign = lambda shape: 1.0 - 2.0 * rng.integers(0, 2, size=shape)
    for i in range(NB):      # cumulative columns: zero in every third state, seeded in the others; bgs(1,:) always seeded (the unset slot carries it)
        c, k = seeded(rng, nspec), seeded(rng, nr)
        b, s = np.zeros((nr, 2)), np.zeros((NBGS, 2))
        b[:, 0], s[:, 0] = seeded(rng, nr), seeded(rng, NBGS) * sign(NBGS)
        cum_b, cum_s = seeded(rng, nr), seeded(rng, NBGS) * sign(NBGS)
        if i % 3:
            b[:, 1], s[:, 1] = cum_b, cum_s
        add("seeded %d" % i, c, k, 10.0, b, s)
    e = edge_species(mech)
    c0, k0 = C[0], K[0]
    zb, zs = np.zeros((nr, 2)), np.zeros((NBGS, 2))

    def named(name, over_c=(), over_k=(), d=10.0, b=zb, s=zs):
        c, k = c0.copy(), k0.copy()
        for i, v in over_c:
            c[i] = v
        for i, v in over_k:
            k[i] = v
        add(name, c, k, d, b, s)

    named("ordinary")
    for nm, v in (("+0.0", 0.0), ("-0.0", -0.0), ("<0", NEG), ("NaN", math.nan)):
        named("C(%d)=%s" % (e["hot"] + 1, nm), [(e["hot"], v)])
    named("RCONST(%d)=Inf" % (e["rs"] + 1), over_k=[(e["rs"], math.inf)])
    named("RCONST(%d)=Inf dt=0" % (e["rs"] + 1), over_k=[(e["rs"], math.inf)], d=0.0)
    pair = lambda x, y: [(e["a"], x), (e["b"], y), (e["sa"], x), (e["sb"], y)]
    one = [(e["ra"], 1.0), (e["rs"], 1.0)]
    named("product subnormal", pair(1.0e-160, 1.0e-155), one)
    named("product underflows to 0", pair(1.0e-160, 1.0e-170), one)
    named("product overflows", pair(1.0e160, 1.0e155), one)
    named("dt=0", d=0.0)
    named("dt=0.1", d=0.1)
    fb, fs = zb.copy(), zs.copy()
    fb[:, 1], fs[:, 1] = math.inf, math.inf
    named("cumulative=Inf", b=fb, s=fs)
    for slot in UNSET_SLOTS[mech]:
        s = zs.copy()
        s[slot - 1, 0] = 3.25
        named("bgs(1,%d)=3.25 on entry" % slot, s=s)
    assert len(set(names)) == len(names)
    return _freeze(dict(names=names, C=np.stack(C), rconst=np.stack(K), dt=np.array(dt), bg_in=np.stack(bg), bgs_in=np.stack(bgs)))


def input_sha256(mech):
    c = budget_cases(mech)
    h = hashlib.sha256()
    for key in ("C", "rconst", "dt", "bg_in", "bgs_in"):
        h.update(np.ascontiguousarray(c[key], "<f8").tobytes())
    return h.hexdigest()


def fixture(mech):
    return np.load(os.path.join(GOLD, "drive_edges_%s.npz" % mech))


@functools.lru_cache(maxsize=None)
def expected_budgets(mech):
    """-> (bg [n, nreact, 2], bgs [n, 122, 2]) as the COMPILED reference left them.  Where the fixture holds the instantaneous column of bg only (`bg1`: the
    file would have outgrown drive_<mech>.npz), the cumulative one is in + dt*inst: one multiply, one add, exact in numpy — the generator asserted that
    the reference's own column is these bits before it dropped it."""
    fx, c = fixture(mech), budget_cases(mech)
    if "bg" in fx.files:
        bg = fx["bg"]
    else:
        with np.errstate(all="ignore"):
            bg = np.stack([fx["bg1"], c["bg_in"][:, :, 1] + c["dt"][:, None] * fx["bg1"]], axis=2)
    return _freeze((bg, fx["bgs"]))


@functools.lru_cache(maxsize=None)
def restated_budgets(mech):
    c, tab, t = budget_cases(mech), table(mech), load_mech(mech)
    with np.errstate(all="ignore"):
        out = [pack_py.budgets(tab, t, c["C"][i], c["rconst"][i], float(c["dt"][i]), c["bg_in"][i], c["bgs_in"][i]) for i in range(len(c["names"]))]
    return _freeze((np.stack([o[0] for o in out]), np.stack([o[1] for o in out])))


def product(mech, order, C, K, r):
    """RCONST(r) * factors in `order`, left to right, over all states at once: [n]"""
    X = np.concatenate([C, np.broadcast_to(load_mech(mech).consts, (C.shape[0], load_mech(mech).nconst))], axis=1)
    p = K[:, r].copy()
    with np.errstate(all="ignore"):
        for f in order:
            p = p * X[:, f]
    return p


def orders_not_told_apart(mech):
    """condition (a): [(reaction number, 1-based; order)] for which NO state gives other bits than the table's order"""
    c = budget_cases(mech)
    left = []
    for r, others in multi_factor_reactions(mech):
        base = product(mech, factors(mech, r), c["C"], c["rconst"], r)
        for o in others:
            if not where_differ(base, product(mech, o, c["C"], c["rconst"], r)).any():
                left.append((r + 1, o))
    return left


def _subnormal(x):
    return (x != 0.0) & (np.abs(x) < np.finfo(np.float64).tiny)


def budget_reach(mech):
    """{edge: [names of the states that reach it]}, counted where the edge acts: in the rate products of bg and in the terms of bgs"""
    c, tab, t = budget_cases(mech), table(mech), load_mech(mech)
    bg, bgs = restated_budgets(mech)
    e = edge_species(mech)
    out = {}
    hit = lambda edge, i: out.setdefault(edge, []).append(c["names"][i])
    for edge in ("species +0.0", "species -0.0", "species < 0", "species NaN", "Inf rate constant", "bg: product subnormal", "bg: product underflows to 0",
                 "bg: product overflows", "bg: product NaN", "bgs: term subnormal", "bgs: term underflows to 0", "bgs: term overflows", "bgs: NaN",
                 "dt = 10", "dt = 0", "dt = 0.1", "cumulative from 0", "cumulative from seeded values", "cumulative from Inf", "0 * Inf: NaN accumulated",
                 "unset accumulated slot carries a non-zero value"):
        out[edge] = []
    uses_hot = [r for r in range(t.nreact) if e["hot"] in factors(mech, r)]
    for i in range(len(c["names"])):
        C, K, d = c["C"][i], c["rconst"][i], float(c["dt"][i])
        X = np.concatenate([C, t.consts])
        h, inst = C[e["hot"]], bg[i, :, 0]
        live = np.array([all(X[f] != 0.0 and np.isfinite(X[f]) for f in factors(mech, r)) and K[r] != 0.0 and np.isfinite(K[r]) for r in range(t.nreact)])
        if h == 0.0 and not np.signbit(h) and all(inst[r] == 0.0 for r in uses_hot): hit("species +0.0", i)
        if h == 0.0 and np.signbit(h) and any(np.signbit(inst[r]) for r in uses_hot): hit("species -0.0", i)      # (the sign reaches bg)
        if h < 0.0 and all(inst[r] < 0.0 for r in uses_hot if factors(mech, r).count(e["hot"]) == 1): hit("species < 0", i)
        if np.isnan(h) and all(np.isnan(inst[r]) for r in uses_hot): hit("species NaN", i)
        if np.isinf(K).any() and np.isinf(inst[np.isinf(K)]).all(): hit("Inf rate constant", i)
        if (live & _subnormal(inst)).any(): hit("bg: product subnormal", i)
        if (live & (inst == 0.0)).any(): hit("bg: product underflows to 0", i)
        if (live & np.isinf(inst)).any(): hit("bg: product overflows", i)
        if np.isnan(inst).any(): hit("bg: product NaN", i)
        sa, sb, rs = C[e["sa"]], C[e["sb"]], K[e["rs"]]
        first = bgs[i, 0, 0]      # slot 1 = RCONST(rs)*C(sa)*C(sb), one term
        fin = all(v != 0.0 and np.isfinite(v) for v in (sa, sb, rs))
        if fin and _subnormal(first): hit("bgs: term subnormal", i)
        if fin and first == 0.0: hit("bgs: term underflows to 0", i)
        if fin and np.isinf(first): hit("bgs: term overflows", i)
        if np.isnan(bgs[i]).any(): hit("bgs: NaN", i)
        hit({10.0: "dt = 10", 0.0: "dt = 0", 0.1: "dt = 0.1"}[d], i)
        zero_b, zero_s = not c["bg_in"][i, :, 1].any(), not c["bgs_in"][i, :, 1].any()
        if zero_b and zero_s: hit("cumulative from 0", i)
        if np.isinf(c["bg_in"][i, :, 1]).all() and np.isinf(c["bgs_in"][i, :, 1]).all(): hit("cumulative from Inf", i)
        elif c["bg_in"][i, :, 1].all() and c["bgs_in"][i, :, 1].all(): hit("cumulative from seeded values", i)
        if d == 0.0 and np.isinf(inst).any() and np.isnan(bg[i, np.isinf(inst), 1]).all(): hit("0 * Inf: NaN accumulated", i)
        for slot in UNSET_SLOTS[mech]:
            v = c["bgs_in"][i, slot - 1, 0]
            if v != 0.0 and bgs[i, slot - 1, 0] == v and bgs[i, slot - 1, 1] == c["bgs_in"][i, slot - 1, 1] + d * v: hit("unset accumulated slot carries a non-zero value", i)
    if not UNSET_SLOTS[mech]:
        del out["unset accumulated slot carries a non-zero value"]
    return out


# ---------------------------------------------------------------------------------------------------------------- pack layers
def cvv_bins(mech):
    """the liquid-water bins the mechanism's fix list reads (1-based)"""
    return sorted(kc for _, kind, kc in table(mech)["fix"] if kind not in ("O2", "N2", "H2O"))


def arrays_read(mech):
    """which of sl1 / sion1 the pack half reads or clamps"""
    tab = table(mech)
    return ("sl1", "sion1") if tab["preclamp"] else tuple(sorted({arr for _, arr, _, _, _ in tab["pack"]}))


def handover_clamped(mech):
    """C indices (1-based) whose hand-over to sl1 / sion1 is clamped"""
    return sorted({c for _, _, _, c, cl in table(mech)["unpack"] if cl})


@functools.lru_cache(maxsize=None)
def pack_cases(mech):
    """-> dict(names [n], s1, s3, sl1, sion1, scal [n, 6], c_prev, c_out [n, nvar+nfix]): row 0 of the capture, one edge per layer.  c_prev is what the
    arrays of C hold when the pack runs (entries the driver does not set keep it: poison), c_out the state the hand-over reads."""
    g, tab = capture(mech), table(mech)
    sc0, _ = scalars(mech, g["args"][0])
    bins = cvv_bins(mech)
    assert all(sc0[1 + kc] > 0.0 and np.isfinite(sc0[1 + kc]) for kc in bins) and sc0[0] > 0.0 and sc0[1] > 0.0      # an ORDINARY layer
    # c_prev: a poison of its own in every entry, so that an entry the tables do not name shows as kept and a missed assignment shows as poison
    base = dict(s1=g["s1_in"][0], s3=g["s3_in"][0], sl1=g["sl1_in"][0], sion1=g["sion1_in"][0], scal=sc0, c_prev=poison(g["c_in"].shape[1]), c_out=g["c_out"][0])
    names, rows = [], []

    def add(name, **over):
        names.append(name)
        rows.append({k: np.array(over.get(k, v), np.float64) for k, v in base.items()})

    def scal(over):      # {index into [air, h2o, cvv1..4]: value}
        s = sc0.copy()
        for j, v in over.items():
            s[j] = v
        return s

    add("ordinary")
    for nm, v in CVV_KINDS:
        for kc in bins:
            add("cvv%d=%s" % (kc, nm), scal=scal({1 + kc: v}))
        if bins:
            add("cvv*=%s" % nm, scal=scal({1 + kc: v for kc in bins}))
    add("air=0", scal=scal({0: 0.0}))
    add("air<0", scal=scal({0: -1.0}))
    add("h2o=0", scal=scal({1: 0.0}))
    add("h2o<0", scal=scal({1: -1.0e-3}))
    edged = {}
    for key in ("sl1", "sion1"):
        a = base[key].copy()
        a[0::4], a[1::4], a[2::4] = -0.0, math.nan, NEG
        edged[key] = a
    add("sl1, sion1: every fourth entry -0.0, NaN, negative", **edged)
    add("sl1 = sion1 = 0", sl1=np.zeros_like(base["sl1"]), sion1=np.zeros_like(base["sion1"]))
    c_out = base["c_out"].copy()
    reads = np.array(sorted({c for _, _, _, c, _ in tab["unpack"]})) - 1
    c_out[reads[0::3]], c_out[reads[1::3]], c_out[reads[2::3]] = -0.0, math.nan, -2.0e-12
    add("hand-over of -0.0, NaN, negative", c_out=c_out)
    out = {k: np.stack([r[k] for r in rows]) for k in base}
    out["names"] = names
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def restated_pack(mech):
    """-> dict(C, sl1, sion1 after the pack; s1, s3, sl1_out, sion1_out after the hand-over of c_out) of every pack layer, by the restatement"""
    g, tab, p = capture(mech), table(mech), pack_cases(mech)
    m2k, k2m, rm2k, rk2m = map_sets(mech)["capture"]      # (the layers carry the capture's s1 / s3; synthetic maps: map_layer)
    out = {k: [] for k in ("C", "sl1", "sion1", "s1", "s3", "sl1_out", "sion1_out")}
    for i in range(len(p["names"])):
        with np.errstate(all="ignore"):      # (55.55 / subnormal overflows: that is the case)
            C, L, I = pack_py.pack(tab, p["c_prev"][i], p["s1"][i], p["s3"][i], p["sl1"][i], p["sion1"][i], p["scal"][i, 0], p["scal"][i, 1], p["scal"][i, 2:6], m2k, rm2k)
        s1, s3, L2, I2 = pack_py.unpack(tab, p["c_out"][i], p["s1"][i], p["s3"][i], L, I, k2m, rk2m)
        for k, v in zip(out, (C, L, I, s1, s3, L2, I2)):
            out[k].append(v)
    return _freeze({k: np.stack(v) for k, v in out.items()})


def pack_reach(mech):
    """{edge: [layers that reach it]}, counted where the edge acts: on the FIX entry a cvv feeds, on the C entries and model arrays under a clamp"""
    tab, p, r = table(mech), pack_cases(mech), restated_pack(mech)
    out = {}
    hit = lambda edge, i: out.setdefault(edge, []).append(p["names"][i])
    kind_of = {"0.0": lambda v: v == 0.0 and not np.signbit(v), "-0.0": lambda v: v == 0.0 and np.signbit(v), "-1e-3": lambda v: v < 0.0, "NaN": np.isnan,
               "+Inf": lambda v: v == math.inf, "5e-324": lambda v: v == 5.0e-324, "1e-310": lambda v: v == 1.0e-310}
    # what the select leaves in FIX: +0.0 from the ELSE branch; 55.55/Inf = +0.0 and 55.55/subnormal = Inf from the THEN branch
    result = {"0.0": 0.0, "-0.0": 0.0, "-1e-3": 0.0, "NaN": 0.0, "+Inf": 0.0, "5e-324": math.inf, "1e-310": math.inf}
    fix_of = {kc: c for c, kind, kc in tab["fix"] if kind not in ("O2", "N2", "H2O")}
    for kc in cvv_bins(mech):
        for nm, _ in CVV_KINDS:
            out["cvv%d %s" % (kc, nm)] = []
        out["cvv%d > 0, finite quotient" % kc] = []
    for key in arrays_read(mech):
        for what in ("negative clamped to +0.0", "-0.0 kept", "NaN kept"):
            out["%s %s in C" % (key, what)] = []
            if tab["preclamp"]:
                out["%s %s in the model array" % (key, what)] = []
    for edge in ("air = 0", "air < 0", "h2o = 0", "h2o < 0", "sl1 = sion1 = 0", "hand-over reads -0.0", "hand-over reads NaN", "hand-over reads a negative value"):
        out[edge] = []
    o2 = next(c for c, kind, _ in tab["fix"] if kind == "O2")
    h2 = next(c for c, kind, _ in tab["fix"] if kind == "H2O")
    for i in range(len(p["names"])):
        C = r["C"][i]
        for kc in cvv_bins(mech):
            v, f = p["scal"][i, 1 + kc], C[fix_of[kc] - 1]
            for nm, _ in CVV_KINDS:
                if kind_of[nm](v) and f == result[nm] and not np.signbit(f):
                    hit("cvv%d %s" % (kc, nm), i)
            if v > 0.0 and np.isfinite(f) and f > 0.0:
                hit("cvv%d > 0, finite quotient" % kc, i)
        src = {"sl1": p["sl1"][i], "sion1": p["sion1"][i]}
        got = dict(neg=set(), mz=set(), nan=set())
        for c, arr, k, kc, clamp in tab["pack"]:
            v, w = src[arr][pack_py.flat(tab, arr, k, kc)], C[c - 1]
            if not (clamp or tab["preclamp"]):
                continue
            if v < 0.0 and w == 0.0 and not np.signbit(w): got["neg"].add(arr)
            if v == 0.0 and np.signbit(v) and w == 0.0 and np.signbit(w): got["mz"].add(arr)
            if np.isnan(v) and np.isnan(w): got["nan"].add(arr)
        for key in arrays_read(mech):
            for k, what in (("neg", "negative clamped to +0.0"), ("mz", "-0.0 kept"), ("nan", "NaN kept")):
                if key in got[k]: hit("%s %s in C" % (key, what), i)
            if tab["preclamp"]:
                a, b = src[key], r[key][i]
                if ((a < 0.0) & (b == 0.0) & ~np.signbit(b)).any(): hit("%s negative clamped to +0.0 in the model array" % key, i)
                if ((a == 0.0) & np.signbit(a) & (b == 0.0) & np.signbit(b)).any(): hit("%s -0.0 kept in the model array" % key, i)
                if (np.isnan(a) & np.isnan(b)).any(): hit("%s NaN kept in the model array" % key, i)
        air, h2o = p["scal"][i, 0], p["scal"][i, 1]
        if air == 0.0 and C[o2 - 1] == 0.0: hit("air = 0", i)
        if air < 0.0 and C[o2 - 1] < 0.0: hit("air < 0", i)
        if h2o == 0.0 and C[h2 - 1] == 0.0: hit("h2o = 0", i)
        if h2o < 0.0 and C[h2 - 1] == h2o: hit("h2o < 0", i)
        if not p["sl1"][i].any() and not p["sion1"][i].any() and all(C[c - 1] == 0.0 for c, *_ in tab["pack"]): hit("sl1 = sion1 = 0", i)
        rd = p["c_out"][i][np.array(sorted({c for _, _, _, c, _ in tab["unpack"]})) - 1]
        if ((rd == 0.0) & np.signbit(rd)).any(): hit("hand-over reads -0.0", i)
        if np.isnan(rd).any(): hit("hand-over reads NaN", i)
        if (rd < 0.0).any(): hit("hand-over reads a negative value", i)
    return out


# ---------------------------------------------------------------------------------------------------------------- species maps
def _ints(*a):
    return tuple(np.array(x, np.int32).reshape(shape) for x, shape in zip(a, ((-1, 2), (-1,), (-1, 2), (-1,))))


@functools.lru_cache(maxsize=None)
def map_sets(mech):
    """{name: (gas_m2k [j1, 2] = (C index, source index) pairs, gas_k2m [j1], rad_m2k [j5, 2], rad_k2m [j5])}, 1-based as the C ABI takes them: legal maps"""
    g, tab = capture(mech), table(mech)
    nvar = tab["nvar"]
    j1 = len(g["gas_k2m"])
    out = {"capture": _ints(g["gas_m2k"], g["gas_k2m"], g["rad_m2k"], g["rad_k2m"])}
    rev = g["gas_m2k"].copy()
    rev[:, 1] = j1 + 1 - rev[:, 1]
    out["s1 reversed"] = _ints(rev, g["gas_k2m"][::-1], g["rad_m2k"], g["rad_k2m"])
    packed = {c for c, *_ in tab["pack"]}
    free = [c for c in range(1, nvar + 1) if c not in packed]
    out["j1 = 1, j5 = 0"] = _ints([[free[-1], 1]], [free[-1]], [], [])
    out["j1 = j5 = 0"] = _ints([], [], [], [])
    n = len(free)      # the largest legal j1: every variable species the pack list does not set, sources in descending order
    out["largest j1, j5 = 0"] = _ints([[c, n - j] for j, c in enumerate(free)], free[::-1], [], [])
    return _freeze(out)


def refusal_of(mech, maps):
    """None for maps mistra_chem_set_species_maps takes, else the text of its refusal: the five checks in its order (mistra_amd/csrc/capi.cpp) — what makes
    the kernel's PARALLEL assignments equal to the reference's sequential ones"""
    m2k, k2m, rm2k, rk2m = maps
    tab = table(mech)
    nvar, seen = tab["nvar"], set()
    for m, k in ((m2k, k2m), (rm2k, rk2m)):
        for c, src in np.asarray(m).reshape(-1, 2).tolist():
            if c < 1 or c > nvar or src < 1 or src > len(k):
                return REFUSE_RANGE
            if c in seen:
                return REFUSE_TWICE
            seen.add(c)
            if k[src - 1] != c:
                return REFUSE_INVERSE
    if seen & {c for c, *_ in tab["pack"] if c <= nvar}:
        return REFUSE_PACKED
    return None


@functools.lru_cache(maxsize=None)
def refusal_sets(mech):
    """[(name, text of the refusal, maps)]: the capture's maps with ONE mapped species changed (its gas_m2k pair; where the set is about something else than
    the inverse, gas_k2m follows so that the inverse check is not what refuses)"""
    tab = table(mech)
    nvar = tab["nvar"]
    good = map_sets(mech)["capture"]
    j1 = len(good[1])
    out = []

    def add(name, text, edit):
        m2k, k2m, rm2k, rk2m = (a.copy() for a in good)
        edit(m2k, k2m)
        out.append((name, text, (m2k, k2m, rm2k, rk2m)))

    def set_c(v, follow=True):
        def edit(m2k, k2m):
            m2k[0, 0] = v
            if follow:
                k2m[m2k[0, 1] - 1] = v
        return edit

    def set_src(v):
        def edit(m2k, k2m):
            m2k[0, 1] = v
        return edit
    add("C index 0", REFUSE_RANGE, set_c(0))
    add("C index nvar + 1", REFUSE_RANGE, set_c(nvar + 1))
    add("source index 0", REFUSE_RANGE, set_src(0))
    add("source index j1 + 1", REFUSE_RANGE, set_src(j1 + 1))
    add("one species twice", REFUSE_TWICE, lambda m2k, k2m: set_c(int(m2k[0, 0]))(m2k[::-1], k2m))      # the LAST pair names the first pair's species
    add("gas_k2m not the inverse", REFUSE_INVERSE, lambda m2k, k2m: k2m.__setitem__(int(m2k[0, 1]) - 1, int(m2k[1, 0])))
    packed = sorted(c for c, *_ in tab["pack"] if c <= nvar)
    add("a species the pack list also sets", REFUSE_PACKED, set_c(packed[0]))
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def map_layer(mech, name):
    """one ordinary layer under a legal map set -> dict(inputs; restated C, sl1, sion1, s1, s3, sl1_out, sion1_out): s1 / s3 seeded at the set's own widths
    (one poisoned entry where the width is 0: the arrays must then be neither read nor written)"""
    tab, p = table(mech), pack_cases(mech)
    m2k, k2m, rm2k, rk2m = map_sets(mech)[name]
    rng = np.random.default_rng([SEED, 100 + MECHS.index(mech), list(map_sets(mech)).index(name)])
    s1, s3 = seeded(rng, len(k2m)), seeded(rng, len(rk2m))
    C, L, I = pack_py.pack(tab, p["c_prev"][0], s1, s3, p["sl1"][0], p["sion1"][0], p["scal"][0, 0], p["scal"][0, 1], p["scal"][0, 2:6], m2k.tolist(), rm2k.tolist())
    o1, o3, L2, I2 = pack_py.unpack(tab, p["c_out"][0], s1, s3, L, I, k2m.tolist(), rk2m.tolist())
    return _freeze(dict(s1=s1, s3=s3, sl1=p["sl1"][0], sion1=p["sion1"][0], scal=p["scal"][0], c_prev=p["c_prev"][0], c_out=p["c_out"][0],
                        C=C, L=L, I=I, s1_out=o1, s3_out=o3, L_out=L2, I_out=I2))
