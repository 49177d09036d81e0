"""The cases of tests/drive_cases.py on the device (-m gpu): budgets_kernel against what the COMPILED bud_x / bud_s_x of the reference made of the same states
(tests/golden/drive_edges_<mech>.npz), pack_kernel and unpack_kernel against the restatement oracle/pack_py.py on the edge layers and under legal species
maps other than the capture's, the refusals of mistra_chem_set_species_maps, and the host gather / scatter of mistra_chem_drive_begin / _end in the layouts
and layer lists the captured column steps never use.  Every comparison is bit for bit: NaN in the same places, every other entry the same bits, signs of
zeros included (drive_cases.same).  Every output array is the caller's with one row more than the call covers, a poison of its own in every entry
beforehand: the extra row and every entry the tables do not name must still hold it.

The budget states are NOT repeated through mistra_chem_drive_device: the chain integrates before it budgets, and a state with NaN, Inf or products outside
the number range is no input for INTEGRATE_x.  The chain's budgets stay with tests/test_gpu_pack.py and tests/test_gpu_drive.py (captured calls), which run
the same budgets_kernel.  What flang makes of `if (cvv1.gt.0)` settles the cvv edges: NaN, -0.0 and negative take the ELSE branch (FIX = 0.), +Inf gives
55.55/Inf = 0., a subnormal gives Inf; the kernel's `sc > 0.0 ? 55.55/sc : 0.0` must do the same."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import drive_cases as dc
from conftest import REPO
from oracle import pack_py

pytestmark = pytest.mark.gpu
NENV = {"gas": 74, "aer": 330, "tot": 544}
N, NLEV = 150, 15      # global_params.f90: n, nlev


@pytest.fixture(scope="module")
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    return c


def _dev():
    import torch
    return torch.device("cuda", 0)


def T(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=_dev())


def with_extra_row(a, k):
    """rows of `a` plus one poisoned row behind them"""
    a = np.asarray(a, np.float64)
    a = a.reshape(a.shape[0], -1)
    return np.concatenate([a, dc.poison((1, a.shape[1]), k)])


def set_maps(chem, mech, maps):
    chem.set_species_maps(mech, *maps)


# ---------------------------------------------------------------------------------------------------------------- budgets
def _budgets(chem, mech, rows, dt, want_bg, want_bgs):
    """budgets_kernel on the states `rows` (one batch) -> (bg [len(rows), nreact, 2] | None, bgs | None); the row behind the batch must keep its poison"""
    import torch
    c = dc.budget_cases(mech)
    nv = dc.table(mech)["nvar"]
    rows = np.asarray(rows)
    bg = T(with_extra_row(c["bg_in"][rows], 1)) if want_bg else None
    bgs = T(with_extra_row(c["bgs_in"][rows], 2)) if want_bgs else None
    chem.budgets(mech, T(c["C"][rows][:, :nv]), T(c["C"][rows][:, nv:]), T(c["rconst"][rows]), dt, bg, bgs)
    torch.cuda.synchronize()
    out = []
    for t, k in ((bg, 1), (bgs, 2)):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert np.array_equal(a[-1:], dc.poison((1, a.shape[1]), k)), "the row behind the batch was written"
        out.append(a[:-1].reshape(len(rows), -1, 2))
    return out


@pytest.mark.parametrize("mech", dc.MECHS)
def test_budgets_kernel_against_the_compiled_reference(chem, mech):
    """all states of one dt in one batch; the same rows reversed with one more behind them (ncase + 1 cells); every state alone; bg only, bgs only, both"""
    c = dc.budget_cases(mech)
    assert str(dc.fixture(mech)["input_sha256"]) == dc.input_sha256(mech)
    want_bg, want_bgs = dc.expected_budgets(mech)
    set_maps(chem, mech, dc.map_sets(mech)["capture"])      # (the budgets need the hand-over tables, not the maps; a library fresh from init has none)

    def check(rows, got, what):
        for a, want, name in ((got[0], want_bg, "bg"), (got[1], want_bgs, "bgs")):
            if a is None:
                continue
            for j, i in enumerate(rows):
                bad = np.nonzero(dc.where_differ(a[j], want[i]).any(axis=1))[0]
                assert bad.size == 0, "%s, %s, state %r: %s entries %s (numbered from 1) differ from the compiled reference's" % (
                    mech, what, c["names"][i], name, (bad[:8] + 1).tolist())

    nbatch = 0
    for dt in sorted(set(c["dt"].tolist())):
        rows = np.nonzero(c["dt"] == dt)[0]
        for bg, bgs in ((True, True), (True, False), (False, True)):
            check(rows, _budgets(chem, mech, rows, dt, bg, bgs), "one batch (bg %s, bgs %s)" % (bg, bgs))
            more = np.concatenate([rows[::-1], rows[:1]])
            check(more, _budgets(chem, mech, more, dt, bg, bgs), "reversed, one more cell (bg %s, bgs %s)" % (bg, bgs))
            nbatch += 2
        for i in rows:
            check([i], _budgets(chem, mech, [i], dt, True, True), "alone")
            nbatch += 1
    print("%s: budgets_kernel on %d states in %d batches: bit-identical to the compiled bud_x / bud_s_x" % (mech, len(c["names"]), nbatch))


# ---------------------------------------------------------------------------------------------------------------- pack and hand-over
def _pack_unpack(chem, mech, s1, s3, sl1, sion1, scal, c_prev, c_out, j1, j5):
    """pack_kernel on the layers, then unpack_kernel of c_out on what the pack left -> dict(C, sl1, sion1 after the pack; s1, s3, sl1_out, sion1_out).  Every
    array has a poisoned row behind the layers; a map of width 0 gets ONE poisoned entry, which must be neither read nor written."""
    import torch
    n, nv = len(c_prev), dc.table(mech)["nvar"]
    wide = lambda a, w, k: with_extra_row(a, k) if w else dc.poison((1, 1), k)
    t_s1, t_s3 = T(wide(s1, j1, 3)), T(wide(s3, j5, 4))
    t_l, t_i = T(with_extra_row(sl1, 5)), T(with_extra_row(sion1, 6))
    var, fix = T(with_extra_row(c_prev[:, :nv], 7)), T(with_extra_row(c_prev[:, nv:], 8))
    chem.pack(mech, t_s1, t_s3, t_l, t_i, T(scal), var[:n], fix[:n])
    torch.cuda.synchronize()
    out = dict(C=np.concatenate([var.cpu().numpy()[:n], fix.cpu().numpy()[:n]], axis=1), sl1=t_l.cpu().numpy()[:n].copy(), sion1=t_i.cpu().numpy()[:n].copy())
    for t, k, name in ((t_l, 5, "sl1"), (t_i, 6, "sion1"), (var, 7, "var"), (fix, 8, "fix")):
        a = t.cpu().numpy()
        assert np.array_equal(a[-1:], dc.poison((1, a.shape[1]), k)), "pack: the row of %s behind the layers was written" % name
    for t, w, k, name, src in ((t_s1, j1, 3, "s1", s1), (t_s3, j5, 4, "s3", s3)):      # inputs of the pack: untouched
        assert np.array_equal(t.cpu().numpy(), wide(src, w, k)), "pack wrote to " + name
    o1, o3 = T(wide(dc.poison((n, max(j1, 1)), 9), j1, 3)), T(wide(dc.poison((n, max(j5, 1)), 10), j5, 4))
    chem.unpack(mech, T(c_out[:, :nv]), o1, o3, t_l, t_i)
    torch.cuda.synchronize()
    for t, w, k, name in ((o1, j1, 3, "s1"), (o3, j5, 4, "s3"), (t_l, 1, 5, "sl1"), (t_i, 1, 6, "sion1")):
        a = t.cpu().numpy()
        assert np.array_equal(a[-1:], dc.poison((1, a.shape[1]), k)), "hand-over: the row of %s behind the layers (or its one entry, width 0) was written" % name
    out.update(s1=o1.cpu().numpy()[:n] if j1 else np.zeros((n, 0)), s3=o3.cpu().numpy()[:n] if j5 else np.zeros((n, 0)), sl1_out=t_l.cpu().numpy()[:n],
               sion1_out=t_i.cpu().numpy()[:n])
    return out


@pytest.mark.parametrize("mech", dc.MECHS)
def test_pack_and_handover_of_the_edge_layers(chem, mech):
    """every pack layer in one batch under the capture's maps: C (entries the tables do not name keep their poison), the clamped sl1 / sion1 where the driver
    clamps them (else untouched), and the hand-over of every layer's c_out — the last layer's has -0.0 / NaN / negative on every entry the list reads"""
    p, want, tab = dc.pack_cases(mech), dc.restated_pack(mech), dc.table(mech)
    maps = dc.map_sets(mech)["capture"]
    set_maps(chem, mech, maps)
    got = _pack_unpack(chem, mech, p["s1"], p["s3"], p["sl1"], p["sion1"], p["scal"], p["c_prev"], p["c_out"], len(maps[1]), len(maps[3]))
    if not tab["preclamp"]:
        assert dc.same(want["sl1"], p["sl1"]) and dc.same(want["sion1"], p["sion1"])      # (gas_drive leaves the model arrays alone on the way in)
    for i, name in enumerate(p["names"]):
        for key in ("C", "sl1", "sion1", "s1", "s3", "sl1_out", "sion1_out"):
            bad = np.nonzero(dc.where_differ(got[key][i], want[key][i]))[0]
            assert bad.size == 0, "%s, layer %r: %s entries %s (numbered from 1) differ from the restatement" % (mech, name, key, (bad[:8] + 1).tolist())
    kept = want["C"][0] == p["c_prev"][0]
    assert kept.sum() == tab["nvar"] + tab["nfix"] - len(maps[1]) - len(maps[3]) - len(tab["pack"]) - len(tab["fix"]) and kept.any()
    print("%s: %d edge layers packed and handed over bit-identically; %d entries of C named by no table kept their poison" % (mech, len(p["names"]), kept.sum()))


@pytest.mark.parametrize("mech", dc.MECHS)
def test_pack_and_handover_under_other_species_maps(chem, mech):
    """one ordinary layer under each legal map set of drive_cases.map_sets: s1 reversed, j1 = 1, no map at all (s1 / s3 are then one poisoned entry each,
    neither read nor written), the largest j1"""
    sets = dc.map_sets(mech)
    try:
        for name, maps in sets.items():
            lay = dc.map_layer(mech, name)
            j1, j5 = len(maps[1]), len(maps[3])
            set_maps(chem, mech, maps)
            row = lambda a: np.asarray(a)[None]
            got = _pack_unpack(chem, mech, row(lay["s1"]), row(lay["s3"]), row(lay["sl1"]), row(lay["sion1"]), row(lay["scal"]), row(lay["c_prev"]),
                               row(lay["c_out"]), j1, j5)
            for key, wkey in (("C", "C"), ("sl1", "L"), ("sion1", "I"), ("s1", "s1_out"), ("s3", "s3_out"), ("sl1_out", "L_out"), ("sion1_out", "I_out")):
                bad = np.nonzero(dc.where_differ(got[key][0], lay[wkey]))[0]
                assert bad.size == 0, "%s under the maps %r: %s entries %s (numbered from 1) differ from the restatement" % (mech, name, key, (bad[:8] + 1).tolist())
    finally:
        set_maps(chem, mech, sets["capture"])


@pytest.mark.parametrize("mech", dc.MECHS)
def test_refused_species_maps_leave_the_maps_in_force(chem, mech):
    """each refusal set raises with ITS text, and a pack afterwards gives the bits it gave before: the maps in force ("s1 reversed", so that a half-installed
    capture-like map would show) survive the refused call"""
    sets = dc.map_sets(mech)
    lay = dc.map_layer(mech, "s1 reversed")
    row = lambda a: np.asarray(a)[None]

    def pack_now():
        return _pack_unpack(chem, mech, row(lay["s1"]), row(lay["s3"]), row(lay["sl1"]), row(lay["sion1"]), row(lay["scal"]), row(lay["c_prev"]), row(lay["c_out"]), 60, 16)
    try:
        set_maps(chem, mech, sets["s1 reversed"])
        before = pack_now()
        assert dc.same(before["C"][0], lay["C"]) and not dc.same(before["C"][0], dc.map_layer(mech, "capture")["C"])
        for name, text, maps in dc.refusal_sets(mech):
            with pytest.raises(chem.MistraChemError, match=re.escape(text)):
                set_maps(chem, mech, maps)
            after = pack_now()
            for key in before:
                assert dc.same(after[key], before[key]), "%s: %s changed after the refused maps %r" % (mech, key, name)
    finally:
        set_maps(chem, mech, sets["capture"])


# ---------------------------------------------------------------------------------------------------------------- the host driver call
def _column():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "drivecol_base1.npz")))


def _host_call(chem, mech, g, idx, layer, *, bg=True, bgs=True, level=None, nrxn=None, skip=()):
    """mistra_chem_drive for the captured layers `idx` placed at the model layers `layer` (1-based), then mistra_chem_drive_device on the same rows in the same
    order: every bit of every array the call fills must be the chain's, every row, level and column outside the call must keep its poison.  skip: which of
    c_packed, ierr, stats, t_h the caller leaves out."""
    import torch
    lib = chem.lib()
    mid = dc.MECHS.index(mech)
    tab = dc.table(mech)
    nv, nf, nr, ne = tab["nvar"], tab["nfix"], chem.DIMS[mech][2], NENV[mech]
    nl = len(idx)
    layer = np.asarray(layer, np.int32)
    level = np.zeros(nl, np.int32) if level is None else np.asarray(level, np.int32)
    nrxn = nr if nrxn is None else nrxn
    idx = np.asarray(idx)
    names = json.load(open(os.path.join(REPO, "mistra_amd", "mech", mech + ".rates_env.json")))["env"]
    env = g["env"][idx, :ne].copy()
    env[:, [j for j, nm in enumerate(names) if nm.startswith(("c(", "fix("))]] = np.nan      # the device refills them from its own packed C
    scal = np.ascontiguousarray(g["scal"][idx])
    # ---- the model's arrays: N rows and one behind them, every entry poisoned, the call's layers from the capture
    widths = dict(s1=g["s1_in"].shape[1], s3=g["s3_in"].shape[1], sl1=g["sl1_in"].shape[1], sion1=g["sion1_in"].shape[1], bgs=2 * dc.NBGS)
    a = {key: dc.poison((N + 1, w), k) for k, (key, w) in enumerate(widths.items())}
    a["bg"] = dc.poison((NLEV + 1, 2 * nrxn), 11)
    for key in widths:
        a[key][layer - 1] = g[key + "_in"][idx]
    rng = np.random.default_rng([dc.SEED, 200 + mid])
    for lv in set(level.tolist()) - {0}:      # (cumulative budgets of the level as the model would hold them)
        a["bg"][lv - 1].reshape(nrxn, 2)[:nr] = dc.seeded(rng, (nr, 2))
    before = {key: v.copy() for key, v in a.items()}
    out = dict(ierr=np.full(nl + 1, -77, np.int32), stats=np.full((nl + 1, 8), -77, np.int32), t_h=dc.poison((nl + 1, 3), 12), c_packed=dc.poison((nl + 1, nv + nf), 13))
    P = lambda x, t=C.c_double: None if x is None else x.ctypes.data_as(C.POINTER(t))
    O = lambda key, t=C.c_double: None if key in skip else P(out[key], t)
    rc = lib.mistra_chem_drive(mid, nl, P(layer, C.c_int32), N, P(a["s1"]), P(a["s3"]), P(a["sl1"]), P(a["sion1"]), P(scal), P(env), 0.0, 10.0, O("ierr", C.c_int32),
                               O("stats", C.c_int32), O("t_h"), P(a["bg"]) if bg else None, nrxn, P(level, C.c_int32) if bg else None, P(a["bgs"]) if bgs else None,
                               O("c_packed"))
    assert rc == 0, lib.mistra_chem_last_error().decode()
    # ---- the same rows through the device-resident chain
    d = {key: T(before[key][layer - 1]) for key in ("s1", "s3", "sl1", "sion1", "bgs")}
    bgd = np.zeros((nl, nr, 2))
    for j in range(nl):
        if level[j] > 0:
            bgd[j] = before["bg"][level[j] - 1].reshape(nrxn, 2)[:nr]
    bgt = T(bgd)
    dev = _dev()
    var, fix = torch.zeros((nl, nv), dtype=torch.float64, device=dev), torch.zeros((nl, nf), dtype=torch.float64, device=dev)
    di, ds = torch.empty(nl, dtype=torch.int32, device=dev), torch.empty((nl, 8), dtype=torch.int32, device=dev)
    th = torch.empty((nl, 2), dtype=torch.float64, device=dev)
    chem.drive(mech, d["s1"], d["s3"], d["sl1"], d["sion1"], T(scal), T(env), var, fix, 0.0, 10.0, di, ds, th, bgt if bg else None, d["bgs"] if bgs else None)
    torch.cuda.synchronize()
    assert np.all(di.cpu().numpy() == 1)
    what = "%s, layers %s" % (mech, layer.tolist())
    inside = np.zeros(N + 1, bool)
    inside[layer - 1] = True
    for key in ("s1", "s3", "sl1", "sion1", "bgs"):
        if key == "bgs" and not bgs:
            assert np.array_equal(a[key], before[key]), what + ": bgs written though the call had none"
            continue
        assert dc.same(a[key][layer - 1], d[key].cpu().numpy().reshape(nl, -1)), "%s: %s differs from the device-resident chain" % (what, key)
        assert np.array_equal(a[key][~inside], before[key][~inside]), "%s: %s: a row of a layer outside the call was written" % (what, key)
    written = np.zeros(NLEV + 1, bool)
    if bg:
        for j in range(nl):
            if level[j] > 0:
                written[level[j] - 1] = True
                row = a["bg"][level[j] - 1].reshape(nrxn, 2)
                assert dc.same(row[:nr], bgt.cpu().numpy()[j]), "%s: bg of level %d differs from the device-resident chain" % (what, level[j])
                assert np.array_equal(row[nr:], before["bg"][level[j] - 1].reshape(nrxn, 2)[nr:]), what + ": bg: slots past the mechanism's NREACT were written"
    assert np.array_equal(a["bg"][~written], before["bg"][~written]), what + ": a level of bg outside the call was written"
    got = dict(ierr=out["ierr"][:nl], stats=out["stats"][:nl], t_h=out["t_h"][:nl, :2], c_packed=out["c_packed"][:nl])
    want_c = np.stack([pack_py.pack(tab, np.zeros(nv + nf), before["s1"][k - 1], before["s3"][k - 1], before["sl1"][k - 1], before["sion1"][k - 1], scal[j, 0], scal[j, 1],
                                    scal[j, 2:6], g[mech + "_gas_m2k"], g[mech + "_rad_m2k"])[0] for j, k in enumerate(layer)])
    want = dict(ierr=di.cpu().numpy(), stats=ds.cpu().numpy(), t_h=th.cpu().numpy(), c_packed=want_c)
    fresh = dict(ierr=np.full(nl + 1, -77, np.int32), stats=np.full((nl + 1, 8), -77, np.int32), t_h=dc.poison((nl + 1, 3), 12), c_packed=dc.poison((nl + 1, nv + nf), 13))
    for key in got:
        if key in skip:
            assert np.array_equal(out[key], fresh[key])
            continue
        assert dc.same(got[key], want[key]) if got[key].dtype == np.float64 else np.array_equal(got[key], want[key]), "%s: %s" % (what, key)
        assert np.array_equal(out[key][nl:], fresh[key][nl:]), "%s: the row of %s behind the call was written" % (what, key)
    return a


@pytest.mark.parametrize("mech", ["gas", "aer"])
def test_host_driver_call_in_the_layouts_the_captures_never_use(chem, mech):
    """mistra_chem_drive_begin / _end: drive_layout places bg, bgs and c_packed at offsets that depend on which are absent; the gather and the scatter follow
    the layer list and the budget levels.  Layers of one captured column step (tests/golden/drivecol_base1.npz), at most 8 per call; the integrator is not
    under test: everything is compared with mistra_chem_drive_device on the same rows, bit for bit.  Step reuse stays off (tests/test_gpu_step_reuse.py)."""
    g = _column()
    mid = dc.MECHS.index(mech)
    assert not chem.get_step_reuse(mech)
    own = np.nonzero(g["mech"] == mid)[0]
    lev = own[g["level"][own] > 0]
    plain = own[g["level"][own] == 0]
    A = np.concatenate([lev[:3], plain[:5]])           # three layers with a budget level, five without
    B = np.concatenate([plain[5:10], lev[3:6]])
    assert len(A) == len(B) == 8 and not set(A) & set(B)
    levA, levB = g["level"][A], g["level"][B]
    set_maps(chem, mech, tuple(g["%s_%s" % (mech, key)] for key in ("gas_m2k", "gas_k2m", "rad_m2k", "rad_k2m")))
    nr = chem.DIMS[mech][2]
    gaps = [N, 141, 77, 30, 29, 5, 3, 1]               # descending, with gaps, the arrays' last row first
    call = lambda idx, layer, **kw: _host_call(chem, mech, g, idx, layer, **kw)
    call(A[:1], [g["k"][A[0]]], level=levA[:1])                                    # nlayer = 1
    call(A, g["k"][A], level=levA)                                                 # model order, everything present
    call(A, gaps, level=levA)                                                      # reversed, with gaps, layer = n
    call(A, gaps, bg=False)                                                        # bg absent, bgs present
    call(A, gaps, bgs=False, level=levA)                                           # bgs absent, bg present
    call(A, gaps, bg=False, bgs=False)
    call(A, gaps, level=np.zeros(8, np.int32))                                     # every bg_level zero: no row of bg written
    call(A, gaps, level=levA, nrxn=nr + 3)                                         # nrxn larger than NREACT
    for key in ("c_packed", "ierr", "stats", "t_h"):
        call(A, gaps, level=levA, skip=(key,))
    call(A, gaps, level=levA, skip=("c_packed", "ierr", "stats", "t_h"))
    # a call of 8 layers, then 1, then 8 with other inputs at other layers: the arena's old content must not show anywhere
    call(A, g["k"][A], level=levA)
    call(B[3:4], [N])
    call(B, gaps[::-1], level=levB, bgs=False)
    call(B, gaps[::-1], level=levB)
