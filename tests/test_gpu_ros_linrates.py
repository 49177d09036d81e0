"""A series of Rosenbrock_x calls with rate constants linear in time over each leg on the GPU (-m gpu): mistra_chem_rosenbrock_series_linrates_ex /
_device and their cells forms (kernel VARIANT 10) against the restatement that defines them (tests/ros_linrates_py.py;
bounds: tests/ros_linrates_bounds.py, measured on the restatement's side by tests/test_ros_linrates.py), against the series with rates where the
two must agree, and not against it where they must not.  Three cells and four legs per launch unless a test says otherwise."""
import os
import subprocess

import numpy as np
import pytest

import ros_linrates_bounds as lb
import ros_linrates_py as LR
from conftest import MECHS, REPO, rel_diff

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    yield c
    if c.device_count() != 1:      # whatever a test initialised: the other modules' fixtures start from init(0)
        c.finalize()
        c.init(0)
    for mech in MECHS:             # and from INTEGRATE_x's values
        c.clear_options(mech)


_rows = {}


def _nodes(mech):
    """(VAR [3, NVAR], leg FIX [4, 3, NFIX], node RCONST [5, 3, NREACT]): read once, shared, never written"""
    if mech not in _rows:
        _rows[mech] = LR.nodes(mech)
        for x in _rows[mech]:
            x.setflags(write=False)
    return _rows[mech]


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _np(res):
    return type(res)(*(x.cpu().numpy() for x in res))


def _lin(chem, mech, V, F, NK, s, atol=None, rtol=None, host=False):
    """the entry under test: device (-> t_h [nleg, ncell, 2]) or host (-> [nleg, ncell, 3]); F: [ncell, NFIX] shared or [nleg, ncell, NFIX]"""
    import torch
    at, rt = (s.atol, s.rtol) if atol is None else (atol, rtol)
    if host:
        return chem.rosenbrock_series_linrates(mech, V, F, NK, s.times, s.ipar, s.rpar, at, rt, carry_h=s.carry)
    if atol is not None:
        at, rt = _T(at), _T(rt)
    res = chem.rosenbrock_series_linrates(mech, _T(V), _T(F), _T(NK), s.times, s.ipar, s.rpar, at, rt, carry_h=s.carry)
    torch.cuda.synchronize()
    return _np(res)


def _rates(chem, mech, V, F, K, s):
    import torch
    res = chem.rosenbrock_series_rates(mech, _T(V), _T(F), _T(K), s.times, s.ipar, s.rpar, s.atol, s.rtol, carry_h=s.carry)
    torch.cuda.synchronize()
    return _np(res)


def _check(mech, name, times, got, want):
    """IERR and all eight counters equal in every leg; VAR within LINRATES_RTOL, Texit / Hexit within LINRATES_TH_RTOL; every figure printed first"""
    var, ierr, st, te, he = want
    d_var, d_th = lb.leg_diffs(times, got.var, got.t_h[..., 0], got.t_h[..., 1], var, te, he)
    print("%s %s: VAR %.3e (bound %.1e), exit time / step size %.3e (bound %.1e), Nstp %s" %
          (mech, name, d_var, lb.LINRATES_RTOL[mech], d_th, lb.LINRATES_TH_RTOL[mech], got.stats[..., 2].tolist()))
    assert np.array_equal(got.ierr, ierr), (name, got.ierr.tolist(), ierr.tolist())
    assert np.array_equal(got.stats, st), (name, got.stats.tolist(), st.tolist())
    assert d_var <= lb.LINRATES_RTOL[mech], (name, d_var)
    assert d_th <= lb.LINRATES_TH_RTOL[mech], (name, d_th)


# ---- 1. parity with the restatement
@pytest.mark.parametrize("mech", MECHS)
def test_l1_every_set_is_the_restatement(chem, mech):
    """every set of ros_linrates_py.set_names(mech) through the device entry: all five methods, the carried first step, FIX of the leg's own, equal
    nodes, the descending series (IERR -7 in every leg, the next leg going on) and, on gas, IPAR(1) = 1.  The host entry once per mechanism (m2), equal
    to the device entry in every array."""
    want = LR.restated(mech)
    rows = _nodes(mech)
    for name in LR.set_names(mech):
        s, V, F, NK = LR.set_rows(mech, name, rows)
        got = _lin(chem, mech, V, F, NK, s)
        _check(mech, name, s.times, got, want[name])
        assert (got.ierr == LR.FAILING_IERR.get(name, 1)).all(), name
        if name == "m2":
            h = _lin(chem, mech, V, F, NK, s, host=True)
            assert np.array_equal(h.var, got.var) and np.array_equal(h.ierr, got.ierr) and np.array_equal(h.stats, got.stats)
            assert np.array_equal(h.t_h[..., :2], got.t_h)


# ---- 2. equal nodes are the series with rates on the shared block
@pytest.mark.parametrize("method", (2, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_l2_equal_nodes_are_the_series_with_rates(chem, mech, method):
    """all node blocks the night rows: np.array_equal with rosenbrock_series_rates on that block in every output (a zero's sign is not compared: dFdT is
    a sum of zero products here and the literal +0.0 there), ascending and descending, Ros3 and Rodas4"""
    rows = _nodes(mech)
    s, V, F, NK = LR.set_rows(mech, "ros3_equal_nodes" if method == 2 else "rodas4_equal_nodes", rows)
    for times in (s.times, s.times[::-1].copy()):
        ser = s._replace(times=times)
        got, want = _lin(chem, mech, V, F, NK, ser), _rates(chem, mech, V, F, NK[0], ser)
        for a, b, what in zip(got, want, ("var", "ierr", "stats", "t_h")):
            assert np.array_equal(a, b), (what, times.tolist())
        if times[1] > times[0]:
            assert (got.ierr == 1).all(), got.ierr.tolist()
        assert (got.stats[..., 2] >= 1).all()


# ---- 3. linear is not the staircase
@pytest.mark.parametrize("mech", MECHS)
def test_l3_linear_is_not_the_staircase(chem, mech):
    """m2 against rosenbrock_series_rates with node blocks 0 .. nleg-1 as the legs' rate constants: the end states differ by more than 100x
    LINRATES_RTOL"""
    rows = _nodes(mech)
    s, V, F, NK = LR.set_rows(mech, "m2", rows)
    got, stair = _lin(chem, mech, V, F, NK, s), _rates(chem, mech, V, F, NK[:4], s)
    d = float(rel_diff(got.var[-1], stair.var[-1]).max())
    print("%s: linear against the staircase, end state rel_diff %.3e (100x LINRATES_RTOL = %.1e)" % (mech, d, 100.0 * lb.LINRATES_RTOL[mech]))
    assert (got.ierr == 1).all() and (stair.ierr == 1).all()
    assert d > 100.0 * lb.LINRATES_RTOL[mech]


# ---- 4. every cell reads its own nodes
@pytest.mark.parametrize("ncell", (1, 7))
def test_l4_every_cell_reads_its_own_nodes(chem, ncell):
    """gas, ncell copies of one cell, cell c's node blocks scaled by 1 + c/1024 (exact): each cell against its own restatement, through the shared pair
    and through the cells forms with per-cell tolerances [ncell, 1] (device and host)"""
    V3, LF, NK3 = _nodes("gas")
    s = LR.series_set("gas", "m2")[0]
    V = np.repeat(V3[:1], ncell, axis=0)
    F = np.repeat(LF[0, :1], ncell, axis=0)
    NK = np.stack([NK3[:, 0] * (1.0 + c / 1024.0) for c in range(ncell)], axis=1)
    assert NK.shape == (5, ncell, NK3.shape[-1])
    want = LR.chain_cells("gas", s, V, F, NK)
    got = _lin(chem, "gas", V, F, NK, s)
    _check("gas", "m2 x %d" % ncell, s.times, got, want)
    if ncell > 1:      # the cells differ: the scaling is read
        assert all(got.var[-1, c].tobytes() != got.var[-1, 0].tobytes() for c in range(1, ncell))
    # per-cell tolerances: cell c with RelTol 1e-3 / (1 + c), AbsTol 1e-25
    at, rt = np.full((ncell, 1), 1.0e-25), (1.0e-3 / (1.0 + np.arange(ncell))).reshape(ncell, 1)
    ipar = s.ipar.copy()
    ipar[1] = 1
    want_c = [LR.chain_cells("gas", s._replace(ipar=ipar, atol=np.full(V.shape[1], at[c, 0]), rtol=np.full(V.shape[1], rt[c, 0])), V[c:c + 1], F[c:c + 1], NK[:, c:c + 1])
              for c in range(ncell)]
    want_c = tuple(np.concatenate([w[i] for w in want_c], axis=1) for i in range(5))
    sc = s._replace(ipar=ipar)
    got_c = _lin(chem, "gas", V, F, NK, sc, atol=at, rtol=rt)
    _check("gas", "m2 x %d, cells form" % ncell, s.times, got_c, want_c)
    h = _lin(chem, "gas", V, F, NK, sc, atol=at, rtol=rt, host=True)
    assert np.array_equal(h.var, got_c.var) and np.array_equal(h.ierr, got_c.ierr) and np.array_equal(h.stats, got_c.stats) and np.array_equal(h.t_h[..., :2], got_c.t_h)


def test_l4_two_device_slots_ragged_split(chem):
    """init_devices([0, 0]), five gas cells over two slots (3 + 2), the host entry with two legs: every slot takes its own cells of the three node
    blocks and of the two blocks of FIX — a strided upload of nleg + 1 and of nleg blocks — and of every leg's results.  Bit for bit one slot's."""
    V3, LF, NK3 = _nodes("gas")
    s = LR.series_set("gas", "m2")[0]
    s = s._replace(times=np.ascontiguousarray(s.times[:3]))
    idx = np.array([0, 1, 2, 1, 0])
    V = V3[idx] * (1.0 + np.arange(5) / 1024.0).reshape(5, 1)                             # five different cells
    F = np.ascontiguousarray(LF[:2, idx])                                                 # FIX per leg: [2, 5, NFIX]
    NK = np.ascontiguousarray(NK3[:3, idx] * (1.0 + np.arange(5) / 2048.0).reshape(1, 5, 1))      # the nodes: [3, 5, NREACT]
    one = _lin(chem, "gas", V, F, NK, s, host=True)
    assert one.var.shape[:2] == (2, 5) and (one.ierr == 1).all()
    assert len({one.var[-1, c].tobytes() for c in range(5)}) == 5      # (a cell handed to the wrong slot, or its rows from the wrong block, would show)
    try:
        chem.finalize()
        chem.init_devices([0, 0])
        assert chem.device_count() == 2
        two = _lin(chem, "gas", V, F, NK, s, host=True)
    finally:
        chem.finalize()
        chem.init(0)
    for a, b, what in zip(two, one, ("var", "ierr", "stats", "t_h")):
        assert a.tobytes() == b.tobytes(), what


# ---- 5. user slots
def test_l5_user_slots_fail_with_the_slots_text(chem):
    names = chem.user_mechs()
    assert len(names) == 2
    for i, slot in enumerate(names):
        nvar, nfix, nreact, _ = chem.DIMS[slot]
        V, F, NK = np.full((1, nvar), 1.0e-10), np.ones((1, nfix)), np.ones((2, 1, nreact))
        for args in ((V, F, NK), (_T(V), _T(F), _T(NK))):
            with pytest.raises(chem.MistraChemError, match="user mechanism slot %d \\(%s\\) has no series of Rosenbrock_x calls" % (i, slot)):
                chem.rosenbrock_series_linrates(slot, *args, [0.0, 1.0])


# ---- 6. from Fortran
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_l6_from_fortran(chem, tmp_path):
    """shim/shim_driver MG: ROSENBROCK_BATCH_SERIES_LINRATES_g on the descending set, RNODES(NREACT, NCELL, NLEG + 1) with FIX(NFIX, NCELL, 1) and with
    FIX(NFIX, NCELL, NLEG) — the C host entry's bytes, and ros_ErrorMsg_g's lines on unit 6 for every failed leg and cell"""
    mech = "gas"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    rows = _nodes(mech)
    s, V, F1, NK = LR.set_rows(mech, "ros3_descending", rows)
    n, nvar = V.shape
    nleg = len(s.times) - 1
    for F in (F1, np.ascontiguousarray(rows[1][::-1])):
        nlf = 1 if F.ndim == 2 else nleg
        want = _lin(chem, mech, V, F, NK, s, host=True)
        assert (want.ierr == -7).all()
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(fin, "wb") as f:
            np.concatenate([s.ipar.astype(np.float64), s.rpar, s.atol, s.rtol, [float(n), float(nleg), float(s.carry), 0.0, float(nleg + 1), float(nlf)],
                            s.times]).tofile(f)
            V.tofile(f)
            np.ascontiguousarray(F).tofile(f)       # [fix_legs][ncell][NFIX]
            np.ascontiguousarray(NK).tofile(f)      # [nleg + 1][ncell][NREACT]
        r = subprocess.run([DRIVER, "MG", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
        out = np.fromfile(fout, np.float64).reshape(nleg, n, nvar + 2 + 9)      # per leg and cell: VAR, Texit, Hexit, IERR, ISTAT(8)
        assert out[..., :nvar].tobytes() == want.var.tobytes(), nlf
        assert out[..., nvar:nvar + 2].tobytes() == want.t_h[..., :2].tobytes(), nlf
        assert np.array_equal(out[..., nvar + 2].astype(np.int32), want.ierr) and np.array_equal(out[..., nvar + 3:].astype(np.int32), want.stats)
        assert r.stdout.count("Forced exit from Rosenbrock_g") == nleg * n, r.stdout
