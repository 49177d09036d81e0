"""A series of Rosenbrock_x calls on the GPU (-m gpu): mistra_chem_rosenbrock_series_ex / _device and their cells forms run nleg calls of Rosenbrock_x
over times[0 .. nleg] in one launch, the state on chip from leg to leg.  A series is bit for bit the sequence of calls of the existing entries it
replaces — those are unchanged by the series and themselves pinned to the compiled reference by tests/test_gpu_ros_methods.py — and is compared with
the compiled Rosenbrock_x called leg by leg directly (tests/golden/ros_series_<mech>.npz; bounds: tests/ros_series_bounds.py, measured on the reference
side by tests/test_ros_series.py).  1, 3 and 65 cells per launch: cells 0, n/2, n-1 of integrate_<mech>.npz unless a test says otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ros_options_py as R
import ros_series_bounds as sb
import ros_series_py as RS
from conftest import MECHS, REPO, load_golden

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}


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


def _cells(mech):
    g = load_golden(mech)
    c = list(RS.cells_of(g["var_in"].shape[0]))
    return g["var_in"][c], g["fix"][c], g["rconst"][c]


def _fixture(mech):
    return dict(np.load(os.path.join(REPO, "tests", "golden", "ros_series_%s.npz" % mech)))


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _np(res):
    """a SeriesResult of tensors -> of numpy arrays (after a synchronisation)"""
    return type(res)(*(x.cpu().numpy() for x in res))


def _series(chem, mech, V, F, K, s, hstart=None, atol=None, rtol=None, host=False):
    """the series entry: device (-> t_h [nleg, ncell, 2]) or host (-> [nleg, ncell, 3]); atol / rtol: per-cell rows instead of the set's pair"""
    import torch
    at, rt = (s.atol, s.rtol) if atol is None else (atol, rtol)
    if host:
        return chem.rosenbrock_series(mech, V, F, K, s.times, s.ipar, s.rpar, at, rt, hstart=hstart, carry_h=s.carry)
    if atol is not None:
        at, rt = _T(at), _T(rt)
    res = chem.rosenbrock_series(mech, _T(V), _T(F), _T(K), s.times, s.ipar, s.rpar, at, rt, hstart=None if hstart is None else _T(hstart), carry_h=s.carry)
    torch.cuda.synchronize()
    return _np(res)


def _sequence(chem, mech, V, F, K, s, hstart=None, atol=None, rtol=None):
    """what a series replaces: nleg calls of the existing device entry, queued on one stream, each on the state the one before left.  carry: the
    previous call's Hexit column as d_hstart; else d_hstart = None behind leg 0."""
    import torch
    dV, dF, dK = _T(V), _T(F), _T(K)
    hs = None if hstart is None else _T(hstart)
    if atol is not None:
        d_at, d_rt = _T(atol), _T(rtol)
    legs = []
    for k in range(len(s.times) - 1):
        t0, t1 = float(s.times[k]), float(s.times[k + 1])
        if atol is None:
            res, th = chem.rosenbrock(mech, dV, dF, dK, t0, t1, s.ipar, s.rpar, s.atol, s.rtol, hstart=hs)
        else:
            res, th = chem.rosenbrock_cells(mech, dV, dF, dK, t0, t1, s.ipar, s.rpar, d_at, d_rt, hstart=hs)
        legs.append((res, th))
        dV = res.var
        hs = th[:, 1].contiguous() if s.carry else None
    torch.cuda.synchronize()
    return chem.SeriesResult(np.stack([r.var.cpu().numpy() for r, _ in legs]), np.stack([r.ierr.cpu().numpy() for r, _ in legs]),
                             np.stack([r.stats.cpu().numpy() for r, _ in legs]), np.stack([th.cpu().numpy() for _, th in legs]))


def _same(a, b, what=""):
    assert np.array_equal(a.ierr, b.ierr), (what, a.ierr.tolist(), b.ierr.tolist())
    assert np.array_equal(a.stats, b.stats), (what, a.stats.tolist(), b.stats.tolist())
    assert a.var.shape == b.var.shape and a.var.tobytes() == b.var.tobytes(), what
    assert a.t_h.shape == b.t_h.shape and a.t_h.tobytes() == b.t_h.tobytes(), (what, a.t_h.tolist(), b.t_h.tolist())


# ---- 1. one leg is the call
@pytest.mark.parametrize("method", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_s1_one_leg_is_the_call(chem, mech, method):
    """nleg = 1 gives rosenbrock / rosenbrock_cells bit for bit (var, ierr, stats, t_h), host and device entries, all five methods"""
    import torch
    V, F, K = _cells(mech)
    s = RS.method_series(mech, method)._replace(times=np.array([0.0, 10.0]))
    res, th = chem.rosenbrock(mech, V, F, K, 0.0, 10.0, s.ipar, s.rpar, s.atol, s.rtol)
    assert (res.ierr == 1).all()
    got = _series(chem, mech, V, F, K, s, host=True)
    _same(got, chem.SeriesResult(res.var[None], res.ierr[None], res.stats[None], th[None]), "host")
    d_res, d_th = chem.rosenbrock(mech, _T(V), _T(F), _T(K), 0.0, 10.0, s.ipar, s.rpar, s.atol, s.rtol)
    torch.cuda.synchronize()
    want = chem.SeriesResult(d_res.var.cpu().numpy()[None], d_res.ierr.cpu().numpy()[None], d_res.stats.cpu().numpy()[None], d_th.cpu().numpy()[None])
    _same(_series(chem, mech, V, F, K, s), want, "device")
    assert want.var.tobytes() == res.var[None].tobytes()
    # the cells forms, one scalar row per cell
    at = np.array([[1.0e-25], [1.0e-20], [1.0e-18]])
    rt = np.array([[1.0e-3], [1.0e-4], [1.0e-2]])
    c_res, c_th = chem.rosenbrock_cells(mech, V, F, K, 0.0, 10.0, s.ipar, s.rpar, at, rt)
    _same(_series(chem, mech, V, F, K, s, atol=at, rtol=rt, host=True), chem.SeriesResult(c_res.var[None], c_res.ierr[None], c_res.stats[None], c_th[None]), "cells host")
    _same(_series(chem, mech, V, F, K, s, atol=at, rtol=rt), chem.SeriesResult(c_res.var[None], c_res.ierr[None], c_res.stats[None], c_th[None, :, :2]),
          "cells device")


# ---- 2. a series is the sequence; 3. against the compiled reference directly
@pytest.mark.parametrize("name", RS.SET_NAMES)
@pytest.mark.parametrize("mech", MECHS)
def test_s2_a_series_is_the_sequence_and_the_compiled_chain(chem, mech, name):
    """Per set: every per-leg output bit-identical to nleg queued calls of the existing device entry (carry_h: the previous call's Hexit column as
    d_hstart), the host entry gives the device entry's bits, and against the compiled Rosenbrock_x called leg by leg: IERR and the counters identical in
    every leg, VAR, exit time and last step size within ros_series_bounds."""
    V, F, K = _cells(mech)
    s = RS.series_set(mech, name)
    got = _series(chem, mech, V, F, K, s)
    _same(got, _sequence(chem, mech, V, F, K, s), name)
    host = _series(chem, mech, V, F, K, s, host=True)
    _same(type(host)(host.var, host.ierr, host.stats, host.t_h[..., :2].copy()), got, name + " host")
    z = _fixture(mech)
    d_var, d_th = sb.leg_diffs(s.times, got.var, got.t_h[..., 0], got.t_h[..., 1], z[name + "_var"], z[name + "_rpar"][..., 0], z[name + "_rpar"][..., 1])
    print("%s %s: VAR %.3e (bound %.1e), exit time / last step size %.3e (bound %.1e), Nstp %s, IERR %s" %
          (mech, name, d_var, sb.SERIES_RTOL[mech], d_th, sb.SERIES_TH_RTOL[mech], got.stats[..., 2].tolist(), got.ierr.tolist()))
    assert np.array_equal(got.ierr, z[name + "_ierr"]), (got.ierr.tolist(), z[name + "_ierr"].tolist())
    assert np.array_equal(got.stats, z[name + "_ipar"]), (got.stats.tolist(), z[name + "_ipar"].tolist())
    assert d_var <= sb.SERIES_RTOL[mech]
    assert d_th <= sb.SERIES_TH_RTOL[mech]
    if name in RS.FAILING_SETS:      # a failed leg does not end the series: the next starts at its own time from the state left
        assert (got.ierr == -6).all() and got.var[0].tobytes() != got.var[1].tobytes() != got.var[2].tobytes()


@pytest.mark.parametrize("method", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_s2_the_five_methods_on_one_grid(chem, mech, method):
    """each method over METHOD_GRID, without and with the carried first step, and with a per-cell first step on leg 0 mixed with zeros"""
    V, F, K = _cells(mech)
    s = RS.method_series(mech, method)
    plain = _series(chem, mech, V, F, K, s)
    _same(plain, _sequence(chem, mech, V, F, K, s), "carry_h = 0")
    assert (plain.ierr == 1).all()
    c = s._replace(carry=True)
    carried = _series(chem, mech, V, F, K, c)
    _same(carried, _sequence(chem, mech, V, F, K, c), "carry_h = 1")
    assert carried.var[0].tobytes() == plain.var[0].tobytes() and not np.array_equal(carried.stats[1:], plain.stats[1:])
    hs = np.array([0.0, 0.5, -1.0])
    for ser in (s, c):
        got = _series(chem, mech, V, F, K, ser, hstart=hs)
        _same(got, _sequence(chem, mech, V, F, K, ser, hstart=hs), "d_hstart, carry %s" % ser.carry)
        for cell in (0, 2):      # entries <= 0: the options' first step
            assert got.var[:, cell].tobytes() == (carried if ser.carry else plain).var[:, cell].tobytes()
        assert not np.array_equal(got.stats[0, 1], plain.stats[0, 1]) or got.t_h[0, 1].tobytes() != plain.t_h[0, 1].tobytes()


# ---- 4. failing legs and cells
@pytest.mark.parametrize("mech", MECHS)
def test_s4_a_nan_cell_between_two_good_ones(chem, mech):
    """-7 in every leg of the NaN cell; the good cells' bits equal the run without it.  The NaN cell against the sequence: counters, codes and times
    identical, the state equal with NaN = NaN — a cell whose step size has shrunk to zero accepts that step (H <= Hmin = 0, gas.f:1302) before the next
    check ends the call with -7, so its state is Ynew, NaNs formed by arithmetic, and the sign bit of such a NaN follows the operand order the compiler
    chose in each kernel."""
    V, F, K = _cells(mech)
    s = RS.series_set(mech, "ros3_unequal")
    good = _series(chem, mech, V[[0, 2]], F[[0, 2]], K[[0, 2]], s)
    Vn = V.copy()
    Vn[1, 5] = np.nan
    got = _series(chem, mech, Vn, F, K, s)
    seq = _sequence(chem, mech, Vn, F, K, s)
    assert np.array_equal(got.var, seq.var, equal_nan=True) and got.var[:, [0, 2]].tobytes() == seq.var[:, [0, 2]].tobytes()
    _same(got._replace(var=seq.var), seq)
    assert np.isnan(got.var[:, 1]).any(axis=1).all()
    assert (got.ierr[:, 1] == -7).all() and (got.ierr[:, [0, 2]] == 1).all()
    assert got.var[:, [0, 2]].tobytes() == good.var.tobytes() and np.array_equal(got.stats[:, [0, 2]], good.stats)
    assert got.t_h[:, [0, 2]].tobytes() == good.t_h.tobytes()


@pytest.mark.parametrize("mech", MECHS)
def test_s4_zero_pivots_start_afresh_in_every_leg(chem, mech):
    """the crafted zero-pivot cell of tests/test_gpu_phases.py (a first-order loss with k = -1/(H*gamma) at the first step size) over two legs: one
    zero pivot in each leg (Nsng = 1 twice, not 1 then 2) — and six in a row in each: -8 twice, Nsng = 6 twice, the run of singular decompositions
    starting afresh"""
    from mistra_amd.mechtab import load
    from test_gpu_phases import GAMMA, _first_order_losses
    g, t = load_golden(mech), load(mech)
    losses, seen = [], set()
    for r, sp in _first_order_losses(t):
        if sp not in seen:
            seen.add(sp)
            losses.append((r, sp))
    V, F = g["var_in"][:1].copy(), g["fix"][:1].copy()
    ipar, rpar, atol, rtol = R.base_options(mech)
    s = RS.Series(ipar, rpar, atol, rtol, np.array([0.0, 1.5e-3, 3.0e-3]), False)
    for nzero, want_ierr in ((1, 1), (6, -8)):
        K = np.zeros((1, t.nreact))
        for i in range(nzero):
            K[0, losses[i][0]] = -1.0 / ((1.0e-3 / 2 ** i) * GAMMA[0])
        got = _series(chem, mech, V, F, K, s)
        _same(got, _sequence(chem, mech, V, F, K, s), nzero)
        assert got.ierr[:, 0].tolist() == [want_ierr, want_ierr] and got.stats[:, 0, 7].tolist() == [nzero, nzero], (got.ierr.tolist(), got.stats.tolist())


@pytest.mark.parametrize("mech", MECHS)
def test_s4_a_refused_row_in_the_cells_form(chem, mech):
    """per-cell -5: every leg of that cell is var_in, -5, zeros; the neighbours are untouched by it (their bits equal the run without the row)"""
    V, F, K = _cells(mech)
    s = RS.series_set(mech, "ros3_unequal_carry")
    at, rt = np.full((3, 1), 1.0e-25), np.full((3, 1), 1.0e-3)
    good = _series(chem, mech, V, F, K, s, atol=at, rtol=rt)
    _same(good, _series(chem, mech, V, F, K, s), "rows of the shared pair")
    rt[1, 0] = 1.0      # RelTol >= 1: refused
    for host in (False, True):
        got = _series(chem, mech, V, F, K, s, atol=at, rtol=rt, host=host)
        assert (got.ierr[:, 1] == -5).all() and not got.stats[:, 1].any() and not got.t_h[:, 1].any()
        for k in range(len(s.times) - 1):
            assert got.var[k, 1].tobytes() == V[1].tobytes()
        assert got.var[:, [0, 2]].tobytes() == good.var[:, [0, 2]].tobytes() and np.array_equal(got.stats[:, [0, 2]], good.stats[:, [0, 2]])
        assert got.t_h[:, [0, 2], :2].tobytes() == good.t_h[:, [0, 2]].tobytes()
    _same(_series(chem, mech, V, F, K, s, atol=at, rtol=rt), _sequence(chem, mech, V, F, K, s, atol=at, rtol=rt))


def test_s4_host_refusals_fill_every_leg_and_launch_nothing(chem):
    """-1 .. -4 and -5 on a shared pair through both entries: the call returns 0, every leg of every cell is var_in, the code, zeros; the block behind
    the legs and the row behind the cells stay as they were"""
    import torch
    mech = "gas"
    V, F, K = _cells(mech)
    n, nvar = V.shape
    L = chem.lib()
    times, nleg = np.array([0.0, 1.0, 5.0]), 2
    for name in R.REFUSED_NAMES:
        ipar, rpar, atol, rtol = R.refused_set(mech, name)
        code = R.REFUSED_IERR[name]
        opts = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip))
        out, ierr, stats, th = np.full((nleg + 1, n, nvar), -7.25), np.full((nleg + 1, n), 77, np.int32), np.full((nleg + 1, n, 8), 77, np.int32), np.full((nleg + 1, n, 3), -7.25)
        rc = L.mistra_chem_rosenbrock_series_ex(0, n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), nleg, times.ctypes.data_as(_dp), *opts,
                                                0, None, out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp))
        assert rc == 0, (name, L.mistra_chem_last_error())
        for k in range(nleg):
            assert (ierr[k] == code).all() and out[k].tobytes() == V.tobytes() and not stats[k].any() and not th[k].any(), name
        assert (out[nleg] == -7.25).all() and (ierr[nleg] == 77).all() and (stats[nleg] == 77).all() and (th[nleg] == -7.25).all(), name
        dV, dF, dK = _T(V), _T(F), _T(K)
        d_out, d_ierr, d_stats, d_th = _T(np.full((nleg + 1, n, nvar), -7.25)), _T(np.full((nleg + 1, n), 77, np.int32)), _T(np.full((nleg + 1, n, 8), 77, np.int32)), _T(np.full((nleg + 1, n, 2), -7.25))
        rc = L.mistra_chem_rosenbrock_series_device(0, n, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), nleg, times.ctypes.data_as(_dp), *opts, d_out.data_ptr(),
                                                    d_ierr.data_ptr(), d_stats.data_ptr(), d_th.data_ptr(), 1, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (name, L.mistra_chem_last_error())
        torch.cuda.synchronize()
        out, ierr, stats, th = d_out.cpu().numpy(), d_ierr.cpu().numpy(), d_stats.cpu().numpy(), d_th.cpu().numpy()
        for k in range(nleg):
            assert (ierr[k] == code).all() and out[k].tobytes() == V.tobytes() and not stats[k].any() and not th[k].any(), name
        assert (out[nleg] == -7.25).all() and (ierr[nleg] == 77).all() and (stats[nleg] == 77).all() and (th[nleg] == -7.25).all(), name


# ---- 5. memory discipline
@pytest.mark.parametrize("mech", MECHS)
def test_s5_outputs_poison_absent_arrays_and_aliasing(chem, mech):
    """caller-owned outputs with one leg and one cell more than the call: the poison is intact outside, through the host and the device entry; ierr,
    stats and t_h each absent in turn (host entry), d_texit_hexit absent (device entry); var_in aliasing the last leg's block"""
    import torch
    V, F, K = _cells(mech)
    n, nvar = V.shape
    s = RS.series_set(mech, "ros3_unequal_carry")
    nleg = len(s.times) - 1
    want = _series(chem, mech, V, F, K, s)
    host_want = _series(chem, mech, V, F, K, s, host=True)
    L, mid = chem.lib(), MID[mech]
    opts = (s.atol.ctypes.data_as(_dp), s.rtol.ctypes.data_as(_dp), s.rpar.ctypes.data_as(_dp), s.ipar.ctypes.data_as(_ip))
    tp = s.times.ctypes.data_as(_dp)
    # the arrays hold nleg blocks of n cells back to back: one block and one cell's worth of poison behind them
    def bufs():
        return (np.full((nleg + 1) * n * nvar + nvar, -7.25), np.full((nleg + 1) * n + 1, 77, np.int32), np.full((nleg + 1) * n * 8 + 8, 77, np.int32),
                np.full((nleg + 1) * n * 3 + 3, -7.25))
    for absent in (None, "ierr", "stats", "t_h"):
        out, ierr, stats, th = bufs()
        rc = L.mistra_chem_rosenbrock_series_ex(mid, n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), nleg, tp, *opts, 1, None,
                                                out.ctypes.data_as(_dp), None if absent == "ierr" else ierr.ctypes.data_as(_ip),
                                                None if absent == "stats" else stats.ctypes.data_as(_ip), None if absent == "t_h" else th.ctypes.data_as(_dp))
        assert rc == 0, L.mistra_chem_last_error()
        assert out[:nleg * n * nvar].tobytes() == host_want.var.tobytes() and (out[nleg * n * nvar:] == -7.25).all(), absent
        assert (ierr == 77).all() if absent == "ierr" else (np.array_equal(ierr[:nleg * n], host_want.ierr.ravel()) and (ierr[nleg * n:] == 77).all()), absent
        assert (stats == 77).all() if absent == "stats" else (np.array_equal(stats[:nleg * n * 8], host_want.stats.ravel()) and (stats[nleg * n * 8:] == 77).all()), absent
        assert (th == -7.25).all() if absent == "t_h" else (th[:nleg * n * 3].tobytes() == host_want.t_h.tobytes() and (th[nleg * n * 3:] == -7.25).all()), absent
    dV, dF, dK = _T(V), _T(F), _T(K)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_th in (True, False):
        out, ierr, stats, th = bufs()
        d_out, d_ierr, d_stats, d_th = _T(out), _T(ierr), _T(stats), _T(th[:(nleg + 1) * n * 2 + 2])
        rc = L.mistra_chem_rosenbrock_series_device(mid, n, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), nleg, tp, *opts, d_out.data_ptr(), d_ierr.data_ptr(),
                                                    d_stats.data_ptr(), d_th.data_ptr() if with_th else None, 1, None, stream)
        assert rc == 0, L.mistra_chem_last_error()
        torch.cuda.synchronize()
        out, ierr, stats, th = d_out.cpu().numpy(), d_ierr.cpu().numpy(), d_stats.cpu().numpy(), d_th.cpu().numpy()
        assert out[:nleg * n * nvar].tobytes() == want.var.tobytes() and (out[nleg * n * nvar:] == -7.25).all()
        assert np.array_equal(ierr[:nleg * n], want.ierr.ravel()) and (ierr[nleg * n:] == 77).all()
        assert np.array_equal(stats[:nleg * n * 8], want.stats.ravel()) and (stats[nleg * n * 8:] == 77).all()
        assert (th[:nleg * n * 2].tobytes() == want.t_h.tobytes() and (th[nleg * n * 2:] == -7.25).all()) if with_th else (th == -7.25).all()
    # var_in is the last leg's block of var_series: every cell's inputs are read before any of its outputs is written
    d_out = torch.full((nleg, n, nvar), -7.25, dtype=torch.float64, device=dV.device)
    d_out[nleg - 1] = dV
    res = chem.rosenbrock_series(mech, d_out[nleg - 1], dF, dK, s.times, s.ipar, s.rpar, s.atol, s.rtol, carry_h=True, out=d_out)
    torch.cuda.synchronize()
    assert res.var.data_ptr() == d_out.data_ptr()
    _same(_np(res), want, "var_in aliases the last leg")
    h_out = np.full((nleg, n, nvar), -7.25)
    h_out[nleg - 1] = V
    ierr, stats, th = np.zeros((nleg, n), np.int32), np.zeros((nleg, n, 8), np.int32), np.zeros((nleg, n, 3))
    rc = L.mistra_chem_rosenbrock_series_ex(mid, n, h_out[nleg - 1].ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), nleg, tp, *opts, 1, None,
                                            h_out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp))
    assert rc == 0, L.mistra_chem_last_error()
    _same(chem.SeriesResult(h_out, ierr, stats, th), host_want, "host: var_in aliases the last leg")


# ---- 6. plumbing
def test_s6_series_queued_on_one_stream_each_run_with_their_own_times(chem):
    """two series with different times and nleg queued back to back on one stream, then nine in flight (one more than
    MISTRA_ROSENBROCK_CALLS_IN_FLIGHT = 8: the ring of blocks comes round): each equals its own synchronous result"""
    import torch
    mech = "tot"
    V, F, K = _cells(mech)
    a, b = RS.series_set(mech, "ros3_unequal"), RS.series_set(mech, "rodas4_rtol_1e-7")
    want = {"a": _series(chem, mech, V, F, K, a), "b": _series(chem, mech, V, F, K, b)}
    assert len(a.times) != len(b.times)
    dV, dF, dK = _T(V), _T(F), _T(K)
    torch.cuda.synchronize()
    queued = [chem.rosenbrock_series(mech, dV, dF, dK, x.times, x.ipar, x.rpar, x.atol, x.rtol, carry_h=x.carry) for x in (a, b)]
    torch.cuda.synchronize()
    _same(_np(queued[0]), want["a"], "first of two")
    _same(_np(queued[1]), want["b"], "second of two")
    mech = "gas"
    V, F, K = _cells(mech)
    dV, dF, dK = _T(V), _T(F), _T(K)
    grids = [np.linspace(0.0, 1.0 + i, 2 + i % 4) for i in range(9)]
    sets = [RS.method_series(mech, 1 + i % 5)._replace(times=t, carry=bool(i % 2)) for i, t in enumerate(grids)]
    want = [_series(chem, mech, V, F, K, x) for x in sets]
    torch.cuda.synchronize()
    queued = [chem.rosenbrock_series(mech, dV, dF, dK, x.times, x.ipar, x.rpar, x.atol, x.rtol, carry_h=x.carry) for x in sets]
    torch.cuda.synchronize()
    for i, (q, w) in enumerate(zip(queued, want)):
        _same(_np(q), w, "series %d of nine in flight" % i)


def test_s6_two_device_slots_ragged_split(chem):
    """init_devices([0, 0]), five tot cells over two slots (3 + 2): every slot gets its own rows and its own slices of every leg; shared and cells form"""
    mech = "tot"
    g = load_golden(mech)
    V, F, K = g["var_in"][:5], g["fix"][:5], g["rconst"][:5]
    s = RS.series_set(mech, "ros3_unequal_carry")
    at = np.array([[1.0e-25], [1.0e-20], [1.0e-22], [1.0e-18], [1.0e-24]])
    rt = np.array([[1.0e-3], [1.0e-4], [1.0], [1.0e-2], [2.0e-3]])      # cell 2: refused with -5, in the first slot's block
    hs = np.array([0.0, 0.5, 0.0, 1.0e-4, 0.2])
    one = _series(chem, mech, V, F, K, s, hstart=hs, host=True)
    one_cells = _series(chem, mech, V, F, K, s, atol=at, rtol=rt, host=True)
    assert (one.ierr == 1).all() and (one_cells.ierr[:, 2] == -5).all() and (one_cells.ierr[:, [0, 1, 3, 4]] == 1).all()
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    _same(_series(chem, mech, V, F, K, s, hstart=hs, host=True), one, "the split over two slots differs from one device")
    _same(_series(chem, mech, V, F, K, s, atol=at, rtol=rt, host=True), one_cells, "cells form over two slots")


def test_s6_cells_form_rows_and_batches(chem):
    """gas, Rodas3: vector rows per cell (NVAR wide) with every cell's row different, 65 cells — the cells' rows permuted with the cells give the
    permuted results; 65 cells equal the same cells in batches of 1 and 3"""
    mech = "gas"
    V3, F3, K3 = _cells(mech)
    n, nvar = 65, V3.shape[1]
    idx = np.arange(n) % 3
    rng = np.random.default_rng(11)
    V = V3[idx] * rng.uniform(0.9, 1.1, (n, 1))
    F, K = F3[idx], K3[idx]
    at = 1.0e-25 * 10.0 ** rng.uniform(0.0, 8.0, (n, nvar))
    rt = 10.0 ** rng.uniform(-4.0, -2.0, (n, nvar))
    ipar, rpar, _, _ = R.base_options(mech)
    ipar[1], ipar[3] = 0, 4
    s = RS.Series(ipar, rpar, None, None, np.array(RS.METHOD_GRID), True)
    full = _series(chem, mech, V, F, K, s, atol=at, rtol=rt)
    assert (full.ierr == 1).all()
    perm = rng.permutation(n)
    got = _series(chem, mech, V[perm], F[perm], K[perm], s, atol=at[perm], rtol=rt[perm])
    _same(got, type(full)(full.var[:, perm], full.ierr[:, perm], full.stats[:, perm], full.t_h[:, perm]), "rows travel with their cells")
    host = _series(chem, mech, V, F, K, s, atol=np.asfortranarray(at), rtol=np.asfortranarray(rt), host=True)      # (rows handed over transposed in memory)
    _same(type(host)(host.var, host.ierr, host.stats, host.t_h[..., :2].copy()), full, "host cells form")
    for lo, hi in ((0, 1), (64, 65), (1, 4), (61, 64)):
        part = _series(chem, mech, V[lo:hi], F[lo:hi], K[lo:hi], s, atol=at[lo:hi], rtol=rt[lo:hi])
        _same(part, type(full)(full.var[:, lo:hi], full.ierr[:, lo:hi], full.stats[:, lo:hi], full.t_h[:, lo:hi]), (lo, hi))
    # the shared-pair form likewise
    s2 = RS.method_series(mech, 2)
    full = _series(chem, mech, V, F, K, s2)
    for lo, hi in ((0, 1), (1, 4), (62, 65)):
        _same(_series(chem, mech, V[lo:hi], F[lo:hi], K[lo:hi], s2), type(full)(full.var[:, lo:hi], full.ierr[:, lo:hi], full.stats[:, lo:hi], full.t_h[:, lo:hi]), (lo, hi))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_s6_from_fortran(tmp_path):
    """shim/shim_driver ZT: ROSENBROCK_BATCH_SERIES_t and ROSENBROCK_BATCH_SERIES_CELLS_t on the Max_no_steps set — the host entry's bits, and
    ros_ErrorMsg_t's lines on unit 6 for every failed leg and cell"""
    from mistra_amd import chem
    mech, name = "tot", "ros3_max_steps_3"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, F, K = _cells(mech)
    s = RS.series_set(mech, name)
    n, nvar = V.shape
    nleg = len(s.times) - 1
    chem.init(0)
    want = _series(chem, mech, V, F, K, s, host=True)
    assert (want.ierr == -6).all()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    for ntol in (0, 1):      # 0: the shared pair; 1: one scalar row per cell (the same values)
        with open(fin, "wb") as f:
            np.concatenate([s.ipar.astype(np.float64), s.rpar, s.atol, s.rtol, [float(n), float(nleg), float(s.carry), float(ntol)], s.times]).tofile(f)
            for i in range(n):
                np.concatenate([V[i], F[i], K[i]]).tofile(f)
        r = subprocess.run([DRIVER, "ZT", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
        raw = np.fromfile(fout, np.float64)
        per = nvar + 2 + 9      # per leg and cell: VAR, Texit, Hexit, IERR, ISTAT(8)
        rows = raw.reshape(nleg, n, per)
        assert rows[..., :nvar].tobytes() == want.var.tobytes(), ntol
        assert rows[..., nvar:nvar + 2].tobytes() == want.t_h[..., :2].tobytes(), ntol
        assert np.array_equal(rows[..., nvar + 2].astype(np.int32), want.ierr) and np.array_equal(rows[..., nvar + 3:].astype(np.int32), want.stats), ntol
        assert r.stdout.count("Forced exit from Rosenbrock_t") == nleg * n and r.stdout.count("No of steps exceeds maximum bound") == nleg * n, r.stdout


# ---- 7. nothing else moved
def test_s7_nothing_else_moved(chem):
    """a plain integrate_ex, a rosenbrock call, the options in force and the zero-pivot record of the last call that is not a series: the same before
    and after a series"""
    mech = "aer"
    V, F, K = _cells(mech)
    held = R.option_set(mech, "factors")
    chem.set_options(mech, *held)
    before = (chem.integrate_ex(mech, V, F, K, 0.0, 10.0), chem.rosenbrock(mech, V, F, K, 0.0, 10.0, *RS.method_series(mech, 4)[:4]))
    for name in ("ros3_unequal_carry", "rodas4_rtol_1e-7"):
        s = RS.series_set(mech, name)
        _series(chem, mech, V, F, K, s, host=True)
        _series(chem, mech, V, F, K, s)
    o = chem.get_options(mech)
    assert all(np.array_equal(a, b) for a, b in zip(o, held))
    after = (chem.integrate_ex(mech, V, F, K, 0.0, 10.0), chem.rosenbrock(mech, V, F, K, 0.0, 10.0, *RS.method_series(mech, 4)[:4]))
    for (ra, ta), (rb, tb) in zip(before, after):
        assert ra.var.tobytes() == rb.var.tobytes() and np.array_equal(ra.ierr, rb.ierr) and np.array_equal(ra.stats, rb.stats) and ta.tobytes() == tb.tobytes()
    chem.clear_options(mech)
    # the series ignores the options in force: with them set it gave what it gives without
    s = RS.series_set(mech, "ros3_unequal")
    plain = _series(chem, mech, V, F, K, s)
    chem.set_options(mech, *held)
    _same(_series(chem, mech, V, F, K, s), plain, "options in force")
    chem.clear_options(mech)
    chem.set_policy(mech, 4, 1.0e-13)
    try:
        _same(_series(chem, mech, V, F, K, s), plain, "policy in force")
    finally:
        chem.clear_policy(mech)
