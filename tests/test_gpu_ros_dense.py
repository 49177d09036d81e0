"""Dense output of Rosenbrock_x on the GPU (-m gpu): mistra_chem_rosenbrock_dense_ex / _device and their cells forms.  The
integration is the sibling entry's bit for bit; the samples of a one-step call are exact against the formula on the oracle's Fun_x at the GPU's own end
state; whole calls are held to the restatement (tests/ros_dense_py.py) with identical counters and nout and the bounds of tests/ros_dense_bounds.py,
measured on the reference side by tests/test_ros_dense.py.  Three cells per launch (cells 0, n/2, n-1 of integrate_<mech>.npz) unless said otherwise, one
workgroup per cell."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ros_dense_bounds as db
import ros_dense_py as RD
import ros_flux_py as RF
import ros_methods_py as RM
from conftest import MECHS, REPO, load_golden

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}
METHODS = (1, 2, 3, 4, 5)


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


def _cells(mech):
    g = load_golden(mech)
    c = list(RD.cells_of(g["var_in"].shape[0]))
    return g["var_in"][c], g["fix"][c], g["rconst"][c]


def _batch(mech, n):
    """n cells: the three test cells in turn, each state scaled by a factor of its own (seeded)"""
    V3, F3, K3 = _cells(mech)
    idx = np.arange(n) % 3
    return V3[idx] * np.random.default_rng(5).uniform(0.9, 1.1, (n, 1)), F3[idx], K3[idx]


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _np(out):
    """(IntegrateResult, t_h[, samples, nout]) of tensors -> (var, ierr, stats, t_h[, samples, nout]) numpy arrays, after a synchronisation"""
    import torch
    torch.cuda.synchronize()
    res = out[0]
    return tuple(x.cpu().numpy() for x in (res.var, res.ierr, res.stats) + tuple(out[1:]))


def _host(out):
    """the host entry's tuple with t_h cut to the device entry's two columns"""
    return (out[0].var, out[0].ierr, out[0].stats, out[1][:, :2].copy()) + tuple(out[2:])


def _same(got, want, what=""):
    """var, ierr, stats, t_h — and samples, nout where both have them — bit for bit"""
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[2], want[2]), (what, got[2].tolist(), want[2].tolist())
    for i in (0, 3) + ((4, 5) if len(got) > 4 and len(want) > 4 else ()):
        assert got[i].shape == want[i].shape and got[i].tobytes() == want[i].tobytes(), (what, i)


def _prefix(samples, nout, what=""):
    """nout is a prefix: the rows behind it are +0.0 (bytes), the reached ones finite"""
    ns = samples.shape[0]
    for c, n in enumerate(nout):
        assert 0 <= n <= ns, (what, c, n)
        assert samples[n:, c].tobytes() == np.zeros((ns - n, samples.shape[2])).tobytes(), (what, c)
        assert np.isfinite(samples[:n, c]).all(), (what, c)


# ---- 1. the siblings
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mech", MECHS)
def test_d1_the_integration_is_the_siblings(chem, mech, method):
    """var, ierr, stats, t_h of the dense entry are chem.rosenbrock's bit for bit, 0 -> 10 s, through the device and the host entry; every sample is
    reached and the one at Tend is var bit for bit (th == 1)"""
    V, F, K = _cells(mech)
    opts = RM.method_set(mech, "m%d" % method)[:4]
    ts = RD.LINEAR8
    dV, dF, dK = _T(V), _T(F), _T(K)
    want = _np(chem.rosenbrock(mech, dV, dF, dK, 0.0, 10.0, *opts))
    got = _np(chem.rosenbrock_dense(mech, dV, dF, dK, 0.0, 10.0, ts, *opts))
    assert (want[1] == 1).all()
    _same(got, want, "device")
    assert got[4].shape == (8, 3, V.shape[1]) and (got[5] == 8).all() and np.isfinite(got[4]).all()
    assert got[4][-1].tobytes() == got[0].tobytes()
    hw = chem.rosenbrock(mech, V, F, K, 0.0, 10.0, *opts)
    hg = chem.rosenbrock_dense(mech, V, F, K, 0.0, 10.0, ts, *opts)
    assert hg[1].tobytes() == hw[1].tobytes()      # t_h [ncell, 3]: Texit, Hexit, H
    _same(_host(hg), _host(hw), "host")
    _same(_host(hg), got, "host against device")


# ---- 2. exact
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mech", MECHS)
def test_d2_one_step_samples_are_exact(chem, mech, method):
    """AbsTol = 1e30, RelTol = 0.5, 0 -> 1e-3 s: one attempt, accepted, and the samples at 2.5e-4, 5e-4, 1e-3 are the formula applied in numpy to Y_0,
    the call's var and the oracle's Fun_x at both, bit for bit.  Every one of the 15 kernels."""
    from oracle.oracle import Oracle
    o = Oracle(mech)
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RF.single_step_set(mech, method)
    var, ierr, stats, th, samples, nout = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), t0, t1, RD.SINGLE_TS, ipar, rpar, atol, rtol))
    assert (ierr == 1).all() and (stats[:, 2] == 1).all() and (stats[:, 3] == 1).all() and np.isfinite(var).all() and (nout == 3).all()
    assert (th[:, 0] == t1).all() and (th[:, 1] == 1.0e-3).all()
    for c in range(3):
        f0, f1 = o.fun(V[c], F[c], K[c]), o.fun(var[c], F[c], K[c])
        for k, tk in enumerate(RD.SINGLE_TS):
            want = RD.hermite(V[c], f0, var[c], f1, 1.0e-3, (tk - 0.0) / 1.0e-3)
            assert samples[k, c].tobytes() == want.tobytes(), (c, k, int((samples[k, c] != want).sum()))
        assert samples[2, c].tobytes() == var[c].tobytes() and samples[0, c].tobytes() != samples[1, c].tobytes()


# ---- 3. whole calls
@pytest.mark.parametrize("name", RD.DENSE_SETS)
@pytest.mark.parametrize("mech", MECHS)
def test_d3_whole_calls_against_the_restatement(chem, mech, name):
    """Per set of the bounds module, with the set's sample times: IERR, the counters and nout identical to the restatement's, the reached samples
    within ros_dense_bounds (rel_diff, and over the row maximum), the rows behind nout +0.0; the host entry gives the device entry's bits"""
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, name)
    ts = RD.times_of(name)
    want = RD.restated(mech, load_golden(mech), 0, (name,))[name]
    got = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), t0, t1, ts, ipar, rpar, atol, rtol))
    _same(_host(chem.rosenbrock_dense(mech, V, F, K, t0, t1, ts, ipar, rpar, atol, rtol)), got, name + " host")
    samples = got[4].transpose(1, 0, 2)      # [ncell, ns, NVAR] as the restatement keeps them
    d, s = db.sample_diff(samples, want[5], want[6]), db.scaled_diff(samples, want[5], want[6])
    print("%s %s: IERR %s, Nstp %s, nout %s of %d, samples %.3e (bound %.1e), over the row maximum %.3e (bound %.1e)" %
          (mech, name, got[1].tolist(), got[2][:, 2].tolist(), got[5].tolist(), len(ts), d, db.DENSE_RTOL[mech], s, db.DENSE_SCALED[mech]))
    assert np.array_equal(got[1], want[1]), (name, got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[2], want[2]), (name, got[2].tolist(), want[2].tolist())
    assert np.array_equal(got[5], want[6]), (name, got[5].tolist(), want[6].tolist())
    _prefix(got[4], got[5], name)
    assert d <= db.DENSE_RTOL[mech], (name, d)
    assert s <= db.DENSE_SCALED[mech], (name, s)


# ---- 4. edges
@pytest.mark.parametrize("mech", MECHS)
def test_d4_poisoned_outputs_are_fully_overwritten(chem, mech):
    """the Max_no_steps set (0 < nout < ns) through the raw entries, host and device, shared pair and cells form, into caller-owned outputs poisoned with
    NaN that have one row (one sample block) more than the call: every entry of the call's rows is written — the rows behind nout +0.0 — and what lies
    behind stays NaN"""
    import torch
    V, F, K = _cells(mech)
    n, nvar = V.shape
    ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, "m5_max_steps_5")
    ts = RD.MAX_STEPS
    ns = len(ts)
    want = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), t0, t1, ts, ipar, rpar, atol, rtol))
    assert ((0 < want[5]) & (want[5] < ns)).all() and (want[1] == -6).all()
    L, mid = chem.lib(), MID[mech]
    opts = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip))
    at, rt = np.full((n, 1), atol[0]), np.full((n, 1), rtol[0])      # the cells form with the same values: the same results

    def bufs(nth):
        return (np.full((n + 1, nvar), np.nan), np.full(n + 1, 77, np.int32), np.full((n + 1, 8), 77, np.int32), np.full((n + 1, nth), np.nan),
                np.full((ns + 1, n, nvar), np.nan), np.full(n + 1, 77, np.int32))

    def check(b, what, nth):
        out, ierr, stats, th, ys, nout = b
        assert out[:n].tobytes() == want[0].tobytes() and np.array_equal(ierr[:n], want[1]) and np.array_equal(stats[:n], want[2]), what
        assert th[:n, :2].tobytes() == want[3].tobytes() and np.isfinite(th[:n]).all(), what
        assert ys[:ns].tobytes() == want[4].tobytes() and np.array_equal(nout[:n], want[5]), what
        assert np.isnan(out[n:]).all() and ierr[n] == 77 and (stats[n] == 77).all() and np.isnan(th[n:]).all() and np.isnan(ys[ns:]).all() and nout[n] == 77, what
        _prefix(ys[:ns], nout[:n], what)
    for cells in (False, True):
        b = bufs(3)
        head = (mid, n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), t0, t1)
        tail = (b[0].ctypes.data_as(_dp), b[1].ctypes.data_as(_ip), b[2].ctypes.data_as(_ip), b[3].ctypes.data_as(_dp), ns, ts.ctypes.data_as(_dp),
                b[4].ctypes.data_as(_dp), b[5].ctypes.data_as(_ip))
        if cells:
            rc = L.mistra_chem_rosenbrock_dense_cells_ex(*head, at.ctypes.data_as(_dp), rt.ctypes.data_as(_dp), 1, *opts[2:], *tail)
        else:
            rc = L.mistra_chem_rosenbrock_dense_ex(*head, *opts, *tail)
        assert rc == 0, L.mistra_chem_last_error()
        check(b, "host, cells %s" % cells, 3)
        b = bufs(2)
        dV, dF, dK, d_at, d_rt = _T(V), _T(F), _T(K), _T(at), _T(rt)
        d = [_T(x) for x in b]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (mid, n, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), t0, t1)
        tail = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, stream, ns, ts.ctypes.data_as(_dp), d[4].data_ptr(), d[5].data_ptr())
        if cells:
            rc = L.mistra_chem_rosenbrock_dense_cells_device(*head, d_at.data_ptr(), d_rt.data_ptr(), 1, *opts[2:], *tail)
        else:
            rc = L.mistra_chem_rosenbrock_dense_device(*head, *opts, *tail)
        assert rc == 0, L.mistra_chem_last_error()
        torch.cuda.synchronize()
        check([x.cpu().numpy() for x in d], "device, cells %s" % cells, 2)


def test_d4_one_sample_and_the_most_a_call_takes(chem):
    """ns = 1 (Tend alone: var) on every mechanism; ns = MISTRA_DENSE_MAX_TIMES on gas, one cell: every sample reached, monotone times kept apart (the
    first and the last row are the restatement's within the bound, the last one var), and what ns = 8 gives at the same times, bit for bit"""
    for mech in MECHS:
        V, F, K = _cells(mech)
        opts = RM.method_set(mech, "m2")[:4]
        got = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.END, *opts))
        assert got[4].shape == (1, 3, V.shape[1]) and (got[5] == 1).all() and got[4][0].tobytes() == got[0].tobytes(), mech
    mech = "gas"
    V, F, K = (x[:1] for x in _cells(mech))
    opts = RM.method_set(mech, "m2")[:4]
    ts = np.linspace(0.0, 10.0, RD.MAX_TIMES + 1)[1:]
    assert ts.size == RD.MAX_TIMES and ts[-1] == 10.0 and ts[511] == 1.25
    got = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, ts, *opts))
    few = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *opts))
    assert (got[5] == RD.MAX_TIMES).all() and np.isfinite(got[4]).all() and got[4][-1].tobytes() == got[0].tobytes()
    _same(got[:4], few[:4], "the integration")
    assert np.array_equal(ts[511::512], RD.LINEAR8) and got[4][511::512].tobytes() == few[4].tobytes()
    host = chem.rosenbrock_dense(mech, V, F, K, 0.0, 10.0, ts, *opts)
    assert host[2].tobytes() == got[4].tobytes() and np.array_equal(host[3], got[5])


@pytest.mark.parametrize("mech", MECHS)
def test_d4_a_nan_cell_between_two_good_ones(chem, mech):
    """cell 1 all NaN: it ends with an error code, reaches no sample and has +0.0 rows; its neighbours' bytes are what they are without it"""
    V, F, K = _cells(mech)
    opts = RM.method_set(mech, "m2")[:4]
    good = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *opts))
    B = V.copy()
    B[1] = np.nan
    got = _np(chem.rosenbrock_dense(mech, _T(B), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *opts))
    sib = _np(chem.rosenbrock(mech, _T(B), _T(F), _T(K), 0.0, 10.0, *opts))
    assert np.array_equal(got[1], sib[1]) and np.array_equal(got[2], sib[2]) and got[1][1] < 0 and got[5].tolist() == [8, 0, 8]
    assert got[4][:, 1].tobytes() == np.zeros((8, V.shape[1])).tobytes()
    for i in (0, 3):
        assert got[i][[0, 2]].tobytes() == good[i][[0, 2]].tobytes()
    assert got[4][:, [0, 2]].tobytes() == good[4][:, [0, 2]].tobytes()


@pytest.mark.parametrize("mech", MECHS)
def test_d4_zero_pivots(chem, mech):
    """the crafted zero-pivot cell of the series tests (first-order losses with k = -1/(H*gamma) at the first step sizes), 0 -> 3e-3 s: one zero pivot —
    the call completes; six in a row — -8 in the first step, no accepted step, no sample.  IERR, the counters and nout are the restatement's, the
    integration the sibling's"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    from test_gpu_phases import GAMMA, _first_order_losses
    g, t = load_golden(mech), mechtab.load(mech)
    o = Oracle(mech)
    losses, seen = [], set()
    for r, sp in _first_order_losses(t):
        if sp not in seen:
            seen.add(sp)
            losses.append((r, sp))
    V, F = g["var_in"][:1].copy(), g["fix"][:1].copy()
    opts = RM.R.base_options(mech)
    ts = np.array([5.0e-4, 1.0e-3, 2.0e-3, 3.0e-3])
    for nzero, want_ierr in ((1, 1), (6, -8)):
        K = np.zeros((1, t.nreact))
        for i in range(nzero):
            K[0, losses[i][0]] = -1.0 / ((1.0e-3 / 2 ** i) * GAMMA[0])
        got = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 3.0e-3, ts, *opts))
        _same(got[:4], _np(chem.rosenbrock(mech, _T(V), _T(F), _T(K), 0.0, 3.0e-3, *opts)), nzero)
        want = RD.rosenbrock(o, t.diag, V[0], F[0], K[0], ts, *opts, 0.0, 3.0e-3)
        assert got[1][0] == want_ierr == want[1] and got[2][0, 7] == nzero and np.array_equal(got[2][0], want[2]), (nzero, got[1], got[2])
        assert got[5][0] == want[6] == (4 if nzero == 1 else 0), (nzero, got[5], want[6])
        _prefix(got[4], got[5], nzero)


def test_d4_refusals_stay_results(chem):
    """a call Rosenbrock_x refuses (-3) through both entries: the sibling's results, nout = 0 and +0.0 rows, a block behind untouched — nothing is
    launched (the device entry's var is a copy, its samples a memset).  A per-cell -5 row in the cells form affects that cell alone."""
    import torch
    mech = "gas"
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, "m3_rpar1_-1")
    want = chem.rosenbrock(mech, V, F, K, t0, t1, ipar, rpar, atol, rtol)
    host = chem.rosenbrock_dense(mech, V, F, K, t0, t1, RD.LINEAR8, ipar, rpar, atol, rtol)
    assert (want[0].ierr == -3).all()
    _same(_host(host)[:4], _host(want), "host")
    assert host[2].tobytes() == np.zeros((8, 3, V.shape[1])).tobytes() and host[3].tolist() == [0, 0, 0]
    L = chem.lib()
    ys, nout = _T(np.full((9, 3, V.shape[1]), np.nan)), _T(np.full(4, 77, np.int32))
    dV, dF, dK = _T(V), _T(F), _T(K)
    out, ierr, stats = torch.empty_like(dV), _T(np.zeros(3, np.int32)), _T(np.ones((3, 8), np.int32))
    rc = L.mistra_chem_rosenbrock_dense_device(MID[mech], 3, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), t0, t1, atol.ctypes.data_as(_dp),
                                               rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip), out.data_ptr(), ierr.data_ptr(),
                                               stats.data_ptr(), None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream), 8,
                                               RD.LINEAR8.ctypes.data_as(_dp), ys.data_ptr(), nout.data_ptr())
    assert rc == 0, L.mistra_chem_last_error()
    torch.cuda.synchronize()
    y, n = ys.cpu().numpy(), nout.cpu().numpy()
    assert (ierr.cpu().numpy() == -3).all() and out.cpu().numpy().tobytes() == V.tobytes() and not stats.cpu().numpy().any()
    assert y[:8].tobytes() == np.zeros((8, 3, V.shape[1])).tobytes() and np.isnan(y[8]).all() and n.tolist() == [0, 0, 0, 77]
    # per-cell -5
    for mech in MECHS:
        V, F, K = _cells(mech)
        opts = RM.method_set(mech, "m4")[:4]
        at, rt = np.full((3, 1), 1.0e-25), np.full((3, 1), 1.0e-3)
        good = _np(chem.rosenbrock_dense_cells(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, opts[0], opts[1], _T(at), _T(rt)))
        _same(good, _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *opts)), "rows of the shared pair")
        rt[1, 0] = 1.0      # RelTol >= 1: refused
        got = _np(chem.rosenbrock_dense_cells(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, opts[0], opts[1], _T(at), _T(rt)))
        sib = _np(chem.rosenbrock_cells(mech, _T(V), _T(F), _T(K), 0.0, 10.0, opts[0], opts[1], _T(at), _T(rt)))
        _same(got[:4], sib, mech)
        assert got[1].tolist() == [1, -5, 1] and got[5].tolist() == [8, 0, 8] and got[0][1].tobytes() == V[1].tobytes()
        assert got[4][:, 1].tobytes() == np.zeros((8, V.shape[1])).tobytes() and got[4][:, [0, 2]].tobytes() == good[4][:, [0, 2]].tobytes()
        hostc = chem.rosenbrock_dense_cells(mech, V, F, K, 0.0, 10.0, RD.LINEAR8, opts[0], opts[1], at, rt)
        _same(_host(hostc), got, mech + " host cells")


# ---- 5. plumbing
def test_d5_two_calls_queued_on_one_stream_each_get_their_own_times(chem):
    """two dense calls with different sample times, methods and intervals queued back to back on one stream, no synchronisation between: each equals
    its own synchronous result"""
    import torch
    mech = "aer"
    V, F, K = _cells(mech)
    a, b = RM.method_set(mech, "m2"), RM.method_set(mech, "m5_rtol_1e-5")
    calls = ((a[:4], 0.0, 2.0, np.array([0.5, 1.0, 2.0])), (b[:4], 0.0, 1.0, np.linspace(0.0, 1.0, 41)[1:]))
    dV, dF, dK = _T(V), _T(F), _T(K)
    want = [_np(chem.rosenbrock_dense(mech, dV, dF, dK, t0, t1, ts, *o)) for o, t0, t1, ts in calls]
    assert (want[0][5] == 3).all() and (want[1][5] == 40).all()
    torch.cuda.synchronize()
    queued = [chem.rosenbrock_dense(mech, dV, dF, dK, t0, t1, ts, *o) for o, t0, t1, ts in calls]
    for q, w, what in zip(queued, want, ("first of two", "second of two")):
        _same(_np(q), w, what)


def test_d5_three_device_slots_split_65_cells(chem):
    """init_devices([0, 0, 0]): 65 tot cells, ragged over three slots, give the one-device results bit for bit, shared pair and cells form (one row
    refused by -5 in a later slot's block); the sample blocks land in the caller's [ns][65] layout"""
    mech = "tot"
    V, F, K = _batch(mech, 65)
    ipar, rpar, atol, rtol = RM.method_set(mech, "m2")[:4]
    ts = np.array([0.25, 0.5, 1.0])
    at, rt = np.full((65, 1), 1.0e-25), np.full((65, 1), 1.0e-3)
    rt[40, 0] = 1.0
    one = _host(chem.rosenbrock_dense(mech, V, F, K, 0.0, 1.0, ts, ipar, rpar, atol, rtol))
    one_cells = _host(chem.rosenbrock_dense_cells(mech, V, F, K, 0.0, 1.0, ts, ipar, rpar, at, rt))
    assert (one[1] == 1).all() and (one[5] == 3).all() and one[4][2].tobytes() == one[0].tobytes()
    assert one_cells[1][40] == -5 and one_cells[5][40] == 0 and (np.delete(one_cells[5], 40) == 3).all()
    assert one_cells[4][:, 39].tobytes() == one[4][:, 39].tobytes() and not one_cells[4][:, 40].any()
    _same(_np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 1.0, ts, ipar, rpar, atol, rtol)), one, "device against host")
    chem.finalize()
    chem.init_devices([0, 0, 0])
    assert chem.device_count() == 3
    _same(_host(chem.rosenbrock_dense(mech, V, F, K, 0.0, 1.0, ts, ipar, rpar, atol, rtol)), one, "the split over three slots differs from one device")
    _same(_host(chem.rosenbrock_dense_cells(mech, V, F, K, 0.0, 1.0, ts, ipar, rpar, at, rt)), one_cells, "cells form over three slots")


@pytest.mark.parametrize("mech", MECHS)
def test_d5_cells_forms_and_hstart(chem, mech):
    """the cells forms with ntol = 1 and ntol = NVAR (vector tolerances) are rosenbrock_cells' integration bit for bit, host and device; d_hstart per
    cell gives the sibling's integration with the same d_hstart, and the cell whose entry is 0 runs as without one, a sample at 2e-5 s included"""
    V, F, K = _cells(mech)
    nvar = V.shape[1]
    ts = RD.LINEAR8
    ipar, rpar, atol, rtol = RM.method_set(mech, "m4")[:4]
    vip, vrp, vat, vrt = RM.method_set(mech, "m4_vector_tol")[:4]
    rows1 = (ipar, rpar, np.array([[1.0e-25], [1.0e-20], [1.0e-18]]), np.array([[1.0e-3], [1.0e-4], [1.0e-2]]))
    rowsv = (vip, vrp, np.tile(vat, (3, 1)) * np.array([[1.0], [10.0], [0.1]]), np.tile(vrt, (3, 1)))
    assert rowsv[2].shape == (3, nvar)
    for what, (ip, rp, at, rt) in (("ntol = 1", rows1), ("ntol = NVAR", rowsv)):
        want = _np(chem.rosenbrock_cells(mech, _T(V), _T(F), _T(K), 0.0, 10.0, ip, rp, _T(at), _T(rt)))
        got = _np(chem.rosenbrock_dense_cells(mech, _T(V), _T(F), _T(K), 0.0, 10.0, ts, ip, rp, _T(at), _T(rt)))
        assert (want[1] == 1).all(), what
        _same(got[:4], want, what)
        assert (got[5] == 8).all() and got[4][-1].tobytes() == got[0].tobytes(), what
        _same(_host(chem.rosenbrock_dense_cells(mech, V, F, K, 0.0, 10.0, ts, ip, rp, at, rt)), got, what + " host")
    hs = _T(np.array([1.0e-4, 0.0, 5.0e-5]))      # cell 1: <= 0, the options' Hstart
    early = np.concatenate([[2.0e-5], RD.LINEAR8])
    want = _np(chem.rosenbrock(mech, _T(V), _T(F), _T(K), 0.0, 10.0, ipar, rpar, atol, rtol, hstart=hs))
    got = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, early, ipar, rpar, atol, rtol, hstart=hs))
    plain = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, early, ipar, rpar, atol, rtol))
    _same(got[:4], want, "d_hstart")
    assert (got[5] == 9).all() and got[4][-1].tobytes() == got[0].tobytes()
    for i in (0, 3, 4):      # cell 1 runs as without a d_hstart, samples included
        assert got[i][..., 1, :].tobytes() == plain[i][..., 1, :].tobytes(), i
    gotc = _np(chem.rosenbrock_dense_cells(mech, _T(V), _T(F), _T(K), 0.0, 10.0, early, ipar, rpar, _T(np.full((3, 1), atol[0])), _T(np.full((3, 1), rtol[0])),
                                           hstart=hs))
    _same(gotc, got, "d_hstart, cells form")


@pytest.mark.parametrize("mech", MECHS)
def test_d5_first_call_of_a_library_initialised_anew(chem, mech):
    """finalize, init: no kernel of the mechanism is configured, and the first call of each method is a dense one — the first user of its own
    configuration flag (a kernel whose dynamic LDS was never configured fails its launch).  Each returns IERR 1 and the plain call's bits, made after"""
    chem.finalize()
    chem.init(0)
    V, F, K = (_T(x[:2]) for x in _cells(mech))
    sets = {m: RM.method_set(mech, "m%d" % m)[:4] for m in METHODS}
    dense = {m: _np(chem.rosenbrock_dense(mech, V, F, K, 0.0, 10.0, RD.LINEAR8, *sets[m])) for m in METHODS}
    for m in METHODS:
        plain = _np(chem.rosenbrock(mech, V, F, K, 0.0, 10.0, *sets[m]))
        assert (dense[m][1] == 1).all() and (dense[m][5] == 8).all(), (m, dense[m][1].tolist())
        _same(dense[m][:4], plain, m)
    assert len({dense[m][0].tobytes() for m in METHODS}) == len(METHODS)


# ---- 6. Fortran
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_d6_from_fortran(tmp_path):
    """shim/shim_driver IT and IG: ROSENBROCK_BATCH_DENSE_t (the pair) and ROSENBROCK_BATCH_DENSE_CELLS_g (one scalar row per cell) on the Max_no_steps
    set — the host entry's bits, YS and NOUT included, and ros_ErrorMsg_x's lines on unit 6 for every cell"""
    from mistra_amd import chem
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    chem.init(0)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    for mech, mode, ntol, sfx in (("tot", "IT", 0, "t"), ("gas", "IG", 1, "g")):
        V, F, K = _cells(mech)
        ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, "m5_max_steps_5")
        ts = RD.MAX_STEPS
        n, nvar = V.shape
        want = _host(chem.rosenbrock_dense(mech, V, F, K, t0, t1, ts, ipar, rpar, atol, rtol))
        assert (want[1] == -6).all() and ((0 < want[5]) & (want[5] < len(ts))).all()
        with open(fin, "wb") as f:
            np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [t0, t1, float(n), float(ntol), float(len(ts))], ts]).tofile(f)
            for i in range(n):
                np.concatenate([V[i], F[i], K[i]]).tofile(f)
        r = subprocess.run([DRIVER, mode, str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
        raw = np.fromfile(fout, np.float64)
        per = nvar + 2 + 9 + 1
        rows, ys = raw[:n * per].reshape(n, per), raw[n * per:].reshape(len(ts), n, nvar)
        assert rows[:, :nvar].tobytes() == want[0].tobytes(), mode
        assert rows[:, nvar:nvar + 2].tobytes() == want[3].tobytes(), mode
        assert np.array_equal(rows[:, nvar + 2].astype(np.int32), want[1]) and np.array_equal(rows[:, nvar + 3:nvar + 11].astype(np.int32), want[2]), mode
        assert np.array_equal(rows[:, nvar + 11].astype(np.int32), want[5]) and ys.tobytes() == want[4].tobytes(), mode
        assert r.stdout.count("Forced exit from Rosenbrock_" + sfx) == n and r.stdout.count("No of steps exceeds maximum bound") == n, r.stdout


# ---- 7. nothing else moved
def test_d7_nothing_else_moved(chem):
    """the product call, a rosenbrock call, the options in force, a series and a flux call: the same bytes before and after dense calls through both
    entries; and a dense call ignores the options and the policy in force"""
    mech = "aer"
    V, F, K = _cells(mech)
    held = RM.R.option_set(mech, "factors")
    chem.set_options(mech, *held)
    o4 = RM.method_set(mech, "m4")[:4]
    times = [0.0, 2.5, 10.0]

    def others():
        s = chem.rosenbrock_series(mech, V, F, K, times, *o4)
        fl = chem.rosenbrock_flux(mech, V, F, K, 0.0, 10.0, *o4)
        return (chem.integrate_ex(mech, V, F, K, 0.0, 10.0), chem.rosenbrock(mech, V, F, K, 0.0, 10.0, *o4)), (s.var, s.ierr, s.stats), (fl[0].var, fl[2])
    before = others()
    for name in ("m2", "m5_max_steps_5"):
        ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, name)
        chem.rosenbrock_dense(mech, V, F, K, t0, t1, RD.times_of(name), ipar, rpar, atol, rtol)
        _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), t0, t1, RD.times_of(name), ipar, rpar, atol, rtol))
    o = chem.get_options(mech)
    assert all(np.array_equal(a, b) for a, b in zip(o, held))
    after = others()
    for (ra, ta), (rb, tb) in zip(before[0], after[0]):
        assert ra.var.tobytes() == rb.var.tobytes() and np.array_equal(ra.ierr, rb.ierr) and np.array_equal(ra.stats, rb.stats) and ta.tobytes() == tb.tobytes()
    for a, b in zip(before[1] + before[2], after[1] + after[2]):
        assert a.tobytes() == b.tobytes()
    chem.clear_options(mech)
    plain = _np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *o4))
    chem.set_options(mech, *held)
    _same(_np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *o4)), plain, "options in force")
    chem.clear_options(mech)
    chem.set_policy(mech, 4, 1.0e-13)
    try:
        _same(_np(chem.rosenbrock_dense(mech, _T(V), _T(F), _T(K), 0.0, 10.0, RD.LINEAR8, *o4)), plain, "policy in force")
    finally:
        chem.clear_policy(mech)
