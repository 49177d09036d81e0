"""The reaction flux of Rosenbrock_x on the GPU (-m gpu): mistra_chem_rosenbrock_flux_ex / _device and their cells forms.  The
integration is the sibling entry's bit for bit; the flux of a one-step call is exact against the oracle's products at the GPU's own end state; whole
calls are held to the restatement (tests/ros_flux_py.py) with identical counters and the bounds of tests/ros_flux_bounds.py, measured on the reference
side by tests/test_ros_flux.py.  Three cells per launch (cells 0, n/2, n-1 of integrate_<mech>.npz), 1 / 3 / 65 where batch edges are the subject."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ros_flux_bounds as fb
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
    c = list(RF.cells_of(g["var_in"].shape[0]))
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
    """(IntegrateResult, t_h[, flux]) of tensors -> (var, ierr, stats, t_h[, flux]) numpy arrays, after a synchronisation"""
    import torch
    torch.cuda.synchronize()
    res = out[0]
    return tuple(x.cpu().numpy() for x in (res.var, res.ierr, res.stats) + tuple(out[1:]))


def _host(out):
    return (out[0].var, out[0].ierr, out[0].stats) + tuple(out[1:])


def _same(got, want, what=""):
    """var, ierr, stats, t_h (and flux where both have one) bit for bit"""
    assert np.array_equal(got[1], want[1]), (what, got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[2], want[2]), (what, got[2].tolist(), want[2].tolist())
    for i in (0, 3) + ((4,) if len(got) > 4 and len(want) > 4 else ()):
        assert got[i].shape == want[i].shape and got[i].tobytes() == want[i].tobytes(), (what, i)


# ---- 1. the siblings
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mech", MECHS)
def test_f1_the_integration_is_the_siblings(chem, mech, method):
    """var_out, ierr, stats and d_texit_hexit of the flux entry are mistra_chem_rosenbrock_device's bit for bit, 0 -> 10 s; the cells form is
    _cells_device's, with one row refused by -5 whose flux row is zero, its state untouched"""
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = RM.method_set(mech, "m%d" % method)[:4]
    dV, dF, dK = _T(V), _T(F), _T(K)
    want = _np(chem.rosenbrock(mech, dV, dF, dK, 0.0, 10.0, ipar, rpar, atol, rtol))
    got = _np(chem.rosenbrock_flux(mech, dV, dF, dK, 0.0, 10.0, ipar, rpar, atol, rtol))
    assert (want[1] == 1).all()
    _same(got, want, "shared pair")
    assert got[4].shape == (3, K.shape[1]) and np.isfinite(got[4]).all() and (np.abs(got[4]).max(axis=1) > 0).all()
    at = np.array([[1.0e-25], [1.0e-20], [1.0e-18]])
    rt = np.array([[1.0e-3], [1.0], [1.0e-2]])      # cell 1: RelTol = 1 is refused, -5
    want = _np(chem.rosenbrock_cells(mech, dV, dF, dK, 0.0, 10.0, ipar, rpar, _T(at), _T(rt)))
    got = _np(chem.rosenbrock_flux_cells(mech, dV, dF, dK, 0.0, 10.0, ipar, rpar, _T(at), _T(rt)))
    assert want[1].tolist() == [1, -5, 1]
    _same(got, want, "cells")
    assert got[0][1].tobytes() == V[1].tobytes()
    assert got[4][1].tobytes() == np.zeros(K.shape[1]).tobytes() and (np.abs(got[4][[0, 2]]).max(axis=1) > 0).all()


# ---- 2. exact
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("mech", MECHS)
def test_f2_one_step_flux_is_exact(chem, mech, method):
    """AbsTol = 1e30, RelTol = 0.5, 0 -> 1e-3 s: one attempt, accepted, and flux = (0.5 * 1e-3) * (A(Y_0) + A(var_out)) bit for bit, A the oracle's
    products (Oracle.work behind Oracle.fun) at the GPU's own var_out.  Every one of the 15 kernels."""
    from oracle.oracle import Oracle
    o = Oracle(mech)
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RF.single_step_set(mech, method)
    var, ierr, stats, th, flux = _np(chem.rosenbrock_flux(mech, _T(V), _T(F), _T(K), t0, t1, ipar, rpar, atol, rtol))
    assert (ierr == 1).all() and (stats[:, 2] == 1).all() and (stats[:, 3] == 1).all() and np.isfinite(var).all()
    assert (th[:, 0] == t1).all() and (th[:, 1] == 1.0e-3).all()
    for c in range(3):
        a0 = RF.products(o, V[c], F[c], K[c])[1]
        a1 = RF.products(o, var[c], F[c], K[c])[1]
        want = (0.5 * 1.0e-3) * (a0 + a1)
        assert np.abs(want).max() > 0
        assert flux[c].tobytes() == want.tobytes(), (c, int((flux[c] != want).sum()), fb.flux_diff(flux[c], want))


# ---- 3. whole calls
@pytest.mark.parametrize("name", RF.FLUX_SETS)
@pytest.mark.parametrize("mech", MECHS)
def test_f3_whole_calls_against_the_restatement(chem, mech, name):
    """Per set of the bounds module: IERR and the counters identical to the restatement's, the flux within ros_flux_bounds.FLUX_RTOL; the host entry
    gives the device entry's bits"""
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, name)
    want = RF.restated(mech, load_golden(mech), 0, (name,))[name]
    got = _np(chem.rosenbrock_flux(mech, _T(V), _T(F), _T(K), t0, t1, ipar, rpar, atol, rtol))
    host = _host(chem.rosenbrock_flux(mech, V, F, K, t0, t1, ipar, rpar, atol, rtol))
    _same((host[0], host[1], host[2], host[3][:, :2].copy(), host[4]), got, name + " host")
    d = fb.flux_diff(got[4], want[5])
    print("%s %s: IERR %s, Nstp %s, flux %.3e from the restatement (bound %.1e)" % (mech, name, got[1].tolist(), got[2][:, 2].tolist(), d, fb.FLUX_RTOL[mech]))
    assert np.array_equal(got[1], want[1]), (name, got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[2], want[2]), (name, got[2].tolist(), want[2].tolist())
    assert d <= fb.FLUX_RTOL[mech], (name, d)


# ---- 4. batch edges
@pytest.mark.parametrize("n", (1, 3, 65))
@pytest.mark.parametrize("mech", MECHS)
def test_f4_host_and_device_entries_and_poisoned_outputs(chem, mech, n):
    """1 / 3 / 65 cells, Rodas3, 0 -> 1 s: the host entry equals the device entry bit for bit; caller-owned outputs with one row more than the call,
    poisoned: every entry of the call's rows is written, the row behind is untouched, through the host and the device entry (shared pair and cells)"""
    import torch
    V, F, K = _batch(mech, n)
    nvar, nreact = V.shape[1], K.shape[1]
    ipar, rpar, atol, rtol = RM.method_set(mech, "m4")[:4]
    want = _np(chem.rosenbrock_flux(mech, _T(V), _T(F), _T(K), 0.0, 1.0, ipar, rpar, atol, rtol))
    host = _host(chem.rosenbrock_flux(mech, V, F, K, 0.0, 1.0, ipar, rpar, atol, rtol))
    assert (want[1] == 1).all()
    _same((host[0], host[1], host[2], host[3][:, :2].copy(), host[4]), want, "host against device")
    L, mid = chem.lib(), MID[mech]
    opts = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip))
    at, rt = np.full((n, 1), atol[0]), np.full((n, 1), rtol[0])      # the cells form with the same values: the same results

    def bufs(nth):
        return (np.full((n + 1, nvar), -7.25), np.full(n + 1, 77, np.int32), np.full((n + 1, 8), 77, np.int32), np.full((n + 1, nth), -7.25),
                np.full((n + 1, nreact), -7.25))

    def check(b, w, what):
        for x, y, poison in zip(b, w, (-7.25, 77, 77, -7.25, -7.25)):
            assert x[:n].tobytes() == y.tobytes(), what
            assert (x[n:] == poison).all(), what
    for cells in (False, True):
        out, ierr, stats, th, flux = bufs(3)
        head = (mid, n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), 0.0, 1.0)
        tail = (out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp), flux.ctypes.data_as(_dp))
        if cells:
            rc = L.mistra_chem_rosenbrock_flux_cells_ex(*head, at.ctypes.data_as(_dp), rt.ctypes.data_as(_dp), 1, *opts[2:], *tail)
        else:
            rc = L.mistra_chem_rosenbrock_flux_ex(*head, *opts, *tail)
        assert rc == 0, L.mistra_chem_last_error()
        check((out, ierr, stats, th, flux), host, "host, cells %s" % cells)
        out, ierr, stats, th, flux = bufs(2)
        dV, dF, dK, d_at, d_rt = _T(V), _T(F), _T(K), _T(at), _T(rt)
        d = [_T(x) for x in (out, ierr, stats, th, flux)]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (mid, n, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), 0.0, 1.0)
        tail = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, stream, d[4].data_ptr())
        if cells:
            rc = L.mistra_chem_rosenbrock_flux_cells_device(*head, d_at.data_ptr(), d_rt.data_ptr(), 1, *opts[2:], *tail)
        else:
            rc = L.mistra_chem_rosenbrock_flux_device(*head, *opts, *tail)
        assert rc == 0, L.mistra_chem_last_error()
        torch.cuda.synchronize()
        check([x.cpu().numpy() for x in d], want, "device, cells %s" % cells)


def test_f4_refused_call_returns_zeros_and_launches_nothing(chem):
    """a call Rosenbrock_x refuses (-3) through both entries: the siblings' results, the flux rows +0.0, a row behind untouched"""
    mech = "gas"
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, "m3_rpar1_-1")
    want = _host(chem.rosenbrock(mech, V, F, K, t0, t1, ipar, rpar, atol, rtol))
    host = _host(chem.rosenbrock_flux(mech, V, F, K, t0, t1, ipar, rpar, atol, rtol))
    assert (want[1] == -3).all()
    _same(host, want, "host")
    assert host[4].tobytes() == np.zeros_like(host[4]).tobytes()
    import torch
    L = chem.lib()
    flux = _T(np.full((4, K.shape[1]), -7.25))
    dV, dF, dK = _T(V), _T(F), _T(K)
    out, ierr, stats = torch.empty_like(dV), _T(np.zeros(3, np.int32)), _T(np.zeros((3, 8), np.int32))
    rc = L.mistra_chem_rosenbrock_flux_device(MID[mech], 3, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), t0, t1, atol.ctypes.data_as(_dp),
                                              rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip), out.data_ptr(), ierr.data_ptr(),
                                              stats.data_ptr(), None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream), flux.data_ptr())
    assert rc == 0, L.mistra_chem_last_error()
    torch.cuda.synchronize()
    f = flux.cpu().numpy()
    assert (ierr.cpu().numpy() == -3).all() and out.cpu().numpy().tobytes() == V.tobytes()
    assert f[:3].tobytes() == np.zeros((3, K.shape[1])).tobytes() and (f[3] == -7.25).all()


def test_f4_two_device_slots_split_65_cells(chem):
    """init_devices([0, 0]): 65 tot cells over two slots (33 + 32) give the one-device results bit for bit, shared pair and cells form (one row
    refused by -5 in the second slot's block)"""
    mech = "tot"
    V, F, K = _batch(mech, 65)
    ipar, rpar, atol, rtol = RM.method_set(mech, "m2")[:4]
    at, rt = np.full((65, 1), 1.0e-25), np.full((65, 1), 1.0e-3)
    rt[40, 0] = 1.0
    one = _host(chem.rosenbrock_flux(mech, V, F, K, 0.0, 1.0, ipar, rpar, atol, rtol))
    one_cells = _host(chem.rosenbrock_flux_cells(mech, V, F, K, 0.0, 1.0, ipar, rpar, at, rt))
    assert (one[1] == 1).all() and one_cells[1][40] == -5 and (np.delete(one_cells[1], 40) == 1).all()
    assert one_cells[4][40].tobytes() == np.zeros(K.shape[1]).tobytes() and one_cells[4][39].tobytes() == one[4][39].tobytes()
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    _same(_host(chem.rosenbrock_flux(mech, V, F, K, 0.0, 1.0, ipar, rpar, atol, rtol)), one, "the split over two slots differs from one device")
    _same(_host(chem.rosenbrock_flux_cells(mech, V, F, K, 0.0, 1.0, ipar, rpar, at, rt)), one_cells, "cells form over two slots")


def test_f4_two_calls_queued_on_one_stream_each_get_their_own_options(chem):
    """two flux calls with different methods, tolerances and intervals queued back to back on one stream, no synchronisation between: each equals its
    own synchronous result"""
    import torch
    mech = "aer"
    V, F, K = _cells(mech)
    a, b = RM.method_set(mech, "m2"), RM.method_set(mech, "m5_rtol_1e-5")
    calls = ((a[:4], 0.0, 2.0), (b[:4], 0.0, 1.0))
    dV, dF, dK = _T(V), _T(F), _T(K)
    want = [_np(chem.rosenbrock_flux(mech, dV, dF, dK, t0, t1, *o)) for o, t0, t1 in calls]
    assert want[0][4].tobytes() != want[1][4].tobytes()
    torch.cuda.synchronize()
    queued = [chem.rosenbrock_flux(mech, dV, dF, dK, t0, t1, *o) for o, t0, t1 in calls]
    for q, w, what in zip(queued, want, ("first of two", "second of two")):
        _same(_np(q), w, what)


# ---- 5. Fortran
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_f5_from_fortran(tmp_path):
    """shim/shim_driver WT: ROSENBROCK_BATCH_FLUX_t and ROSENBROCK_BATCH_FLUX_CELLS_t on the Max_no_steps set — the host entry's bits, FLUX included,
    and ros_ErrorMsg_t's lines on unit 6 for every cell"""
    from mistra_amd import chem
    mech, name = "tot", "m5_max_steps_5"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol, t0, t1 = RM.method_set(mech, name)
    n, nvar = V.shape
    nreact = K.shape[1]
    chem.init(0)
    want = _host(chem.rosenbrock_flux(mech, V, F, K, t0, t1, ipar, rpar, atol, rtol))
    assert (want[1] == -6).all() and (np.abs(want[4]).max(axis=1) > 0).all()
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    for ntol in (0, 1):      # 0: the shared pair; 1: one scalar row per cell (the same values)
        with open(fin, "wb") as f:
            np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [t0, t1, float(n), float(ntol)]]).tofile(f)
            for i in range(n):
                np.concatenate([V[i], F[i], K[i]]).tofile(f)
        r = subprocess.run([DRIVER, "WT", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
        rows = np.fromfile(fout, np.float64).reshape(n, nvar + 2 + 9 + nreact)
        assert rows[:, :nvar].tobytes() == want[0].tobytes(), ntol
        assert rows[:, nvar:nvar + 2].tobytes() == want[3][:, :2].tobytes(), ntol
        assert np.array_equal(rows[:, nvar + 2].astype(np.int32), want[1]) and np.array_equal(rows[:, nvar + 3:nvar + 11].astype(np.int32), want[2]), ntol
        assert rows[:, nvar + 11:].tobytes() == want[4].tobytes(), ntol
        assert r.stdout.count("Forced exit from Rosenbrock_t") == n and r.stdout.count("No of steps exceeds maximum bound") == n, r.stdout
