"""Rosenbrock_x on the GPU with all five methods (-m gpu): mistra_chem_rosenbrock_ex / _device run one call of Rosenbrock_x per cell with the call's
own IPAR, RPAR, AbsTol, RelTol — Ros3 in the options kernel, Ros2, Ros4, Rodas3 and Rodas4 in method kernels of their own.  Expected values: the
compiled reference's Rosenbrock_x on the same sets and cells (tests/golden/ros_methods_<mech>.npz); bounds: tests/ros_methods_bounds.py, measured on
the reference side (tests/test_ros_methods.py).  One to three cells per launch unless a test says otherwise: cells 0, n/2, n-1 of
integrate_<mech>.npz."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ros_methods_bounds as mb
import ros_methods_py as RM
import ros_options_py as R
from conftest import MECHS, REPO, load_golden

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


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
    c = list(RM.cells_of(g["var_in"].shape[0]))
    return g["var_in"][c], g["fix"][c], g["rconst"][c]


def _fixture(mech):
    return dict(np.load(os.path.join(REPO, "tests", "golden", "ros_methods_%s.npz" % mech)))


def _same(a, b):
    (ra, ta), (rb, tb) = a, b
    return ra.var.tobytes() == rb.var.tobytes() and np.array_equal(ra.ierr, rb.ierr) and np.array_equal(ra.stats, rb.stats) and ta.tobytes() == tb.tobytes()


def _run(chem, mech, name, V, F, K):
    ipar, rpar, atol, rtol, tstart, tend = RM.method_set(mech, name)
    return chem.rosenbrock(mech, V, F, K, tstart, tend, ipar, rpar, atol, rtol)


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _host(res):
    (r, th) = res
    return type(r)(r.var.cpu().numpy(), r.ierr.cpu().numpy(), r.stats.cpu().numpy()), th.cpu().numpy()


def _run_device(chem, mech, name, V, F, K, hstart=None, sync=True):
    import torch
    ipar, rpar, atol, rtol, tstart, tend = RM.method_set(mech, name)
    res = chem.rosenbrock(mech, _T(V), _T(F), _T(K), tstart, tend, ipar, rpar, atol, rtol, hstart=None if hstart is None else _T(hstart))
    if not sync:
        return res
    torch.cuda.synchronize()
    return _host(res)


@pytest.mark.parametrize("mech", MECHS)
def test_g1_ros3_through_the_entry_is_the_options_kernel(chem, mech):
    """Ros3 with every option set of ros_options_py: var, ierr, stats, t_h bit-identical to set_options + integrate_ex; the options in force are
    neither read nor changed by the call; a plain integrate_ex afterwards gives the product kernel's bits."""
    V, F, K = _cells(mech)
    product = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    want = {}
    for name in R.SET_NAMES:
        chem.set_options(mech, *R.option_set(mech, name))
        want[name] = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    chem.clear_options(mech)
    for name in R.SET_NAMES:
        assert chem.get_options(mech) is None
        got = chem.rosenbrock(mech, V, F, K, R.TIN, R.TOUT, *R.option_set(mech, name))
        assert _same(got, want[name]), name
    assert chem.get_options(mech) is None
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), product)
    # with options in force: the call runs with its own, they stay as they are and keep governing integrate_ex
    held = R.option_set(mech, "factors")
    chem.set_options(mech, *held)
    assert _same(chem.rosenbrock(mech, V, F, K, R.TIN, R.TOUT, *R.option_set(mech, "hmax_0.5")), want["hmax_0.5"])
    assert _same(chem.rosenbrock(mech, V, F, K, R.TIN, R.TOUT), product), "None must mean INTEGRATE_x's values, not the options in force"
    o = chem.get_options(mech)
    assert all(np.array_equal(a, b) for a, b in zip(o, held))
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), want["factors"])


@pytest.mark.parametrize("name", RM.SET_NAMES)
@pytest.mark.parametrize("mech", MECHS)
def test_g2_method_sets_against_the_compiled_rosenbrock(chem, mech, name):
    """Per set: IERR and /Statistics/ identical to Rosenbrock_x's, VAR within METHODS_RTOL, exit time and last accepted step size within
    METHODS_TH_RTOL; the device entry gives the host entry's bits; one set per mechanism also alone (ncell = 1)."""
    V, F, K = _cells(mech)
    z = _fixture(mech)
    tstart, tend = RM.method_set(mech, name)[4:]
    res, th = _run(chem, mech, name, V, F, K)
    d_var = mb.var_diff(res.var, z[name + "_var"])
    d_te, d_he = mb.th_diff(th[:, 0], th[:, 1], z[name + "_rpar"][:, 0], z[name + "_rpar"][:, 1], tstart, tend)
    print("%s %s: VAR %.3e (bound %.1e), exit time %.3e, last step size %.3e (bound %.1e), Nstp %s, IERR %s" %
          (mech, name, d_var, mb.METHODS_RTOL[mech], d_te, d_he, mb.METHODS_TH_RTOL[mech], res.stats[:, 2].tolist(), res.ierr.tolist()))
    assert np.array_equal(res.ierr, z[name + "_ierr"]), (res.ierr, z[name + "_ierr"])
    assert np.array_equal(res.stats, z[name + "_ipar"]), (res.stats, z[name + "_ipar"])
    assert d_var <= mb.METHODS_RTOL[mech]
    assert d_te <= mb.METHODS_TH_RTOL[mech] and d_he <= mb.METHODS_TH_RTOL[mech]
    d_res, d_th = _run_device(chem, mech, name, V, F, K)
    assert _same((d_res, d_th), (res, th[:, :2].copy()))
    if name == "m5_vector_tol":
        one, th1 = _run(chem, mech, name, V[1:2], F[1:2], K[1:2])
        assert _same((one, th1), (type(res)(res.var[1:2], res.ierr[1:2], res.stats[1:2]), th[1:2]))


@pytest.mark.parametrize("mech", MECHS)
def test_g3_a_refusal_is_a_result(chem, mech):
    """Every set Rosenbrock_x refuses (ros_options_py.REFUSED_NAMES: IERR -1 .. -5, IPAR(4) = 9 among them) through both entries: the call
    returns 0, every cell's ierr is the code, var_out equals var_in bit for bit, stats and t_h are zero; a row behind the batch stays as it was."""
    import torch
    V, F, K = _cells(mech)
    n, nvar = V.shape
    L = chem.lib()
    mid = {"gas": 0, "aer": 1, "tot": 2}[mech]
    names = R.REFUSED_NAMES
    assert "ipar4_9" in names and R.refused_set(mech, "ipar4_9")[0][3] == 9
    for name in names:
        ipar, rpar, atol, rtol = R.refused_set(mech, name)
        code = R.REFUSED_IERR[name]
        opts = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip))
        out, ierr, stats, th = np.full((n + 1, nvar), -7.25), np.full(n + 1, 77, np.int32), np.full((n + 1, 8), 77, np.int32), np.full((n + 1, 3), -7.25)
        rc = L.mistra_chem_rosenbrock_ex(mid, n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), R.TIN, R.TOUT, *opts,
                                         out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp))
        assert rc == 0, (name, L.mistra_chem_last_error())
        assert (ierr[:n] == code).all() and out[:n].tobytes() == V.tobytes() and not stats[:n].any() and not th[:n].any(), name
        assert (out[n] == -7.25).all() and ierr[n] == 77 and (stats[n] == 77).all() and (th[n] == -7.25).all(), name
        dV, dF, dK = _T(V), _T(F), _T(K)
        d_out, d_ierr, d_stats, d_th = _T(np.full((n + 1, nvar), -7.25)), _T(np.full(n + 1, 77, np.int32)), _T(np.full((n + 1, 8), 77, np.int32)), _T(np.full((n + 1, 2), -7.25))
        rc = L.mistra_chem_rosenbrock_device(mid, n, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), R.TIN, R.TOUT, *opts, d_out.data_ptr(), d_ierr.data_ptr(),
                                             d_stats.data_ptr(), d_th.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (name, L.mistra_chem_last_error())
        torch.cuda.synchronize()
        out, ierr, stats, th = d_out.cpu().numpy(), d_ierr.cpu().numpy(), d_stats.cpu().numpy(), d_th.cpu().numpy()
        assert (ierr[:n] == code).all() and out[:n].tobytes() == V.tobytes() and not stats[:n].any() and not th[:n].any(), name
        assert (out[n] == -7.25).all() and ierr[n] == 77 and (stats[n] == 77).all() and (th[n] == -7.25).all(), name
    # through the Python surface: no exception
    res, th = chem.rosenbrock(mech, V, F, K, R.TIN, R.TOUT, *R.refused_set(mech, "ipar4_9"))
    assert (res.ierr == -2).all() and res.var.tobytes() == V.tobytes() and not res.stats.any() and not th.any()


def test_g4_calls_queued_on_one_stream_each_run_with_their_own_options(chem):
    """Device calls with different methods queued on one stream before any synchronisation — more of them than the entry keeps options blocks
    (MISTRA_ROSENBROCK_CALLS_IN_FLIGHT = 8), so the ring comes round — each equal their own synchronous result."""
    import torch
    mech = "gas"
    V, F, K = _cells(mech)
    names = ("m1", "m5_rtol_1e-5", "m3", "m4_hmax_0.5", "m5", "m4", "m1_autonomous", "m4_vector_tol", "m3_rpar1_-1", "m5_vector_tol", "m1", "m4_backward")
    want = {name: _run_device(chem, mech, name, V, F, K) for name in set(names)}
    assert not _same(want["m1"], want["m5"]) and not _same(want["m4"], want["m4_hmax_0.5"])
    dV, dF, dK = _T(V), _T(F), _T(K)
    torch.cuda.synchronize()
    queued = []
    for name in names:
        ipar, rpar, atol, rtol, tstart, tend = RM.method_set(mech, name)
        queued.append(chem.rosenbrock(mech, dV, dF, dK, tstart, tend, ipar, rpar, atol, rtol))
    torch.cuda.synchronize()
    for name, res in zip(names, queued):
        assert _same(_host(res), want[name]), name
    # two tot calls back to back: long enough kernels that the second is queued while the first runs
    mech = "tot"
    V, F, K = _cells(mech)
    want = {name: _run_device(chem, mech, name, V, F, K) for name in ("m4", "m5_rtol_1e-5")}
    queued = [_run_device(chem, mech, name, V, F, K, sync=False) for name in ("m4", "m5_rtol_1e-5")]
    torch.cuda.synchronize()
    for name, res in zip(("m4", "m5_rtol_1e-5"), queued):
        assert _same(_host(res), want[name]), name


@pytest.mark.parametrize("name", ("m1", "m2", "m3", "m4", "m5"))
def test_g5_per_cell_first_step_size(chem, name):
    """d_hstart as in mistra_chem_integrate_device_hstart, per method on gas: entries <= 0 give the call's bits; 0.5 on one cell equals that cell
    run with rpar[2] = 0.5, the other cells keep their bits."""
    mech = "gas"
    V, F, K = _cells(mech)
    if name == "m2":      # Ros3: INTEGRATE_x's own options
        ipar, rpar, atol, rtol = R.base_options(mech)
    else:
        ipar, rpar, atol, rtol = RM.method_set(mech, name)[:4]

    def run(rp, hstart=None):
        import torch
        res = chem.rosenbrock(mech, _T(V), _T(F), _T(K), R.TIN, R.TOUT, ipar, rp, atol, rtol, hstart=None if hstart is None else _T(hstart))
        torch.cuda.synchronize()
        return _host(res)

    plain = run(rpar)
    assert _same(run(rpar, np.array([0.0, -1.0, 0.0])), plain)
    rp05 = rpar.copy()
    rp05[2] = 0.5
    all05 = run(rp05)
    assert not np.array_equal(all05[0].stats[1], plain[0].stats[1]) or all05[1][1].tobytes() != plain[1][1].tobytes()
    (r, th), (rp, thp), (r5, th5) = run(rpar, np.array([0.0, 0.5, -3.0])), plain, all05
    for c, (w, wt) in enumerate(((rp, thp), (r5, th5), (rp, thp))):
        assert r.var[c].tobytes() == w.var[c].tobytes() and r.ierr[c] == w.ierr[c] and np.array_equal(r.stats[c], w.stats[c]) and th[c].tobytes() == wt[c].tobytes(), c


def test_g6_two_device_slots_give_one_devices_bits(chem):
    """init_devices([0, 0]), five tot cells, Rodas3: the batch is split over the slots, each uploads the call's options block itself."""
    mech, name = "tot", "m4"
    g = load_golden(mech)
    V, F, K = g["var_in"][:5], g["fix"][:5], g["rconst"][:5]
    one = _run(chem, mech, name, V, F, K)
    assert (one[0].ierr == 1).all()
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    assert _same(_run(chem, mech, name, V, F, K), one), "the split over two slots differs from one device"


def test_g7_batch_edges(chem):
    """gas, Rodas4: the three cells tiled to 1, 63, 64, 65 and 130 rows give, row for row, the bits of the batch of three."""
    mech, name = "gas", "m5"
    V, F, K = _cells(mech)
    (res3, th3) = _run(chem, mech, name, V, F, K)
    for n in (1, 63, 64, 65, 130):
        idx = np.arange(n) % 3
        res, th = _run(chem, mech, name, V[idx], F[idx], K[idx])
        assert res.var.tobytes() == res3.var[idx].tobytes() and np.array_equal(res.ierr, res3.ierr[idx]) and np.array_equal(res.stats, res3.stats[idx]), n
        assert th.tobytes() == th3[idx].tobytes(), n
        d_res, d_th = _run_device(chem, mech, name, V[idx], F[idx], K[idx])
        assert d_res.var.tobytes() == res.var.tobytes() and np.array_equal(d_res.stats, res.stats) and d_th.tobytes() == th[:, :2].tobytes(), n


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_g8_from_fortran(tmp_path):
    """shim/shim_driver XT: ROSENBROCK_BATCH_t with Rodas3 at RTOL 1e-5, against the compiled Rosenbrock_t."""
    mech, name = "tot", "m4_rtol_1e-5"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, F, K = _cells(mech)
    z = _fixture(mech)
    ipar, rpar, atol, rtol, tstart, tend = RM.method_set(mech, name)
    n, nvar = V.shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [tstart, tend, float(n)]]).tofile(f)
        for i in range(n):
            np.concatenate([V[i], F[i], K[i]]).tofile(f)
    subprocess.run([DRIVER, "XT", str(fin), str(fout)], check=True, timeout=300)
    raw = np.fromfile(fout, np.float64)
    out = raw[:n * (nvar + 2)].reshape(n, nvar + 2)
    tail = raw[n * (nvar + 2):].reshape(n, 9)
    assert np.array_equal(tail[:, 0].astype(np.int32), z[name + "_ierr"])
    assert np.array_equal(tail[:, 1:].astype(np.int32), z[name + "_ipar"])
    d_te, d_he = mb.th_diff(out[:, nvar], out[:, nvar + 1], z[name + "_rpar"][:, 0], z[name + "_rpar"][:, 1], tstart, tend)
    d_var = mb.var_diff(out[:, :nvar], z[name + "_var"])
    print("tot %s from Fortran: VAR %.3e, exit time %.3e, last step size %.3e" % (name, d_var, d_te, d_he))
    assert d_var <= mb.METHODS_RTOL[mech] and d_te <= mb.METHODS_TH_RTOL[mech] and d_he <= mb.METHODS_TH_RTOL[mech]
    # a refusal from Fortran: ros_ErrorMsg_t's lines on unit 6, the code per cell, VAR untouched
    ipar, rpar, atol, rtol, tstart, tend = RM.method_set(mech, "m3_rpar1_-1")
    with open(fin, "wb") as f:
        np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [tstart, tend, 1.0], V[0], F[0], K[0]]).tofile(f)
    r = subprocess.run([DRIVER, "XT", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
    assert "Forced exit from Rosenbrock_t" in r.stdout and "Hmin/Hmax/Hstart must be positive" in r.stdout
    raw = np.fromfile(fout, np.float64)
    assert raw[:nvar].tobytes() == V[0].tobytes() and raw[nvar + 2] == -3.0 and not raw[nvar + 3:].any()
