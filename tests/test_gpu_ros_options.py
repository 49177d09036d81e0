"""Rosenbrock_x's options on the GPU (-m gpu): mistra_chem_set_options puts IPAR, RPAR, AbsTol, RelTol in force for every integrate path of a
mechanism, in a kernel instantiation of its own.  Expected values: the compiled reference's Rosenbrock_x on the same option sets and cells
(tests/golden/ros_options_<mech>.npz); bounds: tests/ros_options_bounds.py, measured on the reference side (tests/test_ros_options.py).  Three
cells per launch: cells 0, n/2, n-1 of integrate_<mech>.npz, 0 -> 10 s."""
import os
import subprocess

import numpy as np
import pytest

import ros_options_bounds as ob
import ros_options_py as R
from conftest import MECHS, REPO, load_golden

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


def _cells(mech):
    g = load_golden(mech)
    c = list(R.cells_of(g["var_in"].shape[0]))
    return g["var_in"][c], g["fix"][c], g["rconst"][c]


def _fixture(mech):
    return dict(np.load(os.path.join(REPO, "tests", "golden", "ros_options_%s.npz" % mech)))


def _same(a, b):
    (ra, ta), (rb, tb) = a, b
    return np.array_equal(ra.var, rb.var) and np.array_equal(ra.ierr, rb.ierr) and np.array_equal(ra.stats, rb.stats) and np.array_equal(ta, tb)


def _device_call(chem, mech, V, F, K):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    n = V.shape[0]
    out, ierr, stats = torch.empty((n, V.shape[1]), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 8), dtype=torch.int32, device=dev)
    th = torch.empty((n, 2), dtype=torch.float64, device=dev)
    chem.integrate_into(mech, T(V), T(F), T(K), out, ierr, stats, R.TIN, R.TOUT, texit_hexit=th)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ierr.cpu().numpy(), stats.cpu().numpy(), th.cpu().numpy()


@pytest.mark.parametrize("mech", MECHS)
def test_g1_base_values_through_the_options_kernel_are_bit_identical(chem, mech):
    """INTEGRATE_x's own values handed to set_options run the options instantiation: var, ierr, stats, t_h equal the product kernel's bit for bit,
    and clear_options brings the product path back."""
    V, F, K = _cells(mech)
    product = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    chem.set_options(mech, *R.base_options(mech))
    assert chem.get_options(mech) is not None
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), product), "the options kernel at INTEGRATE_x's values differs from the product kernel"
    chem.clear_options(mech)
    assert chem.get_options(mech) is None
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), product)


@pytest.mark.parametrize("name", R.SET_NAMES + R.ACCEPTED_EXTRA)
@pytest.mark.parametrize("mech", MECHS)
def test_g2_option_sets_against_the_compiled_rosenbrock(chem, mech, name):
    """Per set: IERR and /Statistics/ identical to Rosenbrock_x's, VAR within OPTIONS_RTOL, exit time and last accepted step size within
    OPTIONS_TH_RTOL; the device-buffer entry gives the host-buffer entry's bits; one set also alone (ncell = 1)."""
    V, F, K = _cells(mech)
    z = _fixture(mech)
    chem.set_options(mech, *R.any_set(mech, name))
    res, th = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    d_var = ob.var_diff(res.var, z[name + "_var"])
    d_te, d_he = ob.th_diff(th[:, 0], th[:, 1], z[name + "_rpar"][:, 0], z[name + "_rpar"][:, 1])
    print("%s %s: VAR %.3e (bound %.1e), exit time %.3e, last step size %.3e (bound %.1e), Nstp %s, IERR %s" %
          (mech, name, d_var, ob.OPTIONS_RTOL[mech], d_te, d_he, ob.OPTIONS_TH_RTOL[mech], res.stats[:, 2].tolist(), res.ierr.tolist()))
    assert np.array_equal(res.ierr, z[name + "_ierr"]), (res.ierr, z[name + "_ierr"])
    assert np.array_equal(res.stats, z[name + "_ipar"]), (res.stats, z[name + "_ipar"])
    assert d_var <= ob.OPTIONS_RTOL[mech]
    assert d_te <= ob.OPTIONS_TH_RTOL[mech] and d_he <= ob.OPTIONS_TH_RTOL[mech]
    d_out, d_ierr, d_stats, d_th = _device_call(chem, mech, V, F, K)
    assert np.array_equal(d_out, res.var) and np.array_equal(d_ierr, res.ierr) and np.array_equal(d_stats, res.stats) and np.array_equal(d_th, th[:, :2])
    if name == "vector_tol":
        one, th1 = chem.integrate_ex(mech, V[1:2], F[1:2], K[1:2], R.TIN, R.TOUT)
        assert np.array_equal(one.var, res.var[1:2]) and np.array_equal(one.stats, res.stats[1:2]) and np.array_equal(th1, th[1:2])


@pytest.mark.parametrize("mech", MECHS)
def test_g3_refusals_round_trip_and_the_diagnostic_kernels(chem, mech):
    """A refused set leaves the previous options in force; get_options reads back what was set; a valid method that is not built is the library's
    error; the first-step dump, which keeps INTEGRATE_x's values, is refused while options are set."""
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = R.option_set(mech, "vector_tol")
    rpar[3:7] = (0.5, 2.0, 0.25, 0.8)
    chem.set_options(mech, ipar, rpar, atol, rtol)
    want = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    for name in R.REFUSED_NAMES:
        with pytest.raises(chem.MistraChemError, match="IERR = %d" % R.REFUSED_IERR[name]):
            chem.set_options(mech, *R.refused_set(mech, name))
    for method in (0, 1, 3, 4, 5):
        bad = ipar.copy()
        bad[3] = method
        with pytest.raises(chem.MistraChemError, match="Ros3"):
            chem.set_options(mech, bad, rpar, atol, rtol)
    got = chem.get_options(mech)
    assert np.array_equal(got.ipar, ipar) and np.array_equal(got.rpar, rpar) and np.array_equal(got.atol, atol) and np.array_equal(got.rtol, rtol)
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), want), "a refused set changed the options in force"
    with pytest.raises(chem.MistraChemError, match="INTEGRATE_x's values"):
        chem.debug_first_step(mech, V, F, K)
    # scalar tolerances come back as the integrator uses them: entry 1 for every species
    chem.set_options(mech, *R.refused_set(mech, "atol51_0_scalar"))
    assert (chem.get_options(mech).atol == 1.0e-25).all()
    # IPAR(3) goes before the debug hook, the hook still holds without it.  Max_no_steps is looked at once per accepted step (gas.f:1204), so a
    # first step with many rejected attempts overshoots it: what the hook must give is Rosenbrock_x's result at IPAR(3) = 4 (the restatement's;
    # aer's and tot's first step alone takes more attempts than either limit, gas tells 4 from 5)
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    ipar4, rpar0, atol0, rtol0 = R.base_options(mech)
    ipar4[2] = 4
    at4 = [R.rosenbrock(o, diag, V[i], F[i], K[i], ipar4, rpar0, atol0, rtol0) for i in range(len(V))]
    assert all(x[1] == -6 and x[2][2] > 4 for x in at4)
    chem.debug_set_max_steps(4)
    try:
        chem.set_options(mech, *R.option_set(mech, "max_steps_5"))
        assert np.array_equal(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)[0].stats, _fixture(mech)["max_steps_5_ipar"])
        chem.set_options(mech, *R.base_options(mech))
        r = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)[0]
        assert (r.ierr == -6).all() and np.array_equal(r.stats, np.array([x[2] for x in at4])), r.stats
    finally:
        chem.debug_set_max_steps(0)
    chem.clear_options(mech)
    chem.debug_first_step(mech, V, F, K)


def test_g4_two_device_slots_give_one_devices_bits(chem):
    """init_devices([0, 0]), five tot cells, vector tolerances: the block every slot reads is uploaded to every slot."""
    mech = "tot"
    g = load_golden(mech)
    V, F, K = g["var_in"][:5], g["fix"][:5], g["rconst"][:5]
    opts = R.option_set(mech, "vector_tol")
    chem.set_options(mech, *opts)
    one = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    plain = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT)
    assert not np.array_equal(plain[0].stats, one[0].stats)      # finalize dropped the options: INTEGRATE_x's values
    chem.set_options(mech, *opts)
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), one), "the split over two slots differs from one device"
    chem.init_devices([0])                                       # a re-initialisation keeps them
    assert chem.device_count() == 1
    assert _same(chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT), one)


def test_g5_column_driver_honours_the_options(chem):
    """mistra_chem_drive on the captured Joyce2014 column step (148 gas layers): with Hmax = 0.5 s every layer takes at least 10 / 0.5 = 20 steps;
    without options the captured /Statistics/ come back."""
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "drivecol_Joyce2014.npz")))
    mech = "gas"
    assert (g["mech"] == 0).all() and len(g["k"]) == 148
    chem.set_species_maps(mech, g[mech + "_gas_m2k"], g[mech + "_gas_k2m"], g[mech + "_rad_m2k"], g[mech + "_rad_k2m"])
    n = 150

    def step():
        a = {}
        for key in ("s1", "s3", "sl1", "sion1"):
            a[key] = np.full((n, g[key + "_in"].shape[1]), -7.25)
            a[key][g["k"] - 1] = g[key + "_in"]
        ierr, stats, th = chem.drive_host(mech, g["k"], a["s1"], a["s3"], a["sl1"], a["sion1"], g["scal"], g["env"][:, :74].copy(), 0.0, 10.0)
        return ierr, stats

    ierr, stats = step()
    assert (ierr == 1).all() and np.array_equal(stats, g["stats"])
    assert (stats[:, 2] < 20).any()
    chem.set_options(mech, *R.option_set(mech, "hmax_0.5"))
    ierr, stats = step()
    assert (ierr == 1).all() and (stats[:, 2] >= 20).all(), stats[:, 2].min()
    chem.clear_options(mech)
    ierr, stats = step()
    assert np.array_equal(stats, g["stats"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_g6_from_fortran(tmp_path):
    """shim/shim_driver OT: MISTRA_SET_OPTIONS_t with RTOL 1e-5, then the batched call INTEGRATE_BATCH_t, against the compiled Rosenbrock_t."""
    mech, name = "tot", "rtol_1e-5"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, F, K = _cells(mech)
    z = _fixture(mech)
    ipar, rpar, atol, rtol = R.option_set(mech, name)
    n, nvar = V.shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [float(n)]]).tofile(f)
        for i in range(n):
            np.concatenate([V[i], F[i], K[i]]).tofile(f)
    subprocess.run([DRIVER, "OT", str(fin), str(fout)], check=True, timeout=300)
    raw = np.fromfile(fout, np.float64)
    out = raw[:n * (nvar + 4)].reshape(n, nvar + 4)
    tail = raw[n * (nvar + 4):n * (nvar + 4) + 9 * n].reshape(n, 9)
    assert raw[-1] == 1.0, "IERR of MISTRA_SET_OPTIONS_t"
    assert np.array_equal(tail[:, 0].astype(np.int32), z[name + "_ierr"])
    assert np.array_equal(tail[:, 1:].astype(np.int32), z[name + "_ipar"])
    d_te, d_he = ob.th_diff(out[:, nvar], out[:, nvar + 1], z[name + "_rpar"][:, 0], z[name + "_rpar"][:, 1])
    d_var = ob.var_diff(out[:, :nvar], z[name + "_var"])
    print("tot %s from Fortran: VAR %.3e, exit time %.3e, last step size %.3e" % (name, d_var, d_te, d_he))
    assert d_var <= ob.OPTIONS_RTOL[mech] and d_te <= ob.OPTIONS_TH_RTOL[mech] and d_he <= ob.OPTIONS_TH_RTOL[mech]
    # a refusal from Fortran: Rosenbrock_t's lines on unit 6, IERR handed back, the run goes on at INTEGRATE_t's values
    ipar, rpar, atol, rtol = R.refused_set(mech, "rpar1_-1")
    with open(fin, "wb") as f:
        np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [1.0], V[0], F[0], K[0]]).tofile(f)
    r = subprocess.run([DRIVER, "OT", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
    assert "Forced exit from Rosenbrock_t" in r.stdout and "Hmin/Hmax/Hstart must be positive" in r.stdout
    raw = np.fromfile(fout, np.float64)
    assert raw[-1] == -3.0
    assert np.array_equal(raw[nvar + 4 + 1:nvar + 4 + 9].astype(np.int32), load_golden(mech)["stats"][0])
