"""Rosenbrock_x's options, CPU side: the fixture recorded from the compiled reference (tests/golden/ros_options_<mech>.npz), its Python restatement
(tests/ros_options_py.py), the library's host decode (mistra_chem_check_options) and the bounds of the GPU tests (tests/ros_options_bounds.py)."""
import os

import numpy as np
import pytest

import ros_options_py as R
from conftest import MECHS, REPO, load_golden
from oracle.oracle import Reference

GOLDEN = os.path.join(REPO, "tests", "golden")


def fixture(mech):
    return dict(np.load(os.path.join(GOLDEN, "ros_options_%s.npz" % mech)))


@pytest.mark.parametrize("mech", MECHS)
def test_restatement_equals_the_compiled_rosenbrock(mech):
    """Bit for bit on every option set that runs (VAR, IERR, IPAR(11:18), Texit, Hexit), and on the refused ones: the code, Y untouched, zero counters.
    At INTEGRATE_x's options the restatement is Oracle.integrate."""
    g, z = load_golden(mech), fixture(mech)
    cells = list(R.cells_of(g["var_in"].shape[0]))
    assert np.array_equal(z["cells"], cells)
    r = R.restated(mech, g)
    for name in R.SET_NAMES + R.ACCEPTED_EXTRA:
        var, ierr, st, te, he = r[name]
        assert np.array_equal(ierr, z[name + "_ierr"]), name
        assert np.array_equal(st, z[name + "_ipar"]), name
        assert np.array_equal(var, z[name + "_var"]), name
        assert np.array_equal(te, z[name + "_rpar"][:, 0]) and np.array_equal(he, z[name + "_rpar"][:, 1]), name
    assert (z["max_steps_5_ierr"] == -6).all() and (z["hmin_0.05_ierr"] == 1).all()
    assert (z["autonomous_ipar"][:, 0] < z["atol51_0_scalar_ipar"][:, 0]).all()      # one Fun count per step less; the scalar zero set IS the base set
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    for name in R.REFUSED_NAMES:
        assert (z[name + "_ierr"] == R.REFUSED_IERR[name]).all(), name
        assert np.array_equal(z[name + "_var"], g["var_in"][cells]) and not z[name + "_ipar"].any() and not z[name + "_rpar"].any(), name
        c = cells[1]
        var, ierr, st, te, he = R.rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *R.refused_set(mech, name))
        assert ierr == R.REFUSED_IERR[name] and np.array_equal(var, g["var_in"][c]) and not st.any() and te == 0.0 and he == 0.0, name
    c = cells[0]
    want = o.integrate(g["var_in"][c], g["fix"][c], g["rconst"][c], R.TIN, R.TOUT)
    got = R.rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *R.base_options(mech))
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]) and got[3:] == want[3:]


@pytest.mark.skipif(not Reference.available(), reason="compiled reference (oracle/_ref) not present")
def test_fixture_regenerates_to_the_committed_arrays():
    """tests/golden/make_ros_options_golden.py on the compiled reference gives the committed arrays, byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ros_options_golden", os.path.join(GOLDEN, "make_ros_options_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for mech in MECHS:
        new, old = mod.record(mech), fixture(mech)
        assert sorted(new) == sorted(old)
        for k in new:
            a, b = np.asarray(new[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (mech, k)


@pytest.mark.parametrize("mech", MECHS)
def test_check_options_decodes_as_rosenbrock_does(mech):
    """mistra_chem_check_options (no GPU): IERR as the compiled reference returned it for every set, the resolved values as the restatement's decode
    hands them to the integrator, at the fixture's interval and at one shorter than Hmax and Hstart."""
    from mistra_amd import chem
    z = fixture(mech)
    for name in R.SET_NAMES + R.ACCEPTED_EXTRA + R.REFUSED_NAMES:
        ipar, rpar, atol, rtol = R.any_set(mech, name)
        want_ierr = R.REFUSED_IERR.get(name, 1)
        if name in R.REFUSED_NAMES:
            assert (z[name + "_ierr"] == want_ierr).all(), name
        for tend in (R.TOUT, 0.25):
            got = chem.check_options(mech, ipar, rpar, atol, rtol, interval=tend - R.TIN)
            ierr, p = R.resolve(ipar, rpar, atol, rtol, R.NVAR[mech], R.TIN, tend)
            assert got.ierr == ierr == want_ierr, (name, got.ierr, ierr)
            if ierr == 1:
                assert (got.hmin, got.hmax, got.hstart, got.facmin, got.facmax, got.facrej, got.facsafe) == \
                    (p["hmin"], p["hmax"], p["hstart"], p["facmin"], p["facmax"], p["facrej"], p["facsafe"]), name
                assert (got.max_steps, got.autonomous, got.vector) == (p["max_steps"], p["autonomous"], p["vector"]), name
    # the four valid methods that are not built: the library's own error, not a code of Rosenbrock_x's
    for method in (0, 1, 3, 4, 5):
        ipar, rpar, atol, rtol = R.base_options(mech)
        ipar[3] = method
        assert R.resolve(ipar, rpar, atol, rtol, R.NVAR[mech], R.TIN, R.TOUT)[0] == 1
        with pytest.raises(chem.MistraChemError, match="Ros3"):
            chem.check_options(mech, ipar, rpar, atol, rtol)
    # the first refusal in Rosenbrock_x's order wins
    ipar, rpar, atol, rtol = R.base_options(mech)
    ipar[3], rpar[0] = 0, -1.0
    assert chem.check_options(mech, ipar, rpar, atol, rtol).ierr == -3
    with pytest.raises(chem.MistraChemError):
        chem.check_options(mech, atol=np.ones(3))


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_options_bounds.py: no re-association of the oracle changes IERR or the counters on any (set, cell); the constants are within
    [10x, 100x] of the spread measured now, or are the floor.  Measured: VAR gas 1.82e-16, aer 1.74e-6, tot 3.67e-8; Texit / Hexit gas 9.22e-14,
    aer 8.86e-5, tot 1.38e-6."""
    import parity_bounds as pb
    import ros_options_bounds as ob
    s_var, s_th, moved = ob.measure_spread(mech, load_golden(mech))
    print("%s: VAR spread %.3e, exit time / last step size spread %.3e" % (mech, s_var, s_th))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    pb.check_constant("OPTIONS_RTOL[%s]" % mech, ob.OPTIONS_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("OPTIONS_TH_RTOL[%s]" % mech, ob.OPTIONS_TH_RTOL[mech], s_th, floor=pb.PARITY_FLOOR)


def test_set_options_needs_a_device_and_get_options_does_not():
    """Without a GPU: the decode and the read-back work, putting options in force does not (there is no CPU path to use them)."""
    import torch
    from mistra_amd import chem
    assert chem.get_options("gas") is None or torch.cuda.is_available()
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.set_options("gas", *R.base_options("gas"))
    assert chem.get_options("gas") is None
