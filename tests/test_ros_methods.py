"""Rosenbrock_x's five methods, CPU side: the fixture recorded from the compiled reference (tests/golden/ros_methods_<mech>.npz), its Python
restatement (tests/ros_methods_py.py), the method tables the kernels are compiled with (mistra_chem_method_table) and the bounds of the GPU tests
(tests/ros_methods_bounds.py)."""
import os

import numpy as np
import pytest

import ros_methods_py as RM
import ros_options_py as R
from conftest import MECHS, REPO, load_golden
from oracle.oracle import Reference

GOLDEN = os.path.join(REPO, "tests", "golden")


def fixture(mech):
    return dict(np.load(os.path.join(GOLDEN, "ros_methods_%s.npz" % mech)))


def test_the_sets_are_the_ones_the_fixture_needs():
    assert len(RM.BASE_SETS) == len(RM.AUTONOMOUS_SETS) == 5 and len(RM.OPTION_SETS) == 8
    assert [RM.method_of(n) for n in RM.BASE_SETS] == [3, 1, 3, 4, 5]
    for mech in MECHS:
        z = fixture(mech)
        assert list(z["sets"]) == list(RM.SET_NAMES)
        path = os.path.join(GOLDEN, "ros_methods_%s.npz" % mech)
        assert os.path.getsize(path) <= min(1 << 20, os.path.getsize(os.path.join(GOLDEN, "integrate_%s.npz" % mech)))


@pytest.mark.parametrize("mech", MECHS)
def test_restatement_equals_the_compiled_rosenbrock(mech):
    """Bit for bit on every set (VAR, IERR, IPAR(11:18), Texit, Hexit), the refused one included; IPAR(4) = 0 gives method 3's arrays; every method
    set at INTEGRATE_x's other options ends with IERR = 1 and the methods are told apart by their counters."""
    g, z = load_golden(mech), fixture(mech)
    cells = list(RM.cells_of(g["var_in"].shape[0]))
    assert np.array_equal(z["cells"], cells)
    r = RM.restated(mech, g)
    for name in RM.SET_NAMES:
        var, ierr, st, te, he = r[name]
        assert np.array_equal(ierr, z[name + "_ierr"]), name
        assert np.array_equal(st, z[name + "_ipar"]), name
        assert var.tobytes() == z[name + "_var"].tobytes(), name
        assert np.array_equal(te, z[name + "_rpar"][:, 0]) and np.array_equal(he, z[name + "_rpar"][:, 1]), name
    for tail in ("", "_autonomous"):
        for part in ("var", "ierr", "ipar", "rpar"):
            assert z["m0%s_%s" % (tail, part)].tobytes() == z["m3%s_%s" % (tail, part)].tobytes()
    for name in RM.BASE_SETS + RM.AUTONOMOUS_SETS:
        assert (z[name + "_ierr"] == 1).all(), name
        tb, st = RM.table(RM.method_of(name)), z[name + "_ipar"]
        assert np.array_equal(st[:, 6], tb.S * (st[:, 5] - st[:, 7])), name      # Nsol = S per decomposition that succeeded
        per_step = 1 if name.endswith("_autonomous") else 2
        assert np.array_equal(st[:, 0], per_step * st[:, 1] + (sum(tb.newf) - 1) * st[:, 2]), name          # Nfun as the reference counts
    for name in RM.REFUSED_SETS:
        assert (z[name + "_ierr"] == RM.REFUSED_IERR[name]).all()
        assert np.array_equal(z[name + "_var"], g["var_in"][cells]) and not z[name + "_ipar"].any() and not z[name + "_rpar"].any()
    assert (z["m4_max_steps_5_ierr"] == -6).all() and (z["m5_max_steps_5_ierr"] == -6).all()
    # Ros3 through the generalised restatement is ros_options_py's
    c = cells[0]
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    a = RM.rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *R.base_options(mech))
    b = R.rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *R.base_options(mech))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


@pytest.mark.skipif(not Reference.available(), reason="compiled reference (oracle/_ref) not present")
def test_fixture_regenerates_to_the_committed_files():
    """tests/golden/make_ros_methods_golden.py on the compiled reference gives the committed files, byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ros_methods_golden", os.path.join(GOLDEN, "make_ros_methods_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for mech in MECHS:
        raw = mod._opt.to_bytes(mod.record(mech))
        assert raw == open(os.path.join(GOLDEN, "ros_methods_%s.npz" % mech), "rb").read(), mech


def test_method_tables_are_the_restatements():
    """mistra_chem_method_table (no GPU): the tables the kernels are compiled with equal the restatement's bit for bit for IPAR(4) = 1 .. 5, 0 maps
    to 3, anything else fails."""
    from mistra_amd import chem
    for m in (1, 2, 3, 4, 5, 0):
        got, want = chem.method_table(m), RM.table(m)
        assert got.S == want.S and got.elo == want.elo, m
        for a, b in ((got.A, want.A), (got.C, want.C), (got.M, want.M), (got.E, want.E), (got.gamma, want.gamma)):
            assert np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes(), m
        assert list(got.newf) == list(want.newf), m
    zero, three = chem.method_table(0), chem.method_table(3)
    assert all(np.array_equal(a, b) for a, b in zip(zero[1:7], three[1:7])) and zero.S == three.S == 4
    for bad in (-1, 6, 9):
        with pytest.raises(chem.MistraChemError, match="methods 1 .. 5"):
            chem.method_table(bad)


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_methods_bounds.py: no re-association of the oracle changes IERR or the counters on any (set, cell) of the fixture; the constants are
    within [10x, 100x] of the spread measured now, or are the floor.  Measured: VAR gas 6.57e-15, aer 8.29e-7, tot 1.13e-8; Texit / Hexit gas
    1.44e-12, aer 1.54e-3, tot 1.51e-6."""
    import parity_bounds as pb
    import ros_methods_bounds as mb
    s_var, s_th, moved = mb.measure_spread(mech, load_golden(mech))
    print("%s: VAR spread %.3e, exit time / last step size spread %.3e" % (mech, s_var, s_th))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    pb.check_constant("METHODS_RTOL[%s]" % mech, mb.METHODS_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("METHODS_TH_RTOL[%s]" % mech, mb.METHODS_TH_RTOL[mech], s_th, floor=pb.PARITY_FLOOR)


def test_rosenbrock_needs_a_device_and_the_tables_do_not():
    """Without a GPU: the tables work, the entry raises (there is no CPU path); the options surface is as it was — the four methods are still
    refused by check_options, nothing is in force."""
    import torch
    from mistra_amd import chem
    assert chem.method_table(5).S == 6
    for method in (0, 1, 3, 4, 5):
        ipar, rpar, atol, rtol = R.base_options("gas")
        ipar[3] = method
        with pytest.raises(chem.MistraChemError, match="Ros3"):
            chem.check_options("gas", ipar, rpar, atol, rtol)
    assert chem.check_options("gas", *R.base_options("gas")).ierr == 1
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert chem.get_options("gas") is None
    g = load_golden("gas")
    ipar, rpar, atol, rtol = RM.method_set("gas", "m4")[:4]
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock("gas", g["var_in"][:1], g["fix"][:1], g["rconst"][:1], 0.0, 10.0, ipar, rpar, atol, rtol)
    assert chem.get_options("gas") is None
