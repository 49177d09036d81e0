"""A series of Rosenbrock_x calls, CPU side: the fixture recorded from the compiled reference called leg by leg (tests/golden/ros_series_<mech>.npz), its
chained Python restatement (tests/ros_series_py.py), the bounds of the GPU tests (tests/ros_series_bounds.py), the refusals the series entries make
before a device is touched, and tools/step_control.py --series on the CPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ros_series_py as RS
from conftest import MECHS, REPO, load_golden
from oracle.oracle import Reference

GOLDEN = os.path.join(REPO, "tests", "golden")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def fixture(mech):
    return dict(np.load(os.path.join(GOLDEN, "ros_series_%s.npz" % mech)))


def test_the_sets_are_the_ones_the_fixture_needs():
    assert len(RS.series_set("gas", "ros3_8").times) == 9 and np.array_equal(np.diff(RS.series_set("gas", "ros3_8").times), np.full(8, 1.25))
    assert RS.series_set("gas", "ros3_unequal_carry").carry and not RS.series_set("gas", "ros3_unequal").carry
    assert np.array_equal(RS.series_set("gas", "ros3_unequal").times, RS.series_set("gas", "ros3_unequal_carry").times)
    assert RS.series_set("tot", "rodas4_rtol_1e-7").ipar[3] == 5 and len(RS.series_set("tot", "rodas4_rtol_1e-7").times) == 5
    assert RS.series_set("aer", "ros2_vector_tol").ipar[1] == 0 and RS.series_set("aer", "ros2_vector_tol").ipar[3] == 1
    assert np.all(np.diff(RS.series_set("gas", "ros3_descending").times) < 0)
    for mech in MECHS:
        z = fixture(mech)
        assert list(z["sets"]) == list(RS.SET_NAMES)
        for name in RS.SET_NAMES:
            assert np.array_equal(z[name + "_times"], RS.series_set(mech, name).times), name
            nleg = len(z[name + "_times"]) - 1
            assert z[name + "_var"].shape == (nleg, 3, RS.NVAR[mech]) and z[name + "_ipar"].shape == (nleg, 3, 8)
        assert os.path.getsize(os.path.join(GOLDEN, "ros_series_%s.npz" % mech)) <= 400 << 10


@pytest.mark.parametrize("mech", MECHS)
def test_chained_restatement_equals_the_compiled_rosenbrock(mech):
    """Bit for bit in every leg of every set (VAR, IERR, IPAR(11:18), Texit, Hexit).  What the sets are there for holds on the fixture: every leg of the
    Max_no_steps set ends with -6 having moved the state, every leg of the ascending others with 1; the carried first step changes the legs behind the
    first and not the first; no step of the 1e-6 s leg is longer than the leg, and the leg of 1e-4 s is one step."""
    g, z = load_golden(mech), fixture(mech)
    cells = list(RS.cells_of(g["var_in"].shape[0]))
    assert np.array_equal(z["cells"], cells)
    r = RS.restated(mech, g)
    for name in RS.SET_NAMES:
        var, ierr, st, te, he = r[name]
        assert np.array_equal(ierr, z[name + "_ierr"]), name
        assert np.array_equal(st, z[name + "_ipar"]), name
        assert var.tobytes() == z[name + "_var"].tobytes(), name
        assert np.array_equal(te, z[name + "_rpar"][..., 0]) and np.array_equal(he, z[name + "_rpar"][..., 1]), name
        if name != "ros3_descending":      # (backward in time the chemistry is unstable: most of its legs end with -7, as the reference has them)
            assert (z[name + "_ierr"] == (-6 if name in RS.FAILING_SETS else 1)).all(), name
    m = "ros3_max_steps_3"
    assert (z[m + "_ipar"][..., 2] > 3).all() and (z[m + "_ipar"][..., 3] >= 1).all()      # Nstp past Max_no_steps in every leg, steps accepted on the way
    assert not np.array_equal(z[m + "_var"][0], z[m + "_var"][1]) and not np.array_equal(z[m + "_var"][1], z[m + "_var"][2])
    assert (np.abs(z[m + "_rpar"][..., 0] - z[m + "_times"][:-1, None]) < np.diff(z[m + "_times"])[:, None]).all()      # Texit inside its own leg
    a, b = z["ros3_unequal_var"], z["ros3_unequal_carry_var"]
    assert a[0].tobytes() == b[0].tobytes() and a[-1].tobytes() != b[-1].tobytes()
    assert (z["ros3_unequal_rpar"][0, :, 1] <= 1.0e-6).all()        # the first step clipped to the leg: no step of leg 0 is longer than the leg
    assert (z["ros3_unequal_ipar"][2, :, 2] == 1).all()             # 0.5 -> 0.5001: a one-step leg
    assert (z["ros3_unequal_ipar"][4, :, 2] > 1).all()              # ... and the long leg behind a short one


@pytest.mark.skipif(not Reference.available(), reason="compiled reference (oracle/_ref) not present")
def test_fixture_regenerates_to_the_committed_files():
    """tests/golden/make_ros_series_golden.py on the compiled reference gives the committed files, byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ros_series_golden", os.path.join(GOLDEN, "make_ros_series_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for mech in MECHS:
        raw = mod._opt.to_bytes(mod.record(mech))
        assert raw == open(os.path.join(GOLDEN, "ros_series_%s.npz" % mech), "rb").read(), mech


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_series_bounds.py: no re-association of the oracle changes IERR or a counter in any leg of any (set, cell) of the fixture; the constants
    are within [10x, 100x] of the spread measured now, or are the floor."""
    import parity_bounds as pb
    import ros_series_bounds as sb
    s_var, s_th, moved = sb.measure_spread(mech, load_golden(mech))
    print("%s: VAR spread %.3e, exit time / last step size spread %.3e" % (mech, s_var, s_th))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    pb.check_constant("SERIES_RTOL[%s]" % mech, sb.SERIES_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("SERIES_TH_RTOL[%s]" % mech, sb.SERIES_TH_RTOL[mech], s_th, floor=pb.PARITY_FLOOR)


def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """nleg, the times, NULL times / var_series, ntol, both user slots and an unknown mechanism: each fails with its own text through all four series
    entries, with every data pointer NULL and no device initialised — never the 'no HIP device' or an unknown-symbol path."""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    ipar = np.array([0, 1, 0, 2] + [0] * 16, np.int32)
    vector = np.array([0, 0, 0, 2] + [0] * 16, np.int32)
    out = np.zeros(4)      # never written: every call below is refused

    def entries(mid, nleg, times, var_series, ntol=nvar, ip=ipar, at=tol):
        tp, vs = None if times is None else _P(times), None if var_series is None else _P(var_series)
        head = (mid, 1, None, None, None, nleg, tp)
        return {
            "series_ex": lambda: L.mistra_chem_rosenbrock_series_ex(*head, _P(at), _P(tol), _P(rpar), _P(ip), 0, None, vs, None, None, None),
            "series_device": lambda: L.mistra_chem_rosenbrock_series_device(*head, _P(at), _P(tol), _P(rpar), _P(ip),
                                                                            None if vs is None else C.cast(vs, C.c_void_p), None, None, None, 0, None, None),
            "series_cells_ex": lambda: L.mistra_chem_rosenbrock_series_cells_ex(*head, _P(at), _P(tol), ntol, _P(rpar), _P(ip), 0, None, vs, None, None, None),
            "series_cells_device": lambda: L.mistra_chem_rosenbrock_series_cells_device(*head, C.cast(_P(at), C.c_void_p), C.cast(_P(tol), C.c_void_p), ntol,
                                                                                        _P(rpar), _P(ip), None if vs is None else C.cast(vs, C.c_void_p), None,
                                                                                        None, None, 0, None, None),
        }

    def refused(calls, text):
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    assert chem.SERIES_MAX_LEGS == 4096
    good = np.array([0.0, 1.0, 2.0])
    long_times = np.arange(chem.SERIES_MAX_LEGS + 2, dtype=np.float64)
    refused(entries(0, 0, good, out), "nleg = 0: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, -3, good, out), "nleg = -3: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, chem.SERIES_MAX_LEGS + 1, long_times, out), "nleg = 4097: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, 2, np.array([0.0, np.nan, 2.0]), out), "times[1] is not finite")
    refused(entries(0, 2, np.array([0.0, 1.0, np.inf]), out), "times[2] is not finite")
    refused(entries(0, 2, np.array([0.0, 1.0, 1.0]), out), "times[2] repeats times[1]")
    refused(entries(0, 2, np.array([0.0, 1.0, 0.5]), out), "the times change direction at times[2]")
    refused(entries(0, 2, np.array([3.0, 1.0, 1.5]), out), "the times change direction at times[2]")
    refused(entries(0, 2, None, out), "null times pointer")
    refused(entries(0, 2, good, None), "null var_series pointer")
    refused(entries(9, 2, good, out), "unknown mechanism id")
    cells = {k: v for k, v in entries(0, 2, good, out, ntol=2).items() if "cells" in k}
    refused(cells, "ntol = 2: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    cells = {k: v for k, v in entries(0, 2, good, out, ntol=0).items() if "cells" in k}
    refused(cells, "ntol = 0: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    cells = {k: v for k, v in entries(0, 2, good, out, ntol=1, ip=vector).items() if "cells" in k}
    refused(cells, "vector tolerances (ipar[1] = 0) need rows of NVAR = %d entries, ntol = 1" % nvar)
    # both user slots: the slot's existing text, whatever else the call carries (ids 3 and 4 of a library without slots are no mechanisms)
    names = chem.user_mechs()
    for i in range(2):
        if i < len(names):
            refused(entries(3 + i, 2, good, out), "user mechanism slot %d (%s) has no series of Rosenbrock_x calls: a user slot integrates" % (i, names[i]))
            refused(entries(3 + i, 2, good, out), "and nothing else")
        else:
            refused(entries(3 + i, 2, good, out), "unknown mechanism id")
    assert len(names) == 2      # the library this repository builds has both
    # the Python surface passes the refusals on, without init()
    g = load_golden("gas")
    V, F, K = g["var_in"][:2], g["fix"][:2], g["rconst"][:2]
    for times, text in (([0.0], "nleg = 0"), ([0.0, 1.0, 1.0], "repeats"), ([0.0, 2.0, 1.0], "change direction"), ([0.0, np.nan], "not finite")):
        with pytest.raises(chem.MistraChemError, match=text):
            chem.rosenbrock_series("gas", V, F, K, times)
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_series("gas", V, F, K, [0.0, 1.0], atol=np.ones((2, 5)), rtol=np.ones((2, 5)))


def test_series_needs_a_device():
    """Without a GPU a well-formed series raises 'no HIP device' (there is no CPU path), and nothing is in force afterwards."""
    import torch
    from mistra_amd import chem
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = load_golden("gas")
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_series("gas", g["var_in"][:1], g["fix"][:1], g["rconst"][:1], [0.0, 5.0, 10.0])
    assert chem.get_options("gas") is None


def test_tool_series_on_the_cpu():
    """step_control.py --series 4 --cpu on a golden gas cell: runs without a GPU and prints the yardstick distance at the four sub-times.  Nothing is
    asserted on the figures but that they are numbers."""
    path = os.path.join(GOLDEN, "integrate_gas.npz")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "step_control.py"), "gas", "--golden", path, "--cells", "0:1", "--cpu", "--series", "4"],
                       check=True, capture_output=True, text=True, timeout=300)
    assert "CPU restatement" in r.stdout
    at = r.stdout.index("distance from the yardstick at 4 sub-times")
    rows = [l.split() for l in r.stdout[at:].split("\n")[2:] if l.strip()]
    assert [float(x[0]) for x in rows] == [2.5, 5.0, 7.5, 10.0], r.stdout
    assert all(np.isfinite(float(x[2])) for x in rows), r.stdout
