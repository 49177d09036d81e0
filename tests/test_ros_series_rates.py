"""A series of Rosenbrock_x calls with rate constants and FIX of the leg's own, CPU side: the fixture recorded from the compiled reference called leg by
leg with the leg's rows (tests/golden/ros_series_rates_<mech>.npz), its chained Python restatement (tests/ros_series_rates_py.py), the bounds of the GPU
tests (tests/ros_series_rates_bounds.py), the refusals the four entries make before a device is touched, and tools/box_series.py --cpu."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ros_series_rates_py as SR
from conftest import MECHS, REPO, load_golden
from oracle.oracle import Reference

GOLDEN = os.path.join(REPO, "tests", "golden")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def fixture(mech):
    return dict(np.load(os.path.join(GOLDEN, "ros_series_rates_%s.npz" % mech)))


def test_the_ramp_and_the_sets_are_the_ones_the_fixture_holds():
    """times and weights as the issue sets them; the leg rows are the blend evaluated in float64 as written, stored once per mechanism; leg 0 is the
    night row itself and the last leg the day row; at least four sets per mechanism, the first three the issue's"""
    assert SR.TIMES == (0.0, 2.5, 5.0, 7.5, 10.0) and SR.W == (0.0, 0.25, 0.5, 1.0)
    assert SR.SET_NAMES[:3] == ("ros3", "ros3_carry", "rodas4") and len(SR.SET_NAMES) >= 4
    s, per_k, per_f = SR.series_set("gas", "ros2_fix_per_leg")
    assert s.ipar[3] == 1 and per_f and not per_k
    assert SR.series_set("gas", "ros3_carry")[0].carry and not SR.series_set("gas", "ros3")[0].carry
    assert SR.series_set("tot", "rodas4")[0].ipar[3] == 5 and SR.series_set("aer", "ros3_max_steps_3")[0].ipar[2] == 3
    for mech in MECHS:
        z, g = fixture(mech), load_golden(mech)
        d = dict(np.load(os.path.join(GOLDEN, "integrate_%s_day.npz" % mech)))
        c, cd = list(SR.cells_of(g["var_in"].shape[0])), list(SR.cells_of(d["var_in"].shape[0]))
        V, LF, LK = SR.ramp(mech)
        assert V.tobytes() == g["var_in"][c].tobytes()
        assert list(z["sets"]) == list(SR.SET_NAMES) and np.array_equal(z["times"], SR.TIMES)
        assert z["leg_fix"].tobytes() == LF.tobytes() and z["leg_rconst"].tobytes() == LK.tobytes()
        for k, w in enumerate(SR.W):
            assert np.array_equal(LK[k], (1 - w) * g["rconst"][c] + w * d["rconst"][cd]) and np.array_equal(LF[k], (1 - w) * g["fix"][c] + w * d["fix"][cd])
        assert LK[0].tobytes() == g["rconst"][c].tobytes() and LK[3].tobytes() == d["rconst"][cd].tobytes()
        for k in range(3):      # every leg's rows differ from the next one's, in both arrays
            assert not np.array_equal(LK[k], LK[k + 1]) and not np.array_equal(LF[k], LF[k + 1]), (mech, k)
        for name in SR.SET_NAMES:
            assert z[name + "_var"].shape == (4, 3, SR.NVAR[mech]) and z[name + "_ipar"].shape == (4, 3, 8) and z[name + "_rpar"].shape == (4, 3, 2)
        assert os.path.getsize(os.path.join(GOLDEN, "ros_series_rates_%s.npz" % mech)) <= 400 << 10


@pytest.mark.parametrize("mech", MECHS)
def test_chained_restatement_equals_the_compiled_rosenbrock(mech):
    """Bit for bit in every leg of every set (VAR, IERR, IPAR(11:18), Texit, Hexit).  What the sets are there for holds on the fixture: every leg of the
    Max_no_steps set ends with -6 having moved the state, every leg of the others with 1; the legs' rows matter (the ramp's result differs from the
    frozen rows' in every leg behind the first, and leg 0 does not); the carried first step changes the legs behind the first and not the first."""
    z = fixture(mech)
    r = SR.restated(mech)
    for name in SR.SET_NAMES:
        var, ierr, st, te, he = r[name]
        assert np.array_equal(ierr, z[name + "_ierr"]), name
        assert np.array_equal(st, z[name + "_ipar"]), name
        assert var.tobytes() == z[name + "_var"].tobytes(), name
        assert np.array_equal(te, z[name + "_rpar"][..., 0]) and np.array_equal(he, z[name + "_rpar"][..., 1]), name
        assert (z[name + "_ierr"] == (-6 if name in SR.FAILING_SETS else 1)).all(), name
    m = "ros3_max_steps_3"
    assert (z[m + "_ipar"][..., 2] > 3).all() and (z[m + "_ipar"][..., 3] >= 1).all()
    assert all(not np.array_equal(z[m + "_var"][k], z[m + "_var"][k + 1]) for k in range(3))
    a, b = z["ros3_var"], z["ros3_carry_var"]
    assert a[0].tobytes() == b[0].tobytes() and a[-1].tobytes() != b[-1].tobytes()
    # the frozen series (tests/ros_series_py.py's chain with the night rows) shares leg 0 with the ramp and no later leg
    import ros_methods_py as RM
    import ros_series_py as RS
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    V, LF, LK = SR.ramp(mech)
    s = SR.series_set(mech, "ros3")[0]
    frozen = RS.chain(lambda y, rpar, t0, t1: RM.rosenbrock(o, diag, y, LF[0, 0], LK[0, 0], s.ipar, rpar, s.atol, s.rtol, t0, t1), V[0], s)[0]
    assert frozen[0].tobytes() == a[0, 0].tobytes() and all(frozen[k].tobytes() != a[k, 0].tobytes() for k in (1, 2, 3))


@pytest.mark.skipif(not Reference.available(), reason="compiled reference (oracle/_ref) not present")
def test_fixture_regenerates_to_the_committed_files():
    """tests/golden/make_ros_series_rates_golden.py on the compiled reference gives the committed files, byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ros_series_rates_golden", os.path.join(GOLDEN, "make_ros_series_rates_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for mech in MECHS:
        raw = mod._opt.to_bytes(mod.record(mech))
        assert raw == open(os.path.join(GOLDEN, "ros_series_rates_%s.npz" % mech), "rb").read(), mech


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_series_rates_bounds.py: no re-association of the oracle changes IERR or a counter in any leg of any (set, cell) of the fixture; the
    constants are within [10x, 100x] of the spread measured now, or are the floor."""
    import parity_bounds as pb
    import ros_series_rates_bounds as sb
    s_var, s_th, moved = sb.measure_spread(mech)
    print("%s: VAR spread %.3e, exit time / last step size spread %.3e" % (mech, s_var, s_th))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    pb.check_constant("RATES_RTOL[%s]" % mech, sb.RATES_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("RATES_TH_RTOL[%s]" % mech, sb.RATES_TH_RTOL[mech], s_th, floor=pb.PARITY_FLOOR)


def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """The two counts, then the series' own refusals through the same checking function, both user slots and an unknown mechanism: each fails with its
    own text through all four entries, with every data pointer NULL and no device initialised — never the 'no HIP device' or an unknown-symbol path."""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    ipar = np.array([0, 1, 0, 2] + [0] * 16, np.int32)
    out = np.zeros(4)      # never written: every call below is refused

    def entries(mid, nleg, times, var_series, nlr=1, nlf=1, ntol=nvar):
        tp, vs = None if times is None else _P(times), None if var_series is None else _P(var_series)
        head = (mid, 1, None, None, None, nlr, nlf, nleg, tp)
        dv = None if vs is None else C.cast(vs, C.c_void_p)
        return {
            "ex": lambda: L.mistra_chem_rosenbrock_series_rates_ex(*head, _P(tol), _P(tol), _P(rpar), _P(ipar), 0, None, vs, None, None, None),
            "device": lambda: L.mistra_chem_rosenbrock_series_rates_device(*head, _P(tol), _P(tol), _P(rpar), _P(ipar), dv, None, None, None, 0, None, None),
            "cells_ex": lambda: L.mistra_chem_rosenbrock_series_rates_cells_ex(*head, _P(tol), _P(tol), ntol, _P(rpar), _P(ipar), 0, None, vs, None, None, None),
            "cells_device": lambda: L.mistra_chem_rosenbrock_series_rates_cells_device(*head, C.cast(_P(tol), C.c_void_p), C.cast(_P(tol), C.c_void_p), ntol,
                                                                                       _P(rpar), _P(ipar), dv, None, None, None, 0, None, None),
        }

    def refused(calls, text):
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    good = np.array([0.0, 1.0, 2.0, 3.0])
    for bad in (0, 2, 4, -1):
        refused(entries(0, 3, good, out, nlr=bad), "series: rconst_legs = %d: rconst has 1 block (shared by all legs) or nleg = 3 blocks" % bad)
        refused(entries(0, 3, good, out, nlf=bad), "series: fix_legs = %d: fix has 1 block (shared by all legs) or nleg = 3 blocks" % bad)
    refused(entries(0, 3, good, out, nlr=2, nlf=2), "rconst_legs = 2")      # (rconst's goes first)
    # the series' own, unchanged, whatever the counts are
    long_times = np.arange(chem.SERIES_MAX_LEGS + 2, dtype=np.float64)
    for nlr, nlf in ((1, 1), (2, 1), (1, 2), (2, 2)):
        refused(entries(0, 0, good, out, nlr, nlf), "nleg = 0: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
        refused(entries(0, chem.SERIES_MAX_LEGS + 1, long_times, out, nlr, nlf), "nleg = 4097: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
        refused(entries(0, 2, np.array([0.0, np.nan, 2.0]), out, nlr, nlf), "times[1] is not finite")
        refused(entries(0, 2, np.array([0.0, 1.0, 1.0]), out, nlr, nlf), "times[2] repeats times[1]")
        refused(entries(0, 2, np.array([0.0, 1.0, 0.5]), out, nlr, nlf), "the times change direction at times[2]")
        refused(entries(0, 2, None, out, nlr, nlf), "null times pointer")
        refused(entries(0, 2, good, None, nlr, nlf), "null var_series pointer")
        refused(entries(9, 2, good, out, nlr, nlf), "unknown mechanism id")
        cells = {k: v for k, v in entries(0, 2, good, out, nlr, nlf, ntol=2).items() if "cells" in k}
        refused(cells, "ntol = 2: a tolerance row holds 1 or NVAR = %d entries" % nvar)
        names = chem.user_mechs()
        for i in range(2):      # both user slots: the slot's existing text
            if i < len(names):
                refused(entries(3 + i, 2, good, out, nlr, nlf), "user mechanism slot %d (%s) has no series of Rosenbrock_x calls: a user slot integrates" % (i, names[i]))
            else:
                refused(entries(3 + i, 2, good, out, nlr, nlf), "unknown mechanism id")
    assert len(chem.user_mechs()) == 2      # the library this repository builds has both
    # the Python surface passes the refusals on, without init()
    V, LF, LK = SR.ramp("gas")
    with pytest.raises(chem.MistraChemError, match="rconst_legs = 4: rconst has 1 block .* or nleg = 2 blocks"):
        chem.rosenbrock_series_rates("gas", V, LF[0], LK, [0.0, 1.0, 2.0])
    with pytest.raises(chem.MistraChemError, match="fix_legs = 4: fix has 1 block .* or nleg = 3 blocks"):
        chem.rosenbrock_series_rates("gas", V, LF, LK[:3], [0.0, 1.0, 2.0, 3.0])
    with pytest.raises(chem.MistraChemError, match="rconst: a 2-D"):
        chem.rosenbrock_series_rates("gas", V, LF, LK[0, 0], SR.TIMES)
    with pytest.raises(chem.MistraChemError, match="cell counts of var / fix / rconst differ"):
        chem.rosenbrock_series_rates("gas", V, LF[:, :2], LK, SR.TIMES)
    for times, text in (([0.0], "nleg = 0"), ([0.0, 1.0, 1.0], "repeats"), ([0.0, 2.0, 1.0], "change direction"), ([0.0, np.nan], "not finite")):
        with pytest.raises(chem.MistraChemError, match=text):
            chem.rosenbrock_series_rates("gas", V, LF[0], LK[0], times)
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_series_rates("gas", V, LF, LK, SR.TIMES, atol=np.ones((3, 5)), rtol=np.ones((3, 5)))


def test_series_rates_needs_a_device():
    """Without a GPU a well-formed call raises 'no HIP device' (there is no CPU path), through the shared-pair and the cells form, with rows of the legs'
    own and with shared ones."""
    import torch
    from mistra_amd import chem
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    V, LF, LK = SR.ramp("gas")
    for F, K in ((LF, LK), (LF[0], LK), (LF, LK[0]), (LF[0], LK[0]), (LF[:1], LK[:1])):
        with pytest.raises(chem.MistraChemError, match="no HIP device"):
            chem.rosenbrock_series_rates("gas", V, F, K, SR.TIMES)
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_series_rates("gas", V, LF, LK, SR.TIMES, atol=np.full((3, 1), 1.0e-20), rtol=np.full((3, 1), 1.0e-3))
    assert chem.get_options("gas") is None


def test_tool_box_series_on_the_cpu():
    """tools/box_series.py gas --cpu: the ramp through the CPU restatement, a few species per leg.  Nothing is asserted on the figures but that they
    are numbers and that there is one line per leg."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "box_series.py"), "gas", "--cpu", "--legs", "4"], check=True, capture_output=True,
                       text=True, timeout=300)
    assert "CPU restatement" in r.stdout
    rows = [l.split("|")[0].split() for l in r.stdout.split("\n") if l.startswith("leg ")]
    assert [int(x[1]) for x in rows] == [0, 1, 2, 3], r.stdout
    assert all(len(x) == 6 and np.isfinite([float(v) for v in x[2:]]).all() for x in rows), r.stdout
