"""Bounds of the series tests on the GPU against the compiled reference (tests/test_gpu_ros_series.py), MEASURED ON THE REFERENCE SIDE exactly as
tests/ros_methods_bounds.py measures its own: nothing here looks at the kernel.  The expected values are the compiled Rosenbrock_x's, called leg by
leg on its own chained state (tests/golden/ros_series_<mech>.npz); the spread is the movement of its bit-identical restatement (tests/ros_series_py.py)
under the oracle's legal re-associations (oracle.set_variant over parity_bounds.VARIANTS) on the fixture's own chained sets, every leg of them: a
difference made in leg k travels through the legs behind it, and so does the restatement's.  tests/test_ros_series.py re-measures every figure and
holds every constant to [10x, 100x] of it, with floor parity_bounds.PARITY_FLOOR (check_constant).

Premise, held by the same test: no variant changes IERR or IPAR(11:18) in any leg of any (set, cell) of the fixture.

  measured (CPU):  VAR, worst rel_diff (conftest), any leg                    gas 2.55e-7   aer 1.35e-6   tot 3.17e-8
                   exit time / last accepted step size (th_diff), any leg     gas 1.13e-6   aer 1.37e-5   tot 1.99e-6"""
import numpy as np

import parity_bounds as pb
from ros_options_bounds import th_diff, var_diff  # noqa: F401

# VAR of every leg against the fixture, rel_diff of conftest.  gas moves most on the descending grid: backward in time the chemistry is unstable
# (one of its cells takes 559 steps through the second leg), and a rounding made early is amplified all the way
SERIES_RTOL = {"gas": 2.6e-6, "aer": 1.4e-5, "tot": 3.2e-7}
# exit time (as a fraction of the larger end of the leg's interval) and last accepted step size (relative) of every leg, as
# ros_options_bounds.OPTIONS_TH_RTOL is taken
SERIES_TH_RTOL = {"gas": 1.2e-5, "aer": 1.4e-4, "tot": 2.0e-5}


def leg_diffs(times, var, texit, hexit, want_var, want_texit, want_hexit):
    """-> (worst VAR rel_diff, worst exit time / last step size difference) over the legs of one set; arrays [nleg, ncell, ...]"""
    d_var, d_th = 0.0, 0.0
    for k in range(len(times) - 1):
        d_var = max(d_var, var_diff(var[k], want_var[k]))
        d_th = max(d_th, *th_diff(texit[k], hexit[k], want_texit[k], want_hexit[k], float(times[k]), float(times[k + 1])))
    return d_var, d_th


def measure_spread(mech, golden_set, names=None):
    """-> (VAR spread, Texit / Hexit spread, [(variant, set) whose IERR or counters moved in any leg]) of the chained restatement over
    parity_bounds.VARIANTS"""
    import ros_series_py as RS
    names = RS.SET_NAMES if names is None else names
    base = RS.restated(mech, golden_set, 0, names)
    s_var, s_th, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = RS.restated(mech, golden_set, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            d_var, d_th = leg_diffs(RS.series_set(mech, name).times, x[0], x[3], x[4], b[0], b[3], b[4])
            s_var, s_th = max(s_var, d_var), max(s_th, d_th)
    return s_var, s_th, moved
