"""Bounds of the series-with-rates tests on the GPU against the compiled reference (tests/test_gpu_ros_series_rates.py), MEASURED ON THE REFERENCE SIDE
exactly as tests/ros_series_bounds.py measures its own: nothing here looks at the kernel.  The expected values are the compiled Rosenbrock_x's, called
leg by leg on its own chained state with the leg's FIX and RCONST (tests/golden/ros_series_rates_<mech>.npz); the spread is the movement of its
bit-identical restatement (tests/ros_series_rates_py.py) under the oracle's legal re-associations (oracle.set_variant over parity_bounds.VARIANTS) on
the fixture's own sets, every leg of them.  tests/test_ros_series_rates.py re-measures every figure and holds every constant to [10x, 100x] of it, with
floor parity_bounds.PARITY_FLOOR (check_constant).

Premise, held by the same test: no variant changes IERR or IPAR(11:18) in any leg of any (set, cell) of the fixture.

  measured (CPU), all five sets:  VAR, worst rel_diff (conftest), any leg                    gas 5.31e-15   aer 1.07e-6   tot 8.97e-9
                                  exit time / last accepted step size (th_diff), any leg     gas 4.78e-12   aer 6.23e-6   tot 2.59e-7"""
import numpy as np

import parity_bounds as pb
from ros_series_bounds import leg_diffs  # noqa: F401

# VAR of every leg against the fixture, rel_diff of conftest.  gas: 10x its spread lies below the project's floor
RATES_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 1.1e-5, "tot": 9.0e-8}
# exit time (as a fraction of the larger end of the leg's interval) and last accepted step size (relative) of every leg, as
# ros_options_bounds.OPTIONS_TH_RTOL is taken
RATES_TH_RTOL = {"gas": 5.0e-11, "aer": 6.3e-5, "tot": 2.6e-6}


def measure_spread(mech, names=None):
    """-> (VAR spread, Texit / Hexit spread, [(variant, set) whose IERR or counters moved in any leg]) of the chained restatement over
    parity_bounds.VARIANTS"""
    import ros_series_rates_py as SR
    names = SR.SET_NAMES if names is None else names
    base = SR.restated(mech, 0, names)
    s_var, s_th, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = SR.restated(mech, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            d_var, d_th = leg_diffs(SR.TIMES, x[0], x[3], x[4], b[0], b[3], b[4])
            s_var, s_th = max(s_var, d_var), max(s_th, d_th)
    return s_var, s_th, moved
