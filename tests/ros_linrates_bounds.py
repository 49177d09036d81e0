"""Bounds of the tests of the series with rate constants linear in time on the GPU (tests/test_gpu_ros_linrates.py), MEASURED ON THE RESTATEMENT'S SIDE
as tests/ros_series_rates_bounds.py measures its own: nothing here looks at the kernel.  The expected values are tests/ros_linrates_py.py's chain (the
definition; there is no compiled reference with rate constants that move inside a call); the spread is its movement under the oracle's legal
re-associations (oracle.set_variant over parity_bounds.VARIANTS) on its own sets, every leg of them, with conftest's rel_diff and
ros_series_bounds.leg_diffs.  tests/test_ros_linrates.py re-measures every figure and holds every constant to [10x, 100x] of it, with floor
parity_bounds.PARITY_FLOOR (check_constant).

Premise, held by the same test: no variant changes IERR or IPAR(11:18) in any leg of any (set, cell).

  measured (CPU), all sets of ros_linrates_py.set_names(mech) (gas: eleven, with ros3_autonomous_flag; aer, tot: ten):
      VAR, worst rel_diff (conftest), any leg                    gas 1.14e-12   aer 8.76e-7   tot 1.90e-8
      exit time / last accepted step size (th_diff), any leg     gas 5.48e-12   aer 1.31e-4   tot 1.07e-6
  the sets that move most: gas VAR ros3_autonomous_flag (some 1800 steps in leg 0), gas exit time m3; aer VAR ros3_equal_nodes (the frozen night rows,
  as tests/ros_series_rates_bounds.py's 1.07e-6), aer and tot step size m5 (Rodas4's error estimate is its last stage alone)."""
import numpy as np

import parity_bounds as pb
from ros_series_bounds import leg_diffs  # noqa: F401

LINRATES_RTOL = {"gas": 1.2e-11, "aer": 8.8e-6, "tot": 2.0e-7}
LINRATES_TH_RTOL = {"gas": 5.5e-11, "aer": 1.4e-3, "tot": 1.1e-5}


def measure_spread(mech, names=None):
    """-> (VAR spread, Texit / Hexit spread, [(variant, set) whose IERR or counters moved in any leg]) of the chained restatement over
    parity_bounds.VARIANTS"""
    import ros_linrates_py as LR
    names = LR.set_names(mech) if names is None else names
    base = LR.restated(mech, 0, names)
    s_var, s_th, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = LR.restated(mech, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            d_var, d_th = leg_diffs(LR.series_set(mech, name)[0].times, x[0], x[3], x[4], b[0], b[3], b[4])
            s_var, s_th = max(s_var, d_var), max(s_th, d_th)
    return s_var, s_th, moved
