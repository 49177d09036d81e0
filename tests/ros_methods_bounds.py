"""Bounds of the tests of mistra_chem_rosenbrock_ex on the GPU (tests/test_gpu_ros_methods.py), MEASURED ON THE REFERENCE SIDE exactly as
tests/ros_options_bounds.py measures its own: nothing here looks at the kernel.  The expected values are the compiled Rosenbrock_x's
(tests/golden/ros_methods_<mech>.npz); the spread is the movement of its bit-identical restatement (tests/ros_methods_py.py) under the oracle's legal
re-associations (oracle.set_variant over parity_bounds.VARIANTS) on the fixture's own sets.  tests/test_ros_methods.py re-measures every figure and
holds every constant to [10x, 100x] of it, with floor parity_bounds.PARITY_FLOOR (check_constant).

Premise, held by the same test: no variant changes IERR or IPAR(11:18) on any (set, cell) of the fixture.

  measured (CPU):  VAR, worst rel_diff (conftest)                        gas 6.57e-15   aer 8.29e-7   tot 1.13e-8
                   exit time / last accepted step size (th_diff)         gas 1.44e-12   aer 1.54e-3   tot 1.51e-6"""
import numpy as np

import parity_bounds as pb
from ros_options_bounds import th_diff, var_diff  # noqa: F401

# VAR against the fixture, rel_diff of conftest.  gas: 10x the spread is 6.6e-14, below the floor
METHODS_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 8.3e-6, "tot": 1.2e-7}
# exit time (as a fraction of the larger end of the interval) and last accepted step size (relative), as ros_options_bounds.OPTIONS_TH_RTOL is taken.
# The largest movements are Hexit of Rodas4 at RelTol 1e-5 (aer, tot) and of Rodas3 backward in time (gas)
METHODS_TH_RTOL = {"gas": 1.5e-11, "aer": 1.6e-2, "tot": 1.6e-5}


def measure_spread(mech, golden_set, names=None):
    """-> (VAR spread, Texit / Hexit spread, [(variant, set) whose IERR or counters moved]) of the restatement over parity_bounds.VARIANTS"""
    import ros_methods_py as RM
    names = RM.SET_NAMES if names is None else names
    base = RM.restated(mech, golden_set, 0, names)
    s_var, s_th, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = RM.restated(mech, golden_set, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            tstart, tend = RM.method_set(mech, name)[4:]
            s_var = max(s_var, var_diff(x[0], b[0]))
            s_th = max(s_th, *th_diff(x[3], x[4], b[3], b[4], tstart, tend))
    return s_var, s_th, moved
