"""Bounds of the tests of Rosenbrock_x's options on the GPU (tests/test_gpu_ros_options.py), MEASURED ON THE REFERENCE SIDE in the manner of
tests/parity_bounds.py: nothing here looks at the kernel.  The expected values are the compiled Rosenbrock_x's (tests/golden/ros_options_<mech>.npz);
the spread is the movement of its bit-identical restatement (tests/ros_options_py.py) under the oracle's legal re-associations
(oracle.set_variant over parity_bounds.VARIANTS) on the same inputs: the nine option sets that run and the scalar zero-tolerance set, cells 0, n/2,
n-1 of integrate_<mech>.npz, 0 -> 10 s.  tests/test_ros_options.py re-measures every figure and holds every constant to [10x, 100x] of it, with
floor parity_bounds.PARITY_FLOOR (check_constant).

Premise, held by the same test: no variant changes IERR or IPAR(11:18) on any (set, cell) — a kernel that differs from the reference by
re-association must then reproduce them exactly.

  measured (CPU):  VAR, worst rel_diff (conftest)          gas 1.82e-16   aer 1.74e-6   tot 3.67e-8
                   last accepted step size Hexit, relative  gas 9.22e-14   aer 8.86e-5   tot 1.38e-6
                   exit time Texit, of the interval's end   gas 0          aer 1.4e-23   tot 0        (the IERR -6 cells of aer; else identical)"""
import numpy as np

import parity_bounds as pb

# VAR against the fixture, rel_diff of conftest.  gas: 10x the spread is 1.8e-15, below the floor
OPTIONS_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 1.8e-5, "tot": 3.7e-7}
# exit time (as a fraction of the larger end of the interval) and last accepted step size (relative), as parity_bounds.REJECT_TH_RTOL is taken
OPTIONS_TH_RTOL = {"gas": 9.3e-13, "aer": 8.9e-4, "tot": 1.4e-5}


def var_diff(got, want):
    from conftest import rel_diff
    return float(rel_diff(got, want).max())


def th_diff(texit, hexit, want_texit, want_hexit, tin=0.0, tout=10.0):
    """-> (exit time difference on the scale of the interval's ends, relative difference of the last accepted step size); cells that accepted no
    step (Hexit 0 on both sides) count 0"""
    d_te = float(np.abs(np.asarray(texit) - want_texit).max() / max(abs(tin), abs(tout)))
    w = np.asarray(want_hexit, np.float64)
    d = np.abs(np.asarray(hexit) - w)
    d_he = float(np.where(w != 0.0, d / np.where(w != 0.0, np.abs(w), 1.0), d).max())
    return d_te, d_he


def measure_spread(mech, golden_set):
    """-> (VAR spread, Texit / Hexit spread, [(variant, set) whose IERR or counters moved]) of the restatement over parity_bounds.VARIANTS"""
    import ros_options_py as R
    base = R.restated(mech, golden_set)
    s_var, s_th, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = R.restated(mech, golden_set, v)
        for name in base:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            s_var = max(s_var, var_diff(x[0], b[0]))
            s_th = max(s_th, *th_diff(x[3], x[4], b[3], b[4]))
    return s_var, s_th, moved
