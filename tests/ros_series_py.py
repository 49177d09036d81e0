"""TEST INFRASTRUCTURE — a series of Rosenbrock_x calls (mistra_chem_rosenbrock_series_ex) restated on the CPU: tests/ros_methods_py.py's restatement of
Rosenbrock_x called leg by leg on its own chained state, and the sets the series tests run.

Pinned as that one is: on every set below the chain equals the compiled Rosenbrock_x called the same way, bit for bit in every leg — VAR, IERR,
IPAR(11:18), Texit, Hexit (tests/test_ros_series.py, against tests/golden/ros_series_<mech>.npz, which tests/golden/make_ros_series_golden.py records
from the compiled reference).  It exists to measure, on the reference side, how far a chained result moves under legal re-association
(tests/ros_series_bounds.py)."""
from collections import namedtuple

import numpy as np

import ros_methods_py as RM
import ros_options_py as R
from ros_options_py import MECHS, NVAR, cells_of  # noqa: F401

# ipar, rpar, atol, rtol: Rosenbrock_x's arguments of every leg; times [nleg + 1]; carry: a later leg's RPAR(3) is the cell's previous RPAR(12) where > 0
Series = namedtuple("Series", "ipar rpar atol rtol times carry")

SET_NAMES = ("ros3_8", "ros3_unequal", "ros3_unequal_carry", "rodas4_rtol_1e-7", "ros2_vector_tol", "ros3_descending", "ros3_max_steps_3")
UNEQUAL = (0.0, 1.0e-6, 0.5, 0.5001, 7.0, 10.0)      # the first step clipped to the leg, a one-step leg, a long leg after a short one
FAILING_SETS = ("ros3_max_steps_3",)                 # every leg ends with IERR = -6 and the next goes on from the state left
METHOD_GRID = (0.0, 2.0, 2.5, 10.0)                  # the grid the five methods are compared on (tests/test_gpu_ros_series.py)


def series_set(mech, name):
    ipar, rpar, atol, rtol = R.base_options(mech)
    carry = False
    if name == "ros3_8":                   # Ros3 at INTEGRATE_x's options, 8 legs of 1.25 s
        times = np.linspace(0.0, 10.0, 9)
    elif name == "ros3_unequal":
        times = UNEQUAL
    elif name == "ros3_unequal_carry":
        times, carry = UNEQUAL, True
    elif name == "rodas4_rtol_1e-7":
        ipar[3] = 5
        rtol[:] = 1.0e-7
        # four legs inside the initial transient.  Behind it Rodas4's error estimate (its last stage alone) is at rounding level at this RelTol, and the
        # step the controller proposes moves by tens of percent under re-association: on 0, 2.5, .. 10 s the oracle's variants change aer's counters
        times = (0.0, 1.0e-4, 1.0e-3, 1.0e-2, 1.0e-1)
    elif name == "ros2_vector_tol":
        ipar, rpar, atol, rtol = R.option_set(mech, "vector_tol")
        ipar[3] = 1
        times = (0.0, 2.0, 5.0, 10.0)
    elif name == "ros3_descending":        # backward in every leg
        times = (10.0, 6.0, 0.0)
    elif name == "ros3_max_steps_3":       # Max_no_steps = 3: IERR = -6 in every leg
        ipar[2] = 3
        times = (0.0, 3.0, 6.0, 10.0)
    else:
        raise KeyError(name)
    return Series(ipar, rpar, atol, rtol, np.array(times, np.float64), carry)


def method_series(mech, method):
    """the five methods on one grid: INTEGRATE_x's other options, METHOD_GRID"""
    ipar, rpar, atol, rtol = R.base_options(mech)
    ipar[3] = method
    return Series(ipar, rpar, atol, rtol, np.array(METHOD_GRID), False)


def leg_rpar(rpar, carry, leg, hexit_prev):
    """RPAR of leg `leg` for a cell whose previous leg left Hexit = hexit_prev: its RPAR(3) under carry, else the call's own"""
    if not carry or leg == 0 or not hexit_prev > 0.0:
        return rpar
    out = np.array(rpar, np.float64)
    out[2] = hexit_prev
    return out


def chain(call, var, s):
    """One cell through the legs of `s`; call(y, rpar, tstart, tend) -> (VAR, IERR, IPAR(11:18), Texit, Hexit) is one Rosenbrock_x call.
    -> (VAR [nleg, NVAR], IERR [nleg], IPAR(11:18) [nleg, 8], Texit [nleg], Hexit [nleg])"""
    y, hexit = np.array(var, np.float64), 0.0
    rows = []
    for k in range(len(s.times) - 1):
        y, ierr, st, texit, hexit = call(y, leg_rpar(s.rpar, s.carry, k, hexit), float(s.times[k]), float(s.times[k + 1]))
        rows.append((np.array(y), ierr, np.array(st), texit, hexit))
    return tuple(np.array([r[i] for r in rows]) for i in range(5))


_restated = {}


def restated(mech, golden, variant=0, names=SET_NAMES):
    """{set name: (VAR [nleg, 3, NVAR], IERR [nleg, 3], IPAR(11:18) [nleg, 3, 8], Texit [nleg, 3], Hexit [nleg, 3])} of the chained restatement on the
    three cells of the golden set, for one oracle variant (oracle.set_variant); computed once per (mechanism, variant, set) and shared by the tests"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    o, diag, g = None, None, golden
    out = {}
    for name in names:
        key = (mech, variant, name)
        if key not in _restated:
            if o is None:
                o, diag = Oracle(mech), mechtab.load(mech).diag
            s = series_set(mech, name)
            try:
                set_variant(variant)
                cells = [chain(lambda y, rpar, t0, t1: RM.rosenbrock(o, diag, y, g["fix"][c], g["rconst"][c], s.ipar, rpar, s.atol, s.rtol, t0, t1),
                               g["var_in"][c], s) for c in cells_of(g["var_in"].shape[0])]
            finally:
                set_variant(0)
            _restated[key] = tuple(np.stack([cell[i] for cell in cells], axis=1) for i in range(5))
        out[name] = _restated[key]
    return out
