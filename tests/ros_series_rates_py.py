"""TEST INFRASTRUCTURE — a series of Rosenbrock_x calls with rate constants and FIX of the leg's own (mistra_chem_rosenbrock_series_rates_ex) restated on
the CPU: tests/ros_series_py.py's chain over tests/ros_methods_py.py's restatement of Rosenbrock_x, every leg with the leg's rows, the sets the tests
run and the ramp that makes the rows.

The ramp: the state, FIX F0 and the night rate constants K0 of cells 0, n/2, n-1 of tests/golden/integrate_<mech>.npz, the day rows K1, F1 of cells
0, n/2, n-1 of integrate_<mech>_day.npz; leg k of times = (0, 2.5, 5, 7.5, 10) integrates with (1-w)*K0 + w*K1 and (1-w)*F0 + w*F1 at w = (0, .25, .5,
1)[k], evaluated in float64 numpy as written: a dawn in four steps of the model's operator splitting.  Day and night cells are different places: the
ramp is an input that moves every rate constant, not a simulation.

Pinned as the series' restatement is: on every set below the chain equals the compiled Rosenbrock_x called leg by leg with the leg's rows in COMMON
/GDATA_x/, bit for bit in every leg (tests/test_ros_series_rates.py, against tests/golden/ros_series_rates_<mech>.npz, recorded by
tests/golden/make_ros_series_rates_golden.py from the compiled reference)."""
import os

import numpy as np

import ros_methods_py as RM
import ros_options_py as R
import ros_series_py as RS
from ros_options_py import MECHS, NVAR, cells_of  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIMES = (0.0, 2.5, 5.0, 7.5, 10.0)
W = (0.0, 0.25, 0.5, 1.0)
# name -> what varies by leg.  The first three are the issue's; "ros2_fix_per_leg": FIX the leg's own and the rate constants shared (K0)
SET_NAMES = ("ros3", "ros3_carry", "rodas4", "ros2_fix_per_leg", "ros3_max_steps_3")
FAILING_SETS = ("ros3_max_steps_3",)


def series_set(mech, name):
    """-> (ros_series_py.Series, rconst by leg?, fix by leg?)"""
    ipar, rpar, atol, rtol = R.base_options(mech)
    carry, per_k, per_f = False, True, True
    if name == "ros3":
        pass
    elif name == "ros3_carry":
        carry = True
    elif name == "rodas4":
        ipar[3] = 5
    elif name == "ros2_fix_per_leg":
        ipar[3] = 1
        per_k = False
    elif name == "ros3_max_steps_3":      # Max_no_steps = 3: IERR = -6 in every leg, each leg going on with its own rows
        ipar[2] = 3
    else:
        raise KeyError(name)
    return RS.Series(ipar, rpar, atol, rtol, np.array(TIMES, np.float64), carry), per_k, per_f


def ramp(mech):
    """-> (VAR [3, NVAR], leg FIX [4, 3, NFIX], leg RCONST [4, 3, NREACT]) of the golden sets"""
    g = np.load(os.path.join(GOLDEN, "integrate_%s.npz" % mech))
    d = np.load(os.path.join(GOLDEN, "integrate_%s_day.npz" % mech))
    c, cd = list(cells_of(g["var_in"].shape[0])), list(cells_of(d["var_in"].shape[0]))
    return g["var_in"][c], blend(g["fix"][c], d["fix"][cd]), blend(g["rconst"][c], d["rconst"][cd])


def blend(a0, a1, w=W):
    return np.stack([(1 - x) * a0 + x * a1 for x in w])


def leg_rows(name, mech, leg_fix, leg_k):
    """the arrays a set hands to the entry: (fix, rconst), each [nleg, ncell, .] where it is the leg's own and [ncell, .] (block 0) where shared"""
    _, per_k, per_f = series_set(mech, name)
    return (leg_fix if per_f else leg_fix[0]), (leg_k if per_k else leg_k[0])


def chain_rates(call, var, s, fix_legs, k_legs):
    """ros_series_py.chain with the leg's rows: call(y, fix, rconst, rpar, tstart, tend) is one Rosenbrock_x call; fix_legs / k_legs: [nleg, .] of the
    cell, or [.] shared"""
    leg = iter(range(len(s.times) - 1))

    def one(y, rpar, t0, t1):
        k = next(leg)
        return call(y, fix_legs[k] if fix_legs.ndim == 2 else fix_legs, k_legs[k] if k_legs.ndim == 2 else k_legs, rpar, t0, t1)
    return RS.chain(one, var, s)


_restated = {}


def restated(mech, variant=0, names=SET_NAMES):
    """{set name: (VAR [nleg, 3, NVAR], IERR [nleg, 3], IPAR(11:18) [nleg, 3, 8], Texit [nleg, 3], Hexit [nleg, 3])} of the chained restatement on the
    ramp, for one oracle variant; computed once per (mechanism, variant, set) and shared by the tests"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    o = diag = rows = None
    out = {}
    for name in names:
        key = (mech, variant, name)
        if key not in _restated:
            if o is None:
                o, diag, rows = Oracle(mech), mechtab.load(mech).diag, ramp(mech)
            V, LF, LK = rows
            s, _, _ = series_set(mech, name)
            F, K = leg_rows(name, mech, LF, LK)
            try:
                set_variant(variant)
                cells = [chain_rates(lambda y, f, k, rpar, t0, t1: RM.rosenbrock(o, diag, y, f, k, s.ipar, rpar, s.atol, s.rtol, t0, t1),
                                     V[c], s, F[:, c] if F.ndim == 3 else F[c], K[:, c] if K.ndim == 3 else K[c]) for c in range(V.shape[0])]
            finally:
                set_variant(0)
            _restated[key] = tuple(np.stack([cell[i] for cell in cells], axis=1) for i in range(5))
        out[name] = _restated[key]
    return out
