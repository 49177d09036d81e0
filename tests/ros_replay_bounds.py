"""Bounds of the tests of the replay on the GPU (tests/test_gpu_ros_replay.py), MEASURED ON THE REFERENCE SIDE exactly as tests/ros_trace_bounds.py
measures its own: nothing here looks at the kernel.  The expected values are those of the restatement (tests/ros_replay_py.py, pinned through
tests/ros_trace_py.py to the compiled Rosenbrock_x); the spread is the movement of the restated replay under the oracle's legal re-associations
(oracle.set_variant over parity_bounds.VARIANTS) along the FROZEN accepted steps of the pinned restated trace, on the trace tests' own sets
(ros_trace_py.SET_NAMES), cells 0, n/2, n-1 of integrate_<mech>.npz, 0 -> 10 s.  tests/test_ros_replay.py re-measures every figure and holds every
constant to [10x, 100x] of it, with floor parity_bounds.PARITY_FLOOR (check_constant): the margin ros_trace_bounds uses.

Premise, held by the same test: no variant changes IERR or the counters on any (set, cell).  Texit does not move at all: it is a sum of the
prescribed steps.

  measured (CPU):  VAR, worst rel_diff (conftest)   gas 4.36e-17   aer 1.81e-6   tot 5.23e-8
                   Err, relative                    gas 4.61e-5    aer 1.08e-2   tot 3.54e-7"""
import numpy as np

import parity_bounds as pb

# VAR against the restated replay, rel_diff of conftest.  gas: 10x the spread is below the floor
REPLAY_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 1.9e-5, "tot": 5.3e-7}
# Err of every step, relative: small error estimates are differences of nearly equal stage vectors (ros_trace_bounds)
REPLAY_ERR_RTOL = {"gas": 4.7e-4, "aer": 1.1e-1, "tot": 3.6e-6}

# ---- the internal-differentiation property (tests/test_ros_replay.py), on the restatement: gas, cell IND_CELL of integrate_gas_day.npz (daylight: the
# night cells of integrate_gas.npz run into FacMax at every step whatever is perturbed, so their adaptive copies share one sequence anyway), INTEGRATE_x's
# options with RelTol = IND_RTOL, three parameters — the most abundant species and the two rate constants the end state answers to most — and central
# differences at IND_EPS and IND_EPS / 10.  dy_diff of the two: replayed along the base cell's accepted steps, and taken from adaptive calls.  The
# bound on the replayed pair is its own measured disagreement times the margin above (10x, rounded up); the adaptive pair must lie above the replayed.
#   measured (CPU):  replayed pair 1.163e-3   adaptive pair 2.58
IND_SET = "_day"
IND_CELL = 0
IND_RTOL = 1.0e-4
IND_EPS = 1.0e-4
IND_PARAMS = (("var", 4), ("rconst", 29), ("rconst", 37))
IND_REPLAY_TOL = 1.2e-2


def ind_options():
    import ros_trace_py as RT
    ipar, rpar, atol, rtol = RT.trace_set("gas", "base")
    rtol = rtol.copy()
    rtol[:] = IND_RTOL
    return ipar, rpar, atol, rtol


def var_diff(got, want):
    from conftest import rel_diff
    return float(rel_diff(got, want).max())


def err_diff(got, want):
    """largest relative difference of the steps' Err; two equal values (two NaNs) count 0"""
    a, b = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if a.size == 0:
        return 0.0
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(same, 0.0, np.abs(a - b) / np.where(b != 0.0, np.abs(b), 1.0))
    return float(np.where(np.isnan(d), np.inf, d).max())


def dy_diff(a, b):
    """two sets of derivatives [P, NVAR] -> the largest difference of a row on the scale of the row's largest entry"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max(axis=1, keepdims=True)
    return float((np.abs(a - b) / np.where(scale > 0.0, scale, 1.0)).max())


def dy_bound(mech, want_var, p, eps):
    """what the state bound allows the derivative of parameter value p to move by, per species [NVAR]: both perturbed end states within REPLAY_RTOL of
    rel_diff's scale, divided by 2*eps*|p|"""
    want = np.asarray(want_var, np.float64)
    scale = np.abs(want) + 1e-12 * np.abs(want).max()
    return 2.0 * REPLAY_RTOL[mech] * scale / (2.0 * eps * abs(p))


def measure_spread(mech, golden_set, names=None):
    """-> (VAR spread, Err spread, [(variant, set, cell) whose IERR, counters or Texit moved]) of the restated replay over parity_bounds.VARIANTS"""
    import ros_replay_py as RP
    import ros_trace_py as RT
    names = RT.SET_NAMES if names is None else names
    base = RP.restated(mech, golden_set, 0, names)
    s_var, s_err, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = RP.restated(mech, golden_set, v, names)
        for name in names:
            for c, (b, x) in enumerate(zip(base[name], r[name])):
                if not (b[1] == x[1] and np.array_equal(b[2], x[2]) and b[3] == x[3] and len(b[5]) == len(x[5])):
                    moved.append((v, name, c))
                    continue
                s_var = max(s_var, var_diff(x[0], b[0]))
                s_err = max(s_err, err_diff(x[5], b[5]))
    return s_var, s_err, moved


def measure_ind(golden_gas):
    """golden_gas: integrate_gas<IND_SET>.npz -> (disagreement of the replayed pair, of the adaptive pair) of the internal-differentiation case above"""
    import ros_replay_py as RP
    import ros_trace_py as RT
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag, g = Oracle("gas"), mechtab.load("gas").diag, golden_gas
    c = IND_CELL
    cell = (g["var_in"][c], g["fix"][c], g["rconst"][c])
    opts = ind_options()
    hs = RP.accepted(RT.rosenbrock_trace(o, diag, *cell, *opts)[5])
    pair = lambda h: [RP.sensitivity_restated(o, diag, *cell, opts, IND_PARAMS, e, h) for e in (IND_EPS, IND_EPS / 10.0)]  # noqa: E731
    rep, ada = pair(hs), pair(None)
    return dy_diff(rep[1], rep[0]), dy_diff(ada[1], ada[0])
