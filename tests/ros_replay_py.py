"""TEST INFRASTRUCTURE — the fixed-sequence mode of tests/ros_trace_py.py's restatement of Rosenbrock_x (Ros3): the replay of include/mistra_chem.h
(mistra_chem_rosenbrock_replay_ex).  The steps are an input, every one is accepted, its Err is returned; the oracle calls of a step are
rosenbrock_trace's, in its order.  No clipping to Tend, no Max_no_steps, no halving at a zero pivot; Hmin, Hmax, Hstart and the factors are not read.

Pinned through tests/ros_trace_py.py: the replay of a restated trace's accepted steps gives that call's VAR and Texit bit for bit and its accepted
records' Err (tests/test_ros_replay.py).  It is what the GPU replay is compared with, what tests/ros_replay_bounds.py measures the movement under
legal re-association on, and what tools/sensitivity.py --restated runs."""
import math

import numpy as np

import ros_trace_py as RT
from ros_trace_py import ROS_A1, ROS_C, ROS_E, ROS_GAMMA, ROS_M, ROUNDOFF, TIN, TOUT, cells_of, error_norm, fdiv, fmax_f, resolve  # noqa: F401


def accepted(tr):
    """the H of a Trace's accepted records, in order"""
    return np.asarray(tr.h, np.float64)[(np.asarray(tr.code) & 1) == 1]


def rosenbrock_replay(o, diag, var, fix, rconst, ipar, rpar, atol, rtol, hsteps, tstart=TIN, tend=TOUT):
    """One cell along hsteps -> (VAR, IERR, IPAR(11:18), Texit, Hexit, Err per step made).  A refusal returns VAR untouched, zero counters, Texit = Hexit
    = 0 and no Err.  Hexit: the last step made, 0 where none was."""
    y = np.array(var, np.float64)
    n = len(y)
    st = np.zeros(8, np.int32)         # Nfun Njac Nstp Nacc Nrej Ndec Nsol Nsng
    errs = []
    ierr, p = resolve(ipar, rpar, atol, rtol, n, tstart, tend)
    if ierr != 1:
        return y, ierr, st, 0.0, 0.0, np.zeros(0)
    assert p["method"] == 2, "the replay is Ros3's"
    autonomous, vector = p["autonomous"], p["vector"]
    t, hexit = tstart, 0.0
    direction = 1.0 if tend >= tstart else -1.0

    def done(code):
        return y, code, st, t, hexit, np.array(errs, np.float64)

    def waxpy(alpha, x, yy):           # WAXPY_x (gas.f:6641)
        return yy if alpha == 0.0 else yy + alpha * x

    for h in np.asarray(hsteps, np.float64).tolist():
        if (t + 0.1 * h) == t or h <= ROUNDOFF:
            return done(-7)
        fcn0 = o.fun(y, fix, rconst)
        st[0] += 1
        if not autonomous:             # ros_FunTimeDerivative_x (gas.f:1375)
            delta = math.sqrt(ROUNDOFF) * fmax_f(1.0e-6, abs(t))
            dfdt = o.fun(y, fix, rconst)
            st[0] += 1
            dfdt = waxpy(-1.0, fcn0, dfdt)
            dfdt = (1.0 / delta) * dfdt
        jac0 = o.jac_sp(y, fix, rconst)
        st[1] += 1
        ghimj = -jac0                  # ros_PrepareMatrix_x (gas.f:1404), once: a prescribed step is not halved
        ghinv = fdiv(1.0, direction * h * ROS_GAMMA[0])
        ghimj[diag] = ghimj[diag] + ghinv
        ghimj, ising = o.decomp(ghimj)
        st[5] += 1
        if ising != 0:
            st[7] += 1
            return done(-8)
        k = []
        fcn = fcn0
        for istage in range(3):
            if istage == 1:            # ros_NewF(2) = .TRUE., ros_NewF(3) = .FALSE.
                ynew = waxpy(ROS_A1, k[0], y.copy())
                fcn = o.fun(ynew, fix, rconst)
                st[0] += 1
            ki = fcn.copy()
            for j in range(istage):
                hc = fdiv(ROS_C[istage * (istage - 1) // 2 + j], direction * h)
                ki = waxpy(hc, k[j], ki)
            if not autonomous and ROS_GAMMA[istage] != 0.0:
                hg = direction * h * ROS_GAMMA[istage]
                ki = waxpy(hg, dfdt, ki)
            k.append(o.solve(ghimj, ki))
            st[6] += 1
        ynew = y.copy()
        for j in range(3):
            ynew = waxpy(ROS_M[j], k[j], ynew)
        yerr = np.zeros(n)
        for j in range(3):
            yerr = waxpy(ROS_E[j], k[j], yerr)
        errs.append(error_norm(y, ynew, yerr, atol, rtol, vector))
        st[2] += 1
        st[3] += 1
        y = ynew
        t = t + direction * h
        hexit = h
    return done(1)


_restated = {}


def restated(mech, golden, variant=0, names=RT.SET_NAMES):
    """{set name: [rosenbrock_replay's tuple for each of the three cells of the golden set]} for one oracle variant, every cell along the accepted
    steps of the PINNED restated trace (variant 0) of that set and cell: the sequence is frozen, only the arithmetic of the steps moves.  Computed once
    per (mechanism, variant, set) and shared by the tests."""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    base = RT.restated(mech, golden, 0, names)
    o, diag, g = None, None, golden
    out = {}
    for name in names:
        key = (mech, variant, name)
        if key not in _restated:
            if o is None:
                o, diag = Oracle(mech), mechtab.load(mech).diag
            try:
                set_variant(variant)
                _restated[key] = [rosenbrock_replay(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *RT.trace_set(mech, name), accepted(base[name][i][5]))
                                  for i, c in enumerate(cells_of(g["var_in"].shape[0]))]
            finally:
                set_variant(0)
        out[name] = _restated[key]
    return out


def sensitivity_restated(o, diag, var, fix, rconst, opts, params, eps, hsteps=None, tstart=TIN, tend=TOUT):
    """dy [P, NVAR] = (y+ - y-) / (2*eps*p) of one cell on the CPU: along hsteps (the internal differentiation of chem.sensitivities), or, hsteps
    None, from plain adaptive calls.  params as chem.sensitivities takes them."""
    base = {"var": np.array(var, np.float64), "fix": np.array(fix, np.float64), "rconst": np.array(rconst, np.float64)}
    dy = []
    for what, i in params:
        p = base[what][i]
        ends = []
        for s in (1.0, -1.0):
            cell = {k: v.copy() for k, v in base.items()}
            cell[what][i] = p * (1.0 + s * eps)
            if hsteps is None:
                ends.append(RT.rosenbrock_trace(o, diag, cell["var"], cell["fix"], cell["rconst"], *opts, tstart=tstart, tend=tend)[0])
            else:
                ends.append(rosenbrock_replay(o, diag, cell["var"], cell["fix"], cell["rconst"], *opts, hsteps, tstart=tstart, tend=tend)[0])
        dy.append((ends[0] - ends[1]) / (2.0 * eps * p))
    return np.array(dy)
