"""TEST INFRASTRUCTURE — tests/ros_methods_py.py's restatement of Rosenbrock_x with the dense output of mistra_chem_rosenbrock_dense_ex added
(INTEGRATION.md §4o), the sample-time sets its tests run, and the interpolant on its own.

The call's accepted states are Y_0 .. Y_N at T_0 = Tstart, T_(n+1) = T_n + dh_n (dh_n = Direction*H_n), F_n = Fun_x(Y_n) as the step's own first Fun_x
forms it.  Samples are taken in order: behind step n every one with Direction*(ts[k] - T_(n+1)) <= 0, on a normal return every one left (to the last
accepted step), after -6 / -7 / -8 none of the ones left.  F_(n+1) is the next step's first Fun_x; on a normal return and on -6 / -7 one more evaluation
at the state the call returns, not counted, made only where a sample is still to be taken; after -8 the failing step's own Fun_x has closed the last
accepted step.  The value is hermite() below, operation for operation.  Everything else is ros_methods_py.rosenbrock statement for statement (as
tests/ros_flux_py.py is, whose close() / leave() became "take the samples of the open step"): VAR, IERR, IPAR(11:18), Texit, Hexit are its bits
(tests/test_ros_dense.py holds that on every set used)."""
import math

import numpy as np

import ros_flux_py as RF
import ros_methods_py as RM
from ros_methods_py import DELTA_MIN, MECHS, ROUNDOFF, TIN, TOUT, cells_of, error_norm, fmax_f, fmin_f, resolve, table  # noqa: F401

DENSE_SETS = RF.FLUX_SETS      # the five methods at INTEGRATE_x's options, Rodas3 backward, Rodas4 stopped by Max_no_steps (-6), Rodas3 with vector tolerances
MAX_TIMES = 4096               # MISTRA_DENSE_MAX_TIMES

# ---- the named sample-time sets of the fixtures' 0 -> 10 s calls
END = np.array([10.0])
LINEAR8 = np.linspace(0.0, 10.0, 9)[1:]
EARLY = np.array([2.5e-4, 5.0e-4, 1.0e-3, 1.5e-3])      # three in the first step (1e-3 where the first attempt is accepted), one exactly on its end, one just behind
CLUSTER = np.linspace(9.0, 9.5, 64)                     # many samples inside one late, long step
BACKWARD = np.linspace(10.0, 0.0, 9)[1:]                # the backward set's: descending, the last one on its Tend = 0
EARLY_LINEAR8 = np.concatenate([EARLY, LINEAR8])        # the Max_no_steps set's: some reached, some not ...
# ... on gas.  Rodas4 stopped after five steps leaves aer at Texit = 1.5e-11 .. 3.7e-10 s and tot at 1.2e-13 .. 8.4e-13 s (rejections in the initial
# transient): none of EARLY_LINEAR8 is reached there.  So the set runs with four more times in front, two below tot's smallest Texit and two below aer's:
# 0 < nout < ns on every test cell of every mechanism, and all of EARLY_LINEAR8 is still in it.
TINY = np.array([1.0e-14, 5.0e-14, 1.0e-12, 1.0e-11])
MAX_STEPS = np.concatenate([TINY, EARLY_LINEAR8])
FORWARD = np.concatenate([EARLY, LINEAR8[:7], CLUSTER, END])      # what a completed forward set is run with: every named set in one call, Tend last
TIME_SETS = {"end": END, "linear8": LINEAR8, "early": EARLY, "cluster": CLUSTER, "backward": BACKWARD, "early_linear8": EARLY_LINEAR8, "max_steps": MAX_STEPS,
             "forward": FORWARD}
SINGLE_TS = np.array([2.5e-4, 5.0e-4, 1.0e-3])          # of ros_flux_py.single_step_set's call, 0 -> 1e-3 in one accepted attempt


def times_of(name):
    """the sample times a whole-call set is run with"""
    if name == "m4_backward":
        return BACKWARD
    if name == "m5_max_steps_5":
        return MAX_STEPS
    return FORWARD


def hermite(y0, f0, y1, f1, dh, th):
    """the sample's value as INTEGRATION.md §4o defines it: every multiply, add and subtract rounded once, in this order"""
    d = y1 - y0
    hf0 = dh * f0
    hf1 = dh * f1
    om = 1.0 - th
    c = ((1.0 - 2.0 * th) * d - om * hf0) + th * hf1
    return (om * y0 + th * y1) - (th * om) * c


def rosenbrock(o, diag, var, fix, rconst, ts, ipar, rpar, atol, rtol, tstart=TIN, tend=TOUT):
    """ros_methods_py.rosenbrock -> (VAR, IERR, IPAR(11:18), Texit, Hexit, samples [ns, NVAR], nout)"""
    y = np.array(var, np.float64)
    st = np.zeros(8, np.int32)         # Nfun Njac Nstp Nacc Nrej Ndec Nsol Nsng
    ts = np.asarray(ts, np.float64)
    samples = np.zeros((len(ts), len(y)))
    ierr, p = resolve(ipar, rpar, atol, rtol, len(y), tstart, tend)
    if ierr != 1:
        return y, ierr, st, 0.0, 0.0, samples, 0
    tb = table(p["method"])
    autonomous, vector = p["autonomous"], p["vector"]
    hmin, hmax = p["hmin"], p["hmax"]
    t, hexit = tstart, 0.0
    h = fmin_f(p["hstart"], hmax)
    if abs(h) <= 10.0 * ROUNDOFF:
        h = DELTA_MIN
    direction = 1.0 if tend >= tstart else -1.0
    reject_last = reject_more = False
    n = len(y)
    opened = None                      # (Y_n, F_n, T_n, dh_n) of the accepted step that is still open
    k_next = 0                         # samples taken so far

    def waxpy(alpha, x, yy):           # WAXPY_x (gas.f:6641): returns at once for a zero coefficient
        return yy if alpha == 0.0 else yy + alpha * x

    def take(f1, every):               # y, t hold Y_(n+1), T_(n+1)
        nonlocal opened, k_next
        y0, f0, t0, dh = opened
        while k_next < len(ts):
            tk = float(ts[k_next])
            if not every and not (direction * (tk - t) <= 0.0):
                break
            samples[k_next] = hermite(y0, f0, y, f1, dh, (tk - t0) / dh)
            k_next += 1
        opened = None

    def leave(code):                   # the closing evaluation at the state the call returns: not counted, only where a sample is still to be taken
        if opened is not None and k_next < len(ts):
            take(o.fun(y, fix, rconst), code == 1)
        return y, code, st, t, hexit, samples, k_next

    while abs(tend - t) >= ROUNDOFF:
        if st[2] > p["max_steps"]:
            return leave(-6)
        if (t + 0.1 * h) == t or h <= ROUNDOFF:
            return leave(-7)
        hexit = h
        h = fmin_f(h, abs(tend - t))
        fcn0 = o.fun(y, fix, rconst)
        if opened is not None:
            take(fcn0, False)
        st[0] += 1
        if not autonomous:             # ros_FunTimeDerivative_x (gas.f:1375)
            delta = math.sqrt(ROUNDOFF) * fmax_f(1.0e-6, abs(t))
            dfdt = o.fun(y, fix, rconst)
            st[0] += 1
            dfdt = waxpy(-1.0, fcn0, dfdt)
            dfdt = (1.0 / delta) * dfdt
        jac0 = o.jac_sp(y, fix, rconst)
        st[1] += 1
        while True:
            nconsecutive = 0
            while True:                # ros_PrepareMatrix_x (gas.f:1404)
                ghimj = -jac0
                ghinv = 1.0 / (direction * h * tb.gamma[0])
                ghimj[diag] = ghimj[diag] + ghinv
                ghimj, ising = o.decomp(ghimj)
                st[5] += 1
                if ising == 0:
                    break
                st[7] += 1
                nconsecutive += 1
                if nconsecutive <= 5:
                    h = h * 0.5
                else:
                    return y, -8, st, t, hexit, samples, k_next      # (the step's own Fun_x has closed the last accepted step)
            k = []
            fcn = fcn0
            for istage in range(tb.S):         # gas.f:1241-1276
                row = istage * (istage - 1) // 2
                if istage >= 1 and tb.newf[istage]:
                    ynew = y.copy()
                    for j in range(istage):
                        ynew = waxpy(tb.A[row + j], k[j], ynew)
                    fcn = o.fun(ynew, fix, rconst)
                    st[0] += 1
                ki = fcn.copy()
                for j in range(istage):
                    hc = tb.C[row + j] / (direction * h)
                    ki = waxpy(hc, k[j], ki)
                if not autonomous and tb.gamma[istage] != 0.0:
                    hg = direction * h * tb.gamma[istage]
                    ki = waxpy(hg, dfdt, ki)
                k.append(o.solve(ghimj, ki))
                st[6] += 1
            ynew = y.copy()
            for j in range(tb.S):
                ynew = waxpy(tb.M[j], k[j], ynew)
            yerr = np.zeros(n)
            for j in range(tb.S):
                yerr = waxpy(tb.E[j], k[j], yerr)
            err = error_norm(y, ynew, yerr, atol, rtol, vector)
            fac = fmin_f(p["facmax"], fmax_f(p["facmin"], p["facsafe"] / math.pow(err, 1.0 / tb.elo)))
            hnew = h * fac
            st[2] += 1
            if err <= 1.0 or h <= hmin:
                st[3] += 1
                opened = (y, fcn0, t, direction * h)
                y = ynew
                t = t + direction * h
                hnew = fmax_f(hmin, fmin_f(hnew, hmax))
                if reject_last:
                    hnew = fmin_f(hnew, h)
                reject_last = reject_more = False
                h = hnew
                break
            if reject_more:
                hnew = h * p["facrej"]
            reject_more = reject_last
            reject_last = True
            h = hnew
            if st[3] >= 1:
                st[4] += 1
    return leave(1)


_restated = {}


def _rows(mech, golden, variant, key, ts, args):
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    if key not in _restated:
        o, diag, g = Oracle(mech), mechtab.load(mech).diag, golden
        try:
            set_variant(variant)
            rows = [rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], ts, *args) for c in cells_of(g["var_in"].shape[0])]
        finally:
            set_variant(0)
        _restated[key] = tuple(np.array([r[i] for r in rows]) for i in range(7))
    return _restated[key]


def restated(mech, golden, variant=0, names=DENSE_SETS):
    """{set name: (VAR [3, NVAR], IERR [3], IPAR(11:18) [3, 8], Texit [3], Hexit [3], samples [3, ns, NVAR], nout [3])} of the restatement on the three
    cells of the golden set with the set's sample times (times_of), for one oracle variant; computed once per (mechanism, variant, set) and shared"""
    return {name: _rows(mech, golden, variant, (mech, variant, name), times_of(name), RM.method_set(mech, name)) for name in names}


def restated_single(mech, golden, method):
    """the single-step call of one method (ros_flux_py.single_step_set) sampled at SINGLE_TS on the same three cells, the pinned oracle"""
    return _rows(mech, golden, 0, (mech, 0, "single", method), SINGLE_TS, RF.single_step_set(mech, method))
