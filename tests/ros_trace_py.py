"""TEST INFRASTRUCTURE — tests/ros_options_py.py's restatement of Rosenbrock_x / RosenbrockIntegrator_x (gas.f:777-1337, Ros3) with the record of
the step-control trace (include/mistra_chem.h: mistra_chem_rosenbrock_trace_ex): one record per attempt that reaches ros_ErrorNorm_x.  The decode,
the error norm and MIN / MAX are ros_options_py's.

Pinned through tests/ros_methods_py.py (itself pinned to the compiled Rosenbrock_x): VAR, IERR, IPAR(11:18), Texit, Hexit equal that restatement's
bit for bit on every set used (tests/test_ros_trace.py).  It is what the GPU trace is compared with, what tests/ros_trace_bounds.py measures the
record's movement under legal re-association on, and what tools/step_control.py --cpu runs."""
import math
from collections import namedtuple

import numpy as np

import ros_options_py as R
from ros_options_py import DELTA_MIN, MECHS, NVAR, ROS_A1, ROS_C, ROS_E, ROS_ELO, ROS_GAMMA, ROS_M, ROUNDOFF, TIN, TOUT, cells_of, error_norm, fmax_f, fmin_f, resolve  # noqa: F401

# t, h, err, share: [n] doubles; species, code: [n] int32; ctrl: [NVAR] int32 (the histogram of species); terms: per attempt the NVAR terms
# of the error norm's sum (what the species tolerance of the GPU test is taken from)
Trace = namedtuple("Trace", "t h err share species code ctrl terms")

# ---- the sets of the trace tests: ros_options_py's, and a scalar AbsTol well above INTEGRATE_x's 1e-25
SET_NAMES = ("base", "rtol_1e-2_atol_1e-12", "vector_tol", "atol_1e-15")


def trace_set(mech, name):
    if name == "base":
        return R.base_options(mech)
    if name == "atol_1e-15":
        ipar, rpar, atol, rtol = R.base_options(mech)
        atol[:] = 1.0e-15
        return ipar, rpar, atol, rtol
    return R.option_set(mech, name)


def error_terms(y, ynew, yerr, atol, rtol, vector):
    """the terms of ros_ErrorNorm_x's sum (gas.f:1361), elementwise as ros_options_py.error_norm forms them"""
    ymax = np.maximum(np.abs(y), np.abs(ynew))
    scale = atol + rtol * ymax if vector else atol[0] + rtol[0] * ymax
    q = yerr / scale
    return q * q


def largest_term(terms):
    """-> (species 1-based, term): the largest term, ties to the lowest species, a NaN never wins; (0, 0.0) where no term is positive"""
    best, at = 0.0, 0
    for i, v in enumerate(terms.tolist()):
        if v > best:
            best, at = v, i + 1
    return at, best


def fdiv(a, b):
    """a / b as the reference divides: by a zero step size (a NaN cell's last attempt, H underflown to 0) it gives an infinity, no exception"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def share_of(term, err, nvar):
    return term / ((float(nvar) * err) * err) if term > 0.0 else 0.0


def rosenbrock_trace(o, diag, var, fix, rconst, ipar, rpar, atol, rtol, tstart=TIN, tend=TOUT):
    """Rosenbrock_x (Ros3) on one cell -> (VAR, IERR, IPAR(11:18), Texit, Hexit, Trace).  A refusal returns VAR untouched, zero counters, Texit =
    Hexit = 0 and an empty trace."""
    y = np.array(var, np.float64)
    n = len(y)
    st = np.zeros(8, np.int32)         # Nfun Njac Nstp Nacc Nrej Ndec Nsol Nsng
    rec = []                           # (T, H, Err, share, species, code, terms)

    def done(ierr, t, hexit):
        ctrl = np.zeros(n, np.int32)
        for r in rec:
            if r[4] > 0:
                ctrl[r[4] - 1] += 1
        tr = Trace(np.array([r[0] for r in rec], np.float64), np.array([r[1] for r in rec], np.float64), np.array([r[2] for r in rec], np.float64),
                   np.array([r[3] for r in rec], np.float64), np.array([r[4] for r in rec], np.int32), np.array([r[5] for r in rec], np.int32), ctrl,
                   np.array([r[6] for r in rec], np.float64).reshape(len(rec), n))
        return y, ierr, st, t, hexit, tr

    ierr, p = resolve(ipar, rpar, atol, rtol, n, tstart, tend)
    if ierr != 1:
        return done(ierr, 0.0, 0.0)
    assert p["method"] == 2, "the trace is Ros3's"
    autonomous, vector = p["autonomous"], p["vector"]
    hmin, hmax = p["hmin"], p["hmax"]
    t, hexit = tstart, 0.0
    h = fmin_f(p["hstart"], hmax)
    if abs(h) <= 10.0 * ROUNDOFF:
        h = DELTA_MIN
    direction = 1.0 if tend >= tstart else -1.0
    reject_last = reject_more = False

    def waxpy(alpha, x, yy):           # WAXPY_x (gas.f:6641)
        return yy if alpha == 0.0 else yy + alpha * x

    while abs(tend - t) >= ROUNDOFF:
        if st[2] > p["max_steps"]:
            return done(-6, t, hexit)
        if (t + 0.1 * h) == t or h <= ROUNDOFF:
            return done(-7, t, hexit)
        hexit = h
        h = fmin_f(h, abs(tend - t))
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
        while True:
            nconsecutive = 0
            while True:                # ros_PrepareMatrix_x (gas.f:1404)
                ghimj = -jac0
                ghinv = fdiv(1.0, direction * h * ROS_GAMMA[0])
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
                    return done(-8, t, hexit)
            k = []
            fcn = fcn0
            for istage in range(3):
                if istage == 1:        # ros_NewF(2) = .TRUE., ros_NewF(3) = .FALSE.
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
            err = error_norm(y, ynew, yerr, atol, rtol, vector)
            terms = error_terms(y, ynew, yerr, atol, rtol, vector)
            species, term = largest_term(terms)
            fac = fmin_f(p["facmax"], fmax_f(p["facmin"], p["facsafe"] / math.pow(err, 1.0 / ROS_ELO)))
            hnew = h * fac
            st[2] += 1
            accept = err <= 1.0 or h <= hmin
            rec.append((t, h, err, share_of(term, err, n), species, (1 if accept else 0) + 2 * nconsecutive, terms))
            if accept:
                st[3] += 1
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
    return done(1, t, hexit)


_restated = {}


def restated(mech, golden, variant=0, names=SET_NAMES):
    """{set name: [rosenbrock_trace's tuple for each of the three cells of the golden set]} for one oracle variant (oracle.set_variant); computed
    once per (mechanism, variant, set) and shared by the tests"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    o, diag, g = None, None, golden
    out = {}
    for name in names:
        key = (mech, variant, name)
        if key not in _restated:
            if o is None:
                o, diag = Oracle(mech), mechtab.load(mech).diag
            try:
                set_variant(variant)
                _restated[key] = [rosenbrock_trace(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *trace_set(mech, name))
                                  for c in cells_of(g["var_in"].shape[0])]
            finally:
                set_variant(0)
        out[name] = _restated[key]
    return out
