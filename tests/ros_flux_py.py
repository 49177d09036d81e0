"""TEST INFRASTRUCTURE — tests/ros_methods_py.py's restatement of Rosenbrock_x with the reaction flux of mistra_chem_rosenbrock_flux_ex added
(INTEGRATION.md §4n), and the sets its tests run.

    flux[r] = sum over the accepted steps n, in time order, of (0.5 * (D*H_n)) * (A_r(Y_n) + A_r(Y_n+1)),   flux[r] starting at +0.0

A_r(Y) is read from Oracle.work[:nreact] right behind Oracle.fun(Y): kpp_fun leaves the products RCT(r)*X*X*X there.  A_r(Y_n), n < N, is what the
step's own first Fun_x formed; A_r(Y_N) takes one more evaluation at the state the call returns (normal return, -6, -7), which is no Fun_x call and is
not counted.  After -8 the failing step's own Fun_x has closed the last accepted step.  Everything else is ros_methods_py.rosenbrock statement for
statement: VAR, IERR, IPAR(11:18), Texit, Hexit are its bits (tests/test_ros_flux.py holds that on every set used)."""
import math

import numpy as np

import ros_methods_py as RM
from ros_methods_py import DELTA_MIN, MECHS, ROUNDOFF, TIN, TOUT, cells_of, error_norm, fmax_f, fmin_f, resolve, table  # noqa: F401

# the sets of the whole-call tests (ros_methods_py.method_set): the five methods at INTEGRATE_x's options, Rodas3 backward, Rodas4 stopped by
# Max_no_steps (IERR = -6: the closing evaluation at Texit), Rodas3 with vector tolerances
FLUX_SETS = ("m1", "m2", "m3", "m4", "m5", "m4_backward", "m5_max_steps_5", "m4_vector_tol")
FLUX_VARIANTS = (1, 2, 4)      # oracle.set_variant: the re-associations the bounds are measured under
SINGLE_TEND = 1.0e-3           # the single-step call: Tstart = 0, Tend = 1e-3 = INTEGRATE_x's Hstart, AbsTol = 1e30, RelTol = 0.5 (scalar)


def single_step_set(mech, method):
    """-> (IPAR, RPAR, AbsTol, RelTol, Tstart, Tend) of the call that makes exactly one attempt, accepted: every Err is far below 1"""
    ipar, rpar, atol, rtol = RM.R.base_options(mech)
    ipar[3] = method
    atol[:] = 1.0e30
    rtol[:] = 0.5
    return ipar, rpar, atol, rtol, 0.0, SINGLE_TEND


def products(o, y, fix, rconst):
    """-> (Fun_x(y), A [NREACT]): the oracle's function value and the products it formed on the way"""
    f = o.fun(y, fix, rconst)
    return f, o.work[:o.nreact].copy()


def rosenbrock(o, diag, var, fix, rconst, ipar, rpar, atol, rtol, tstart=TIN, tend=TOUT):
    """ros_methods_py.rosenbrock -> (VAR, IERR, IPAR(11:18), Texit, Hexit, flux [NREACT])"""
    y = np.array(var, np.float64)
    st = np.zeros(8, np.int32)         # Nfun Njac Nstp Nacc Nrej Ndec Nsol Nsng
    flux = np.zeros(o.nreact)
    ierr, p = resolve(ipar, rpar, atol, rtol, len(y), tstart, tend)
    if ierr != 1:
        return y, ierr, st, 0.0, 0.0, flux
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
    a_prev, half = None, None          # A(Y_n) and 0.5*(D*H_n) of the accepted step that is still open (half is None: no step is open)

    def waxpy(alpha, x, yy):           # WAXPY_x (gas.f:6641): returns at once for a zero coefficient
        return yy if alpha == 0.0 else yy + alpha * x

    def close(a_now):
        nonlocal flux, half
        if half is not None:
            flux = flux + half * (a_prev + a_now)
            half = None

    def leave(code):                   # the closing evaluation at the state the call returns: not a Fun_x call, not counted
        if half is not None:
            close(products(o, y, fix, rconst)[1])
        return y, code, st, t, hexit, flux

    while abs(tend - t) >= ROUNDOFF:
        if st[2] > p["max_steps"]:
            return leave(-6)
        if (t + 0.1 * h) == t or h <= ROUNDOFF:
            return leave(-7)
        hexit = h
        h = fmin_f(h, abs(tend - t))
        fcn0, a_now = products(o, y, fix, rconst)
        close(a_now)
        a_prev = a_now
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
                    return y, -8, st, t, hexit, flux      # (the step's own Fun_x has closed the last accepted step)
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
                y = ynew
                t = t + direction * h
                half = 0.5 * (direction * h)
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


def _rows(mech, golden, variant, key, args):
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    if key not in _restated:
        o, diag, g = Oracle(mech), mechtab.load(mech).diag, golden
        try:
            set_variant(variant)
            rows = [rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *args) for c in cells_of(g["var_in"].shape[0])]
        finally:
            set_variant(0)
        _restated[key] = tuple(np.array([r[i] for r in rows]) for i in range(6))
    return _restated[key]


def restated(mech, golden, variant=0, names=FLUX_SETS):
    """{set name: (VAR [3, NVAR], IERR [3], IPAR(11:18) [3, 8], Texit [3], Hexit [3], flux [3, NREACT])} of the restatement on the three cells of the
    golden set, for one oracle variant; computed once per (mechanism, variant, set) and shared by the tests"""
    return {name: _rows(mech, golden, variant, (mech, variant, name), RM.method_set(mech, name)) for name in names}


def restated_single(mech, golden, method):
    """the single-step call of one method on the same three cells, the pinned oracle"""
    return _rows(mech, golden, 0, (mech, 0, "single", method), single_step_set(mech, method))


def stoich(mech):
    """S [NVAR, NREACT] of the mechanism's table (mechtab.MechTables.stoich)"""
    from mistra_amd import mechtab
    return mechtab.load(mech).stoich()
