"""TEST INFRASTRUCTURE — Rosenbrock_x (gas.f:777-1108) and RosenbrockIntegrator_x (gas.f:1112-1337) restated in Python WITH their options, over
the oracle's exported primitives (Oracle.fun / jac_sp / decomp / solve), and the option sets the tests of mistra_chem_set_options run.

The restatement is pinned twice: at INTEGRATE_x's options it equals Oracle.integrate bit for bit, and on every option set below it equals the
compiled Rosenbrock_x bit for bit — VAR, IERR, IPAR(11:18), Texit, Hexit (tests/test_ros_options.py, against tests/golden/ros_options_<mech>.npz,
which tests/golden/make_ros_options_golden.py records from the compiled reference).  It exists to measure, on the reference side, how far those
results move under legal re-association (tests/ros_options_bounds.py): the compiled reference has no such variants, the oracle has.  The error
norm is summed serially, as ros_ErrorNorm_x does."""
import math

import numpy as np

ROUNDOFF = 2.220446049250313e-16       # epsilon(ONE), gas.f:973
DELTA_MIN = 1.0e-5
# Ros3_x (gas.f:1596-1626)
ROS_A1 = 1.0
ROS_C = (-0.10156171083877702091975600115545e+01, 0.40759956452537699824805835358067e+01, 0.92076794298330791242156818474003e+01)
ROS_M = (0.1e+01, 0.61697947043828245592553615689730e+01, -0.42772256543218573326238373806514e+00)
ROS_E = (0.5e+00, -0.29079558716805469821718236208017e+01, 0.22354069897811569627360909276199e+00)
ROS_GAMMA = (0.43586652150845899941601945119356e+00, 0.24291996454816804366592249683314e+00, 0.21851380027664058511513169485832e+01)
ROS_ELO = 3.0

MECHS = ("gas", "aer", "tot")
NVAR = {"gas": 102, "aer": 257, "tot": 417}
TIN, TOUT = 0.0, 10.0


def cells_of(n):
    return (0, n // 2, n - 1)


# ---- the option sets: IPAR(20), RPAR(20), AbsTol(NVAR), RelTol(NVAR) over INTEGRATE_x's base (gas.f:739-746)
def base_options(mech):
    ipar, rpar = np.zeros(20, np.int32), np.zeros(20)
    ipar[1], ipar[3] = 1, 2            # IPAR(2) = 1: scalar tolerances; IPAR(4) = 2: Ros3
    rpar[2] = 1.0e-3                   # RPAR(3): starting step
    return ipar, rpar, np.full(NVAR[mech], 1.0e-25), np.full(NVAR[mech], 1.0e-3)


SET_NAMES = ("rtol_1e-5", "rtol_1e-2_atol_1e-12", "factors", "hmax_0.5", "hmin_0.05", "vector_tol", "autonomous", "hstart_0.5", "max_steps_5")


def option_set(mech, name):
    ipar, rpar, atol, rtol = base_options(mech)
    if name == "rtol_1e-5":
        rtol[:] = 1.0e-5
    elif name == "rtol_1e-2_atol_1e-12":
        rtol[:] = 1.0e-2
        atol[:] = 1.0e-12
    elif name == "factors":
        rpar[3:7] = (0.5, 2.0, 0.25, 0.8)
    elif name == "hmax_0.5":
        rpar[1] = 0.5
    elif name == "hmin_0.05":          # steps are then accepted through H <= Hmin (gas.f:1302)
        rpar[0], rpar[2] = 0.05, 0.0
    elif name == "vector_tol":
        rng = np.random.default_rng(7)
        ipar[1] = 0
        rtol[:] = 10.0 ** rng.uniform(-4.0, -2.0, NVAR[mech])
        atol[:] = 1.0e-25 * 10.0 ** rng.uniform(0.0, 10.0, NVAR[mech])
    elif name == "autonomous":
        ipar[0] = 1
    elif name == "hstart_0.5":
        rpar[2] = 0.5
    elif name == "max_steps_5":        # IERR -6
        ipar[2] = 5
    else:
        raise KeyError(name)
    return ipar, rpar, atol, rtol


REFUSED_NAMES = ("ipar3_-1", "ipar4_9", "rpar1_-1", "rpar5_-2", "rtol_1", "atol51_0_vector")
REFUSED_IERR = {"ipar3_-1": -1, "ipar4_9": -2, "rpar1_-1": -3, "rpar5_-2": -4, "rtol_1": -5, "atol51_0_vector": -5}
ACCEPTED_EXTRA = ("atol51_0_scalar",)      # the same zero in scalar mode: entries past the first are not checked (gas.f:1045), the set runs


def refused_set(mech, name):
    ipar, rpar, atol, rtol = base_options(mech)
    if name == "ipar3_-1":
        ipar[2] = -1
    elif name == "ipar4_9":
        ipar[3] = 9
    elif name == "rpar1_-1":
        rpar[0] = -1.0
    elif name == "rpar5_-2":
        rpar[4] = -2.0
    elif name == "rtol_1":
        rtol[:] = 1.0
    elif name == "atol51_0_vector":
        ipar[1] = 0
        atol[50] = 0.0
    elif name == "atol51_0_scalar":
        atol[50] = 0.0
    else:
        raise KeyError(name)
    return ipar, rpar, atol, rtol


def any_set(mech, name):
    return option_set(mech, name) if name in SET_NAMES else refused_set(mech, name)


# ---- the restatement
def fmin_f(a, b):      # Fortran MIN / MAX as the oracle states them (oracle/kpp_ros3.c)
    return a if (a < b or b != b) else b


def fmax_f(a, b):
    return a if (a > b or b != b) else b


def resolve(ipar, rpar, atol, rtol, nvar, tstart, tend):
    """Rosenbrock_x's decode (gas.f:936-1053) -> (IERR, dict): IERR 1 and the integrator's arguments, or the refusal's code and None"""
    o = {"autonomous": ipar[0] != 0, "vector": ipar[1] == 0}
    if ipar[2] == 0:
        o["max_steps"] = 100000
    elif ipar[2] > 0:
        o["max_steps"] = int(ipar[2])
    else:
        return -1, None
    if not 0 <= ipar[3] <= 5:
        return -2, None
    o["method"] = 3 if ipar[3] == 0 else int(ipar[3])
    span = abs(tend - tstart)
    if rpar[0] == 0.0:
        o["hmin"] = 0.0
    elif rpar[0] > 0.0:
        o["hmin"] = float(rpar[0])
    else:
        return -3, None
    if rpar[1] == 0.0:
        o["hmax"] = span
    elif rpar[1] > 0.0:
        o["hmax"] = fmin_f(abs(float(rpar[1])), span)
    else:
        return -3, None
    if rpar[2] == 0.0:
        o["hstart"] = fmax_f(o["hmin"], DELTA_MIN)
    elif rpar[2] > 0.0:
        o["hstart"] = fmin_f(abs(float(rpar[2])), span)
    else:
        return -3, None
    for k, (name, default) in enumerate((("facmin", 0.2), ("facmax", 6.0), ("facrej", 0.1), ("facsafe", 0.9))):
        v = float(rpar[3 + k])
        if v == 0.0:
            o[name] = default
        elif v > 0.0:
            o[name] = v
        else:
            return -4, None
    for i in range(nvar if o["vector"] else 1):
        if atol[i] <= 0.0 or rtol[i] <= 10.0 * ROUNDOFF or rtol[i] >= 1.0:
            return -5, None
    return 1, o


def error_norm(y, ynew, yerr, atol, rtol, vector):
    """ros_ErrorNorm_x (gas.f:1341): the scaled terms elementwise, their sum serially in species order"""
    ymax = np.maximum(np.abs(y), np.abs(ynew))
    scale = atol + rtol * ymax if vector else atol[0] + rtol[0] * ymax
    q = yerr / scale
    err = 0.0
    for v in (q * q).tolist():
        err = err + v
    return math.sqrt(err / len(y))


def rosenbrock(o, diag, var, fix, rconst, ipar, rpar, atol, rtol, tstart=TIN, tend=TOUT):
    """Rosenbrock_x on one cell with oracle `o` (oracle.Oracle) and the mechanism's LU_DIAG (0-based) -> (VAR, IERR, IPAR(11:18), Texit, Hexit).
    Ros3 only.  A refusal returns VAR untouched, zero counters and Texit = Hexit = 0."""
    y = np.array(var, np.float64)
    st = np.zeros(8, np.int32)         # Nfun Njac Nstp Nacc Nrej Ndec Nsol Nsng
    ierr, p = resolve(ipar, rpar, atol, rtol, len(y), tstart, tend)
    if ierr != 1:
        return y, ierr, st, 0.0, 0.0
    assert p["method"] == 2, "the restatement has Ros3 only"
    autonomous, vector = p["autonomous"], p["vector"]
    hmin, hmax = p["hmin"], p["hmax"]
    t, hexit = tstart, 0.0
    h = fmin_f(p["hstart"], hmax)
    if abs(h) <= 10.0 * ROUNDOFF:
        h = DELTA_MIN
    direction = 1.0 if tend >= tstart else -1.0
    reject_last = reject_more = False
    n = len(y)

    def waxpy(alpha, x, yy):           # WAXPY_x (gas.f:6641)
        return yy if alpha == 0.0 else yy + alpha * x

    while abs(tend - t) >= ROUNDOFF:
        if st[2] > p["max_steps"]:
            return y, -6, st, t, hexit
        if (t + 0.1 * h) == t or h <= ROUNDOFF:
            return y, -7, st, t, hexit
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
                ghinv = 1.0 / (direction * h * ROS_GAMMA[0])
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
                    return y, -8, st, t, hexit
            k = []
            fcn = fcn0
            for istage in range(3):
                if istage == 1:        # ros_NewF(2) = .TRUE., ros_NewF(3) = .FALSE.
                    ynew = waxpy(ROS_A1, k[0], y.copy())
                    fcn = o.fun(ynew, fix, rconst)
                    st[0] += 1
                ki = fcn.copy()
                for j in range(istage):
                    hc = ROS_C[istage * (istage - 1) // 2 + j] / (direction * h)
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
            fac = fmin_f(p["facmax"], fmax_f(p["facmin"], p["facsafe"] / math.pow(err, 1.0 / ROS_ELO)))
            hnew = h * fac
            st[2] += 1
            if err <= 1.0 or h <= hmin:
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
    return y, 1, st, t, hexit


_restated = {}


def restated(mech, golden, variant=0):
    """{set name: (VAR [3, NVAR], IERR [3], IPAR(11:18) [3, 8], Texit [3], Hexit [3])} of the restatement on the three cells of the golden set, for one
    oracle variant (oracle.set_variant); computed once per (mechanism, variant) and shared by the tests"""
    key = (mech, variant)
    if key not in _restated:
        from mistra_amd import mechtab
        from oracle.oracle import Oracle, set_variant
        o, diag = Oracle(mech), mechtab.load(mech).diag
        g = golden
        out = {}
        try:
            set_variant(variant)
            for name in SET_NAMES + ACCEPTED_EXTRA:
                ipar, rpar, atol, rtol = any_set(mech, name)
                rows = [rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, atol, rtol) for c in cells_of(g["var_in"].shape[0])]
                out[name] = tuple(np.array([r[i] for r in rows]) for i in range(5))
        finally:
            set_variant(0)
        _restated[key] = out
    return _restated[key]
