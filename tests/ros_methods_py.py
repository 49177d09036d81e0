"""TEST INFRASTRUCTURE — tests/ros_options_py.py's restatement of Rosenbrock_x / RosenbrockIntegrator_x (gas.f:777-1337) generalised over the five
method tables (Ros2_x .. Rodas4_x, gas.f:1514-1895), and the sets the tests of mistra_chem_rosenbrock_ex run.  The decode, the error norm and
MIN / MAX are ros_options_py's.

Pinned as that one is: on every set below it equals the compiled Rosenbrock_x bit for bit — VAR, IERR, IPAR(11:18), Texit, Hexit
(tests/test_ros_methods.py, against tests/golden/ros_methods_<mech>.npz, which tests/golden/make_ros_methods_golden.py records from the compiled
reference).  It exists to measure, on the reference side, how far those results move under legal re-association (tests/ros_methods_bounds.py)."""
import math
from collections import namedtuple

import numpy as np

import ros_options_py as R
from ros_options_py import DELTA_MIN, MECHS, NVAR, ROUNDOFF, TIN, TOUT, cells_of, error_norm, fmax_f, fmin_f, resolve  # noqa: F401

Table = namedtuple("Table", "S A C M E gamma newf elo")
METHOD_NAMES = {1: "ros2", 2: "ros3", 3: "ros4", 4: "rodas3", 5: "rodas4"}


def table(method):
    """ros_S, ros_A, ros_C, ros_M, ros_E, ros_Gamma, ros_NewF, ros_ELO as Ros2_x .. Rodas4_x set them (values typed in as data; Ros2's formed from
    g with the reference's expressions); method = IPAR(4), 0 = Ros4 (gas.f:1057-1077)"""
    if method in (0, 3):
        a = (0.2000000000000000e+01, 0.1867943637803922e+01, 0.2344449711399156e+00)
        return Table(4, a + (a[1], a[2], 0.0),
                     (-0.7137615036412310e+01, 0.2580708087951457e+01, 0.6515950076447975e+00, -0.2137148994382534e+01, -0.3214669691237626e+00,
                      -0.6949742501781779e+00),
                     (0.2255570073418735e+01, 0.2870493262186792e+00, 0.4353179431840180e+00, 0.1093502252409163e+01),
                     (-0.2815431932141155e+00, -0.7276199124938920e-01, -0.1082196201495311e+00, -0.1093502252409163e+01),
                     (0.5728200000000000e+00, -0.1769193891319233e+01, 0.7592633437920482e+00, -0.1049021087100450e+00),
                     (True, True, True, False), 4.0)
    if method == 1:
        g = 1.0 + 1.0 / math.sqrt(2.0)
        return Table(2, ((1.0) / g,), ((-2.0) / g,), ((3.0) / (2.0 * g), (1.0) / (2.0 * g)), (1.0 / (2.0 * g), 1.0 / (2.0 * g)), (g, -g), (True, True), 2.0)
    if method == 2:
        return Table(3, (1.0, 1.0, 0.0), R.ROS_C, R.ROS_M, R.ROS_E, R.ROS_GAMMA, (True, True, False), R.ROS_ELO)
    if method == 4:
        return Table(4, (0.0, 2.0, 0.0, 2.0, 0.0, 1.0), (4.0, 1.0, -1.0, 1.0, -1.0, -(8.0 / 3.0)), (2.0, 0.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0),
                     (0.5, 1.5, 0.0, 0.0), (True, False, True, True), 3.0)
    if method == 5:
        a = (0.1544000000000000e+01, 0.9466785280815826e+00, 0.2557011698983284e+00, 0.3314825187068521e+01, 0.2896124015972201e+01,
             0.9986419139977817e+00, 0.1221224509226641e+01, 0.6019134481288629e+01, 0.1253708332932087e+02, -0.6878860361058950e+00)
        return Table(6, a + a[6:10] + (1.0,),
                     (-0.5668800000000000e+01, -0.2430093356833875e+01, -0.2063599157091915e+00, -0.1073529058151375e+00, -0.9594562251023355e+01,
                      -0.2047028614809616e+02, 0.7496443313967647e+01, -0.1024680431464352e+02, -0.3399990352819905e+02, 0.1170890893206160e+02,
                      0.8083246795921522e+01, -0.7981132988064893e+01, -0.3152159432874371e+02, 0.1631930543123136e+02, -0.6058818238834054e+01),
                     a[6:10] + (1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0, 1.0),
                     (0.2500000000000000e+00, -0.1043000000000000e+00, 0.1035000000000000e+00, -0.3620000000000023e-01, 0.0, 0.0),
                     (True,) * 6, 4.0)
    raise KeyError(method)


# ---- the sets: name -> (IPAR, RPAR, AbsTol, RelTol, Tstart, Tend)
BASE_SETS = tuple("m%d" % m for m in (0, 1, 3, 4, 5))                                   # the methods at INTEGRATE_x's other options
AUTONOMOUS_SETS = tuple(n + "_autonomous" for n in BASE_SETS)                         # ... with IPAR(1) = 1
OPTION_SETS = tuple("m%d_%s" % (m, o) for m in (4, 5) for o in ("vector_tol", "rtol_1e-5", "hmax_0.5", "max_steps_5"))      # methods meet the other options
BACKWARD_SETS = ("m4_backward",)                                                      # 10 -> 0 s: the sign of Direction*H*Gamma flips
REFUSED_SETS = ("m3_rpar1_-1",)                                                       # a refusal is not a method matter
REFUSED_IERR = {"m3_rpar1_-1": -3}
RUN_SETS = BASE_SETS + AUTONOMOUS_SETS + OPTION_SETS + BACKWARD_SETS
SET_NAMES = RUN_SETS + REFUSED_SETS


def method_set(mech, name):
    head, _, rest = name.partition("_")
    method = int(head[1:])
    tstart, tend = TIN, TOUT
    if rest in ("", "autonomous", "backward"):
        ipar, rpar, atol, rtol = R.base_options(mech)
        if rest == "autonomous":
            ipar[0] = 1
        if rest == "backward":
            tstart, tend = TOUT, TIN
    elif name in REFUSED_SETS:
        ipar, rpar, atol, rtol = R.refused_set(mech, rest)
    else:
        ipar, rpar, atol, rtol = R.option_set(mech, rest)
    ipar[3] = method
    return ipar, rpar, atol, rtol, tstart, tend


def method_of(name):
    m = int(name.partition("_")[0][1:])
    return 3 if m == 0 else m


# ---- the restatement
def rosenbrock(o, diag, var, fix, rconst, ipar, rpar, atol, rtol, tstart=TIN, tend=TOUT):
    """Rosenbrock_x on one cell with oracle `o` (oracle.Oracle) and the mechanism's LU_DIAG (0-based) -> (VAR, IERR, IPAR(11:18), Texit, Hexit), any
    of the five methods.  A refusal returns VAR untouched, zero counters and Texit = Hexit = 0."""
    y = np.array(var, np.float64)
    st = np.zeros(8, np.int32)         # Nfun Njac Nstp Nacc Nrej Ndec Nsol Nsng
    ierr, p = resolve(ipar, rpar, atol, rtol, len(y), tstart, tend)
    if ierr != 1:
        return y, ierr, st, 0.0, 0.0
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

    def waxpy(alpha, x, yy):           # WAXPY_x (gas.f:6641): returns at once for a zero coefficient
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
                    return y, -8, st, t, hexit
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


def restated(mech, golden, variant=0, names=SET_NAMES):
    """{set name: (VAR [3, NVAR], IERR [3], IPAR(11:18) [3, 8], Texit [3], Hexit [3])} of the restatement on the three cells of the golden set, for one
    oracle variant (oracle.set_variant); computed once per (mechanism, variant, set) and shared by the tests"""
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
                rows = [rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *method_set(mech, name)) for c in cells_of(g["var_in"].shape[0])]
            finally:
                set_variant(0)
            _restated[key] = tuple(np.array([r[i] for r in rows]) for i in range(5))
        out[name] = _restated[key]
    return out
