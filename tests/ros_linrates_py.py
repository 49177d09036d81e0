"""TEST INFRASTRUCTURE — a series of Rosenbrock_x calls with rate constants LINEAR IN TIME over each leg (mistra_chem_rosenbrock_series_linrates_ex;
INTEGRATION.md section 4s) restated on the CPU: tests/ros_methods_py.py's step loop with R(tau), dR/dt and ros_Alpha, chained by tests/ros_series_py.py's
chain, the node blocks and the sets the tests run.

The definition, per cell, reaction r and leg k (times[k] -> times[k+1]), every operation rounded on its own (numpy does that by itself):
    w = 1.0 / (times[k+1] - times[k])      d = R[k+1] - R[k]      R(tau) = R[k] + ((tau - times[k]) * w) * d      dR/dt = d * w
Fcn0 and Jac0 read R(T); a stage that evaluates anew reads R(T + ros_Alpha(i)*Direction*H); with IPAR(1) = 0 dFdT = Fun(Y, FIX, dR/dt), counted as
ros_FunTimeDerivative_x's Fun call, and every stage with ros_Gamma(i) /= 0 adds (Direction*H*ros_Gamma(i))*dFdT; with IPAR(1) /= 0 neither.

There is no compiled reference for this (KPP's FunTemplate_x ignores T): the restatement IS the definition.  It is pinned to the one that is pinned to
the compiled Rosenbrock_x: with equal node blocks it equals tests/ros_series_rates_py.py's chain on the shared block bit for bit
(tests/test_ros_linrates.py)."""
import math

import numpy as np

import ros_methods_py as RM
import ros_options_py as R
import ros_series_py as RS
import ros_series_rates_py as SR
from ros_options_py import DELTA_MIN, MECHS, NVAR, ROUNDOFF, error_norm, fmax_f, fmin_f, resolve  # noqa: F401

TIMES = SR.TIMES                          # (0, 2.5, 5, 7.5, 10)
W_NODES = (0.0, 0.25, 0.5, 0.75, 1.0)     # node k of the dawn: (1 - w)*night + w*day at times[k]
# ros_Alpha of Ros2_x .. Rodas4_x, typed in as data (IPAR(4) -> the stages' abscissae)
ALPHA = {1: (0.0, 1.0),
         2: (0.0, 0.43586652150845899941601945119356e+00, 0.43586652150845899941601945119356e+00),
         3: (0.0, 0.1145640000000000e+01, 0.6552168638155900e+00, 0.6552168638155900e+00),
         4: (0.0, 0.0, 1.0, 1.0),
         5: (0.0, 0.386, 0.21, 0.63, 1.0, 1.0)}

METHOD_SETS = tuple("m%d" % m for m in (1, 2, 3, 4, 5))      # m<IPAR(4)>: every method, IPAR(1) = 0; m2 is Ros3
SET_NAMES = METHOD_SETS + ("ros3_carry", "ros3_fix_per_leg", "ros3_equal_nodes", "rodas4_equal_nodes", "ros3_descending")
GAS_ONLY_SETS = ("ros3_autonomous_flag",)                    # IPAR(1) = 1: the rates still move, the HG*dFdT terms are not added
EQUAL_SETS = ("ros3_equal_nodes", "rodas4_equal_nodes")
FAILING_IERR = {"ros3_descending": -7}                       # backward in time the chemistry is unstable: the step size underflows in every leg


def set_names(mech):
    return SET_NAMES + (GAS_ONLY_SETS if mech == "gas" else ())


def series_set(mech, name):
    """-> (ros_series_py.Series, FIX by leg?, equal node blocks?, descending?)"""
    ipar, rpar, atol, rtol = R.base_options(mech)
    carry = per_f = equal = down = False
    if name in METHOD_SETS:
        ipar[3] = int(name[1:])
    elif name == "ros3_carry":
        carry = True
    elif name == "ros3_fix_per_leg":
        per_f = True
    elif name == "ros3_equal_nodes":
        equal = True
    elif name == "rodas4_equal_nodes":
        equal = True
        ipar[3] = 5
    elif name == "ros3_descending":
        down = True
    elif name == "ros3_autonomous_flag":
        ipar[0] = 1
    else:
        raise KeyError(name)
    times = np.array(TIMES[::-1] if down else TIMES, np.float64)
    return RS.Series(ipar, rpar, atol, rtol, times, carry), per_f, equal, down


def nodes(mech):
    """-> (VAR [3, NVAR], leg FIX [4, 3, NFIX], node RCONST [5, 3, NREACT]): ros_series_rates_py.ramp()'s cells and FIX rows, the rate constants as five
    node blocks at W_NODES"""
    g = np.load(SR.GOLDEN + "/integrate_%s.npz" % mech)
    d = np.load(SR.GOLDEN + "/integrate_%s_day.npz" % mech)
    c, cd = list(R.cells_of(g["var_in"].shape[0])), list(R.cells_of(d["var_in"].shape[0]))
    V, LF, _ = SR.ramp(mech)
    return V, LF, SR.blend(g["rconst"][c], d["rconst"][cd], W_NODES)


def set_rows(mech, name, rows=None):
    """the arrays a set hands to the entry -> (Series, VAR [3, NVAR], fix [4, 3, NFIX] or [3, NFIX], rconst_nodes [5, 3, NREACT])"""
    V, LF, NK = nodes(mech) if rows is None else rows
    s, per_f, equal, down = series_set(mech, name)
    if equal:
        NK = np.stack([NK[0]] * NK.shape[0])
    if down:
        NK, LF = NK[::-1].copy(), LF[::-1].copy()
    return s, V, (LF if per_f else LF[0]), NK


def rate_at(k0, d, t0, w, tau):
    """R(tau) of one leg, as the definition rounds it"""
    return k0 + ((tau - t0) * w) * d


def rosenbrock(o, diag, var, fix, k0, k1, ipar, rpar, atol, rtol, tstart, tend):
    """ros_methods_py.rosenbrock with the rate constants linear from k0 at tstart to k1 at tend -> (VAR, IERR, IPAR(11:18), Texit, Hexit)"""
    y = np.array(var, np.float64)
    st = np.zeros(8, np.int32)
    ierr, p = resolve(ipar, rpar, atol, rtol, len(y), tstart, tend)
    if ierr != 1:
        return y, ierr, st, 0.0, 0.0
    tb, alpha = RM.table(p["method"]), ALPHA[p["method"]]
    autonomous, vector = p["autonomous"], p["vector"]
    hmin, hmax = p["hmin"], p["hmax"]
    w = 1.0 / (tend - tstart)
    d = np.asarray(k1, np.float64) - np.asarray(k0, np.float64)
    kdot = d * w
    t, hexit = tstart, 0.0
    h = fmin_f(p["hstart"], hmax)
    if abs(h) <= 10.0 * ROUNDOFF:
        h = DELTA_MIN
    direction = 1.0 if tend >= tstart else -1.0
    reject_last = reject_more = False
    n = len(y)

    def waxpy(a, x, yy):
        return yy if a == 0.0 else yy + a * x

    while abs(tend - t) >= ROUNDOFF:
        if st[2] > p["max_steps"]:
            return y, -6, st, t, hexit
        if (t + 0.1 * h) == t or h <= ROUNDOFF:
            return y, -7, st, t, hexit
        hexit = h
        h = fmin_f(h, abs(tend - t))
        k_t = rate_at(k0, d, tstart, w, t)
        fcn0 = o.fun(y, fix, k_t)
        st[0] += 1
        if not autonomous:             # in the place of ros_FunTimeDerivative_x: the exact derivative, one Fun call
            dfdt = o.fun(y, fix, kdot)
            st[0] += 1
        jac0 = o.jac_sp(y, fix, k_t)
        st[1] += 1
        while True:
            nconsecutive = 0
            while True:
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
            for istage in range(tb.S):
                row = istage * (istage - 1) // 2
                if istage >= 1 and tb.newf[istage]:
                    ynew = y.copy()
                    for j in range(istage):
                        ynew = waxpy(tb.A[row + j], k[j], ynew)
                    tau = t + alpha[istage] * (direction * h)
                    fcn = o.fun(ynew, fix, rate_at(k0, d, tstart, w, tau))
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


def chain_cell(o, diag, s, var, fix, node_k):
    """one cell through the legs of `s`: fix [nleg, NFIX] or [NFIX], node_k [nleg + 1, NREACT] -> ros_series_py.chain's tuple"""
    leg = iter(range(len(s.times) - 1))

    def one(y, rpar, t0, t1):
        k = next(leg)
        return rosenbrock(o, diag, y, fix[k] if fix.ndim == 2 else fix, node_k[k], node_k[k + 1], s.ipar, rpar, s.atol, s.rtol, t0, t1)
    return RS.chain(one, var, s)


def chain_cells(mech, s, V, F, NK, variant=0):
    """every cell of V through chain_cell -> (VAR [nleg, ncell, NVAR], IERR [nleg, ncell], IPAR(11:18) [nleg, ncell, 8], Texit, Hexit [nleg, ncell])"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    o, diag = Oracle(mech), mechtab.load(mech).diag
    try:
        set_variant(variant)
        cells = [chain_cell(o, diag, s, V[c], F[:, c] if F.ndim == 3 else F[c], NK[:, c]) for c in range(V.shape[0])]
    finally:
        set_variant(0)
    return tuple(np.stack([cell[i] for cell in cells], axis=1) for i in range(5))


_restated, _rows = {}, {}


def restated(mech, variant=0, names=None):
    """{set name: chain_cells' tuple} on the three cells of nodes(mech), for one oracle variant; computed once per (mechanism, variant, set) and shared
    by the tests"""
    out = {}
    for name in set_names(mech) if names is None else names:
        key = (mech, variant, name)
        if key not in _restated:
            if mech not in _rows:
                _rows[mech] = nodes(mech)
            s, V, F, NK = set_rows(mech, name, _rows[mech])
            _restated[key] = chain_cells(mech, s, V, F, NK, variant)
        out[name] = _restated[key]
    return out
