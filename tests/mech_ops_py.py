"""The operators (mistra_chem_ops_ex / _device) restated on the oracle's exported primitives, as tests/ros_options_py.py restates
Rosenbrock_x on them: nothing here looks at the kernel.

    vdot = Oracle.fun(V, F, RCT)                    jvs = Oracle.jac_sp(V, F, RCT)
    A    = (-jvs) with shift added ONCE on the diagonal slots (ros_PrepareMatrix_x's Ghimj for shift = 1/(Direction*H*gamma), gas.f:1404)
    LU, ising = Oracle.decomp(A)                    x_j = Oracle.solve(LU, b_j); ising > 0: no factorisation is used, every x_j = +0.0

and the yardstick of the solves: the row-wise backward error, formed in long double from A,

    omega = max_i |b - A x|_i / (||A_i||_1 * ||x||_inf + |b_i|)

(rows whose denominator is zero have a zero residual and are left out)."""
import os

import numpy as np

from conftest import REPO

GAMMA1 = 0.43586652150845899941601945119356      # Ros3_x (gas.f:1596-1626)
COLUMN = os.path.join(REPO, "tests", "golden", "column_BTZ96.npz")


def column_cells(mech):
    """every captured cell of the BTZ96 column: 68 gas, 31 aer, 49 tot -> (V, F, RCT)"""
    z = np.load(COLUMN)
    return z[mech + "_var_in"], z[mech + "_fix"], z[mech + "_rconst"]


def pattern(mech):
    """(crow, icol, diag), 0-based, of the mechanism's table"""
    from mistra_amd import mechtab
    t = mechtab.load(mech)
    return np.asarray(t.crow, np.int64), np.asarray(t.icol, np.int64), np.asarray(t.diag, np.int64)


def prepared(jvs, diag, shift):
    """jvs -> A = shift*I - J: the single operation (-jvs), then shift added once on the diagonal slots"""
    a = -np.asarray(jvs, np.float64)
    a[diag] = a[diag] + np.float64(shift)
    return a


def ops(oracle, diag, V, F, RCT, shift=None, rhs=(), fun_rhs=False):
    """one cell -> (vdot, jvs, A or None, x [fun_rhs + len(rhs), NVAR] or None, ising or None)"""
    vdot = oracle.fun(V, F, RCT)
    jvs = oracle.jac_sp(V, F, RCT)
    if shift is None:
        return vdot, jvs, None, None, None
    a = prepared(jvs, diag, shift)
    lu, ising = oracle.decomp(a)
    rows = ([vdot + 0.0] if fun_rhs else []) + [np.asarray(b, np.float64) for b in rhs]
    if ising:
        return vdot, jvs, a, np.zeros((len(rows), vdot.size)), ising
    return vdot, jvs, a, np.array([oracle.solve(lu, b) for b in rows]).reshape(len(rows), vdot.size), 0


def backward_error(a, crow, icol, x, b):
    """the row-wise backward error of A x = b, residual and sums in long double"""
    ld = np.longdouble
    a, x, b = np.asarray(a, ld), np.asarray(x, ld), np.asarray(b, ld)
    n = b.size
    row = np.repeat(np.arange(n), np.diff(crow))
    ax = np.zeros(n, ld)
    np.add.at(ax, row, a * x[icol])
    norm1 = np.zeros(n, ld)
    np.add.at(norm1, row, np.abs(a))
    den = norm1 * np.abs(x).max() + np.abs(b)
    res = np.abs(b - ax)
    ok = den > 0
    assert np.all(res[~ok] == 0)
    return float((res[ok] / den[ok]).max()) if ok.any() else 0.0
