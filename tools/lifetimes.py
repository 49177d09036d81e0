#!/usr/bin/env python3
"""Chemical lifetimes of species beside the integrator's step sizes, from the Jacobian the operators hand out (mistra_chem_ops_ex, include/mistra_chem.h;
INTEGRATION.md §4p).

    python tools/lifetimes.py tot --golden tests/golden/column_BTZ96.npz --species 80 206 207      the species named (1-based, as in VAR)
    python tools/lifetimes.py tot --golden tests/golden/column_BTZ96.npz --controlling             the species that controlled the most attempts of a Ros3 trace
    ... --cpu                                                                                      J from a numpy restatement of Jac_SP_x's diagonal and the trace
                                                                                                   from the Python restatement (tests/ros_trace_py.py): no GPU

Per chosen species, over the cells of the batch: the lifetime -1/J(i,i) at the state the call receives as minimum, median and maximum (a species whose
J(i,i) is >= 0 in a cell has no lifetime there: counted, left out of the three); the same beside the accepted step sizes of a Ros3 trace of those cells
with INTEGRATE_x's options (smallest, median and largest accepted H over all cells); and the species' largest off-diagonal couplings |J(i,j)| of the median
cell, as the ratio to |J(i,i)|.  Nothing is asserted on the figures: they are properties of the mechanism at those states."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import step_control as SC  # noqa: E402


def jacobian_cpu(mech, var, fix, rconst):
    """jvs [ncell, LU_NONZERO] restated in numpy from the mechanism's table: B(m) = RCT(b_rct[m]) * prod X[b_fac], JVS(k) = sum jv_coef * B(jv_idx)"""
    from mistra_amd import mechtab
    t = mechtab.load(mech)
    x = np.concatenate([var, fix, np.broadcast_to(t.consts, (var.shape[0], t.nconst))], axis=1)
    b = rconst[:, t.b_rct].copy()
    owner = np.repeat(np.arange(t.nb), np.diff(t.b_ptr))
    for m, f in zip(owner, t.b_fac):
        b[:, m] = b[:, m] * x[:, f]
    jvs = np.zeros((var.shape[0], t.nnz))
    slot = np.repeat(np.arange(t.nnz), np.diff(t.jv_ptr))
    np.add.at(jvs, (slice(None), slot), t.jv_coef * b[:, t.jv_idx])
    return jvs


def accepted_steps(mech, var, fix, rconst, cpu, cap=4096):
    """-> (accepted step sizes of all cells, attempts each species controlled) of a Ros3 trace 0 -> 10 s with INTEGRATE_x's options"""
    opts = SC.options(mech)
    hs, ctrl = [], np.zeros(var.shape[1], np.int64)
    if cpu:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import ros_trace_py as RT
        from mistra_amd import mechtab
        from oracle.oracle import Oracle
        o, diag = Oracle(mech), mechtab.load(mech).diag
        for c in range(var.shape[0]):
            tr = RT.rosenbrock_trace(o, diag, var[c], fix[c], rconst[c], *opts, tstart=0.0, tend=10.0)[5]
            code, h, sp = np.asarray(tr.code), np.asarray(tr.h), np.asarray(tr.species)
            hs.append(h[(code & 1) == 1])
            np.add.at(ctrl, sp[sp > 0] - 1, 1)
    else:
        from mistra_amd import chem
        _, _, tr = chem.rosenbrock_trace(mech, var, fix, rconst, 0.0, 10.0, *opts, cap=cap, ctrl=False)
        for c in range(var.shape[0]):
            k = min(int(tr.n[c]), cap)
            hs.append(tr.h[c, :k][(tr.code[c, :k] & 1) == 1])
            sp = tr.species[c, :k]
            np.add.at(ctrl, sp[sp > 0] - 1, 1)
    return np.concatenate(hs), ctrl


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mech", choices=SC.MECHS)
    ap.add_argument("--golden", required=True)
    ap.add_argument("--cells", help="lo:hi slice of the file's cells")
    ap.add_argument("--species", type=int, nargs="+", help="1-based species numbers")
    ap.add_argument("--controlling", action="store_true", help="the five species that controlled the most attempts of the trace")
    ap.add_argument("--couplings", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    if not a.species and not a.controlling:
        ap.error("--species or --controlling")
    var, fix, rconst = SC.load_cells(a.mech, a.golden, cells=a.cells)
    from mistra_amd import mechtab
    t = mechtab.load(a.mech)
    if a.cpu:
        jvs = jacobian_cpu(a.mech, var, fix, rconst)
    else:
        from mistra_amd import chem
        jvs = chem.jac_sp(a.mech, var, fix, rconst)
    h_acc, ctrl = accepted_steps(a.mech, var, fix, rconst, a.cpu)
    species = list(a.species or [])
    if a.controlling:
        species += [int(s) + 1 for s in np.argsort(-ctrl, kind="stable")[:5] if ctrl[s] > 0 and int(s) + 1 not in species]
    print("%s: %d cells of %s, J from %s" % (a.mech, var.shape[0], os.path.basename(a.golden), "the numpy restatement" if a.cpu else "mistra_chem_ops_ex"))
    print("accepted steps of the Ros3 trace (INTEGRATE_x's options, 0 -> 10 s): %d, H min %.3e  median %.3e  max %.3e s" %
          (h_acc.size, h_acc.min(), np.median(h_acc), h_acc.max()))
    print("%-8s %-10s %-34s %-22s %-10s %s" % ("species", "attempts", "lifetime -1/J(i,i) [s]", "median lifetime over", "cells with", "largest couplings of the median cell"))
    print("%-8s %-10s %-10s %-11s %-11s %-10s %-11s %-10s %s" % ("", "controlled", "min", "median", "max", "min H", "median H", "J(i,i)>=0", "|J(i,j)| / |J(i,i)|: j"))
    for s in species:
        i = s - 1
        d = jvs[:, t.diag[i]]
        neg = d < 0
        if not neg.any():
            print("%-8d %-10d no cell with J(i,i) < 0" % (s, ctrl[i]))
            continue
        tau = -1.0 / d[neg]
        med = float(np.median(tau))
        c = np.flatnonzero(neg)[np.argsort(tau, kind="stable")[tau.size // 2]]
        cols = t.icol[t.crow[i]:t.crow[i + 1]]
        vals = np.abs(jvs[c, t.crow[i]:t.crow[i + 1]])
        off = cols != i
        order = np.argsort(-vals[off], kind="stable")[:a.couplings]
        coup = "  ".join("%.2e: %d" % (vals[off][k] / abs(d[c]), cols[off][k] + 1) for k in order if vals[off][k] > 0)
        print("%-8d %-10d %-10.3e %-11.3e %-11.3e %-10.3e %-11.3e %-10d %s" %
              (s, ctrl[i], tau.min(), med, tau.max(), med / h_acc.min(), med / np.median(h_acc), int((~neg).sum()), coup))


if __name__ == "__main__":
    main()
