#!/usr/bin/env python3
"""Which reactions produce and destroy a species DURING a call of Rosenbrock_x, from the reaction flux of the integrator
(mistra_chem_rosenbrock_flux_ex, include/mistra_chem.h).

    python tools/reaction_budget.py tot --golden tests/golden/column_BTZ96.npz --controlling          the species that controlled the most attempts
    python tools/reaction_budget.py tot --golden tests/golden/column_BTZ96.npz --species 12,40        species 12 and 40 (numbered as in VAR, 1-based)
    ... --method 4                                                                                    IPAR(4): 1 Ros2, 2 Ros3 (default), 3 Ros4, 4 Rodas3, 5 Rodas4
    ... --atol-rel 1e-13                                                                              AbsTol = 1e-13 x the cell's largest concentration, per cell
    ... --cells 0:4   --top 8   --tstart 0 --tend 10
    ... --cpu                                                                                         the Python restatement (tests/ros_flux_py.py) instead of the GPU

flux[r] is the integral of reaction r's rate over the call (trapezoid rule on the accepted states), so S(i,r) * flux[r] is what reaction r added to
species i.  Per chosen species, summed over the cells of the batch: the largest producing and destroying reactions with their S(i,r) * flux[r], the
gross turnover sum_r |S(i,r) * flux[r]|, the net change sum_r S(i,r) * flux[r] beside Y(Texit) - Y(Tstart), the ratio gross / |net| (its median over
the cells too: a species in fast equilibrium has gross >> net), and for every listed reaction the figure the reference's budget rule gives: the rate at
the END state times the interval.  Reactions are numbered as in RCONST (1-based).

--controlling picks the species from a Ros3 step-control trace of the same cells at the same tolerances (tools/step_control.py).
Nothing is asserted on the output: these are properties of the chemistry and of the reference algorithm at the run's tolerances."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import step_control as SC      # noqa: E402


def run_flux(mech, var, fix, rconst, tstart, tend, opts, cpu, atol_rel=None):
    """-> (var_out, ierr, stats, flux) of the batch: one call of the flux entry (per-cell AbsTol rows with atol_rel), or the restatement cell by cell"""
    ipar, rpar, atol, rtol = opts
    rows = None if atol_rel is None else SC.cell_atol_rows(mech, var, atol_rel)
    if not cpu:
        from mistra_amd import chem
        if rows is None:
            res, _, flux = chem.rosenbrock_flux(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol)
        else:
            res, _, flux = chem.rosenbrock_flux_cells(mech, var, fix, rconst, tstart, tend, ipar, rpar, rows, np.full_like(rows, rtol[0]))
        return res.var, res.ierr, res.stats, flux
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_flux_py as RF
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    out = []
    for c in range(var.shape[0]):
        at = atol if rows is None else np.full_like(atol, rows[c, 0])
        out.append(RF.rosenbrock(o, diag, var[c], fix[c], rconst[c], ipar, rpar, at, rtol, tstart, tend))
    return (np.array([r[0] for r in out]), np.array([r[1] for r in out], np.int32), np.array([r[2] for r in out]), np.array([r[5] for r in out]))


def controlling_species(mech, var, fix, rconst, tstart, tend, atol_rel, cpu, count):
    """the `count` species that controlled the most attempts of a Ros3 trace of the same cells (1-based)"""
    opts = SC.options(mech)
    trace = SC.trace_cpu if cpu else SC.trace_gpu
    _, rows = trace(mech, var, fix, rconst, tstart, tend, opts, 4096, atol_rel)
    hits = np.zeros(var.shape[1] + 1, np.int64)
    for species, _, _ in rows:
        hits += np.bincount(species, minlength=hits.size)
    hits[0] = 0
    order = np.argsort(-hits, kind="stable")[:count]
    return [int(s) for s in order if hits[s] > 0], hits


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mech", choices=SC.MECHS)
    ap.add_argument("--golden", required=True)
    ap.add_argument("--cells")
    ap.add_argument("--method", type=int, default=2)
    ap.add_argument("--atol-rel", type=float)
    ap.add_argument("--species")
    ap.add_argument("--controlling", action="store_true")
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--tstart", type=float, default=0.0)
    ap.add_argument("--tend", type=float, default=10.0)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args(argv)
    if bool(a.species) == a.controlling:
        raise SystemExit("one of --species i,j and --controlling")
    from mistra_amd import mechtab
    var, fix, rconst = SC.load_cells(a.mech, a.golden, None, a.cells)
    n, dt = var.shape[0], a.tend - a.tstart
    print("%s, %d cells of %s, %g -> %g s, method %d, AbsTol %s%s" %
          (a.mech, n, os.path.basename(a.golden), a.tstart, a.tend, a.method,
           "1e-25" if a.atol_rel is None else "%g x the cell maximum" % a.atol_rel, ", CPU restatement" if a.cpu else ""))
    if a.controlling:
        chosen, hits = controlling_species(a.mech, var, fix, rconst, a.tstart, a.tend, a.atol_rel, a.cpu, 3)
        print("controlling species of the Ros3 trace (attempts controlled): " + ", ".join("%d (%d)" % (s, hits[s]) for s in chosen))
    else:
        chosen = [int(x) for x in a.species.split(",")]
    opts = SC.options(a.mech)
    opts[0][3] = a.method
    out, ierr, stats, flux = run_flux(a.mech, var, fix, rconst, a.tstart, a.tend, opts, a.cpu, a.atol_rel)
    print("IERR %s; attempts per cell: mean %.1f, max %d" % (sorted(set(int(x) for x in ierr)), stats[:, 2].mean(), stats[:, 2].max()))
    t = mechtab.load(a.mech)
    S = t.stoich()
    a_end = np.array([t.products(out[c], fix[c], rconst[c]) for c in range(n)])
    cmax = np.maximum(np.abs(var), np.abs(out)).max(axis=1)
    for sp in chosen:
        i = sp - 1
        per = flux * S[i]                      # [ncell, NREACT]: what reaction r added to the species in each cell
        end = a_end * S[i] * dt                # the end-state x dt figure
        tot, gross, net = per.sum(axis=0), np.abs(per).sum(), per.sum()
        dy = (out[:, i] - var[:, i]).sum()
        cell_net = np.abs(per.sum(axis=1))
        ratio = np.abs(per).sum(axis=1) / np.where(cell_net > 0, cell_net, np.nan)
        conc = np.median(np.maximum(np.abs(var[:, i]), np.abs(out[:, i])) / cmax)
        print("\nspecies %d: median concentration %.2e of the cell maximum" % (sp, conc))
        print("  gross turnover %.4e   net change %.4e (Y(Texit) - Y(Tstart): %.4e)   gross / |net| %.3e (median over the cells %.3e)" %
              (gross, net, dy, gross / abs(net) if net != 0 else float("inf"), float(np.nanmedian(ratio)) if np.isfinite(ratio).any() else float("inf")))
        for title, order in (("producing", np.argsort(-tot)), ("destroying", np.argsort(tot))):
            print("  %-10s %8s %14s %10s %18s" % (title, "reaction", "S*flux", "of gross", "end state x dt"))
            for r in order[:a.top]:
                if (tot[r] <= 0) if title == "producing" else (tot[r] >= 0):
                    break
                print("  %-10s %8d %14.4e %9.1f%% %18.4e" % ("", r + 1, tot[r], 100.0 * abs(tot[r]) / gross, end[:, r].sum()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
