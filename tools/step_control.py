#!/usr/bin/env python3
"""Which species control the step size of Rosenbrock_x (Ros3) on a batch of cells, from the step-control trace of the integrator
(mistra_chem_rosenbrock_trace_ex, include/mistra_chem.h).

    python tools/step_control.py tot --golden tests/golden/column_BTZ96.npz                 the tot cells of a captured column step, INTEGRATE_x's options
    python tools/step_control.py tot --golden tests/golden/column_BTZ96.npz --atol 1e-15     ... with a scalar AbsTol
    python tools/step_control.py tot --golden tests/golden/integrate_tot.npz --atol-rel 1e-13    AbsTol = 1e-13 x the cell's largest concentration (one call per cell)
    python tools/step_control.py aer --workload 4096                                         cells 0 .. 4095 of the synthetic workload (mistra_amd/workload.py)
    ... --cpu                                                                                the Python restatement (tests/ros_trace_py.py) instead of the GPU

Prints the attempts per cell and, for the species that controlled the most attempts (the species with the largest term of ros_ErrorNorm_x's sum):
the attempts it controlled, how many of those were rejected, in how many cells, and the median over those cells of its concentration relative to the
cell's largest — the concentration being max(|VAR in|, |VAR out|) of the call.  Species are numbered as in VAR (1-based); --names FILE (one name per
line, in that order) prints names, the mechanism tables carry none."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MECHS = ("gas", "aer", "tot")


def load_cells(mech, golden=None, workload=None, cells=None):
    """-> (var, fix, rconst) numpy arrays of the batch: a golden file (integrate_<mech>.npz: var_in / fix / rconst; column_* / drivecol_*:
    <mech>_var_in / ...) or the first `workload` cells of the synthetic workload"""
    if golden:
        z = np.load(golden)
        pre = mech + "_" if mech + "_var_in" in z.files else ""
        if pre + "var_in" not in z.files:
            raise SystemExit("%s holds no cells of the %s mechanism" % (golden, mech))
        var, fix, rconst = z[pre + "var_in"], z[pre + "fix"], z[pre + "rconst"]
    else:
        import torch
        from mistra_amd import workload as W
        var, fix, rconst = (x.numpy() for x in W.make_batch(mech, 0, int(workload), torch.device("cpu")))
    if cells:
        lo, _, hi = cells.partition(":")
        sl = slice(int(lo) if lo else None, int(hi) if hi else None)
        var, fix, rconst = var[sl], fix[sl], rconst[sl]
    return np.ascontiguousarray(var), np.ascontiguousarray(fix), np.ascontiguousarray(rconst)


def options(mech, atol=None, rtol=None):
    """INTEGRATE_x's IPAR, RPAR (gas.f:739-746) with scalar tolerances"""
    from mistra_amd import chem
    nvar = chem.DIMS[mech][0]
    ipar, rpar = np.zeros(20, np.int32), np.zeros(20)
    ipar[1], ipar[3] = 1, 2
    rpar[2] = 1.0e-3
    return ipar, rpar, np.full(nvar, 1.0e-25 if atol is None else float(atol)), np.full(nvar, 1.0e-3 if rtol is None else float(rtol))


def trace_gpu(mech, var, fix, rconst, tstart, tend, opts_of_cell, cap):
    """-> (var_out, [(species, code, n) per cell]) from the kernel; opts_of_cell(c) -> (ipar, rpar, atol, rtol), or None: one set for the batch"""
    from mistra_amd import chem
    n = var.shape[0]
    if callable(opts_of_cell):
        groups = [(slice(c, c + 1), opts_of_cell(c)) for c in range(n)]
    else:
        groups = [(slice(0, n), opts_of_cell)]
    out, rows = np.empty_like(var), []
    for sl, o in groups:
        res, _, tr = chem.rosenbrock_trace(mech, var[sl], fix[sl], rconst[sl], tstart, tend, *o, cap=cap, ctrl=False)
        out[sl] = res.var
        for c in range(res.var.shape[0]):
            k = min(int(tr.n[c]), cap)
            rows.append((tr.species[c, :k].copy(), tr.code[c, :k].copy(), int(tr.n[c])))
    return out, rows


def trace_cpu(mech, var, fix, rconst, tstart, tend, opts_of_cell, cap):
    """the same from the restatement (tests/ros_trace_py.py over the C oracle)"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_trace_py as RT
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    out, rows = np.empty_like(var), []
    for c in range(var.shape[0]):
        opt = opts_of_cell(c) if callable(opts_of_cell) else opts_of_cell
        r = RT.rosenbrock_trace(o, diag, var[c], fix[c], rconst[c], *opt, tstart=tstart, tend=tend)
        out[c] = r[0]
        tr = r[5]
        rows.append((tr.species[:cap].copy(), tr.code[:cap].copy(), len(tr.species)))
    return out, rows


def control_table(var_in, var_out, rows, top=8):
    """rows: (species [k], code [k], n) per cell (k = records kept, n = attempts made) -> dict: attempts per cell, records kept, rejected records, and
    `species`: for the `top` species that controlled the most kept attempts (ties: the lower number first), (species, controlled, rejected, cells,
    median over those cells of max(|VAR in|, |VAR out|)[species] / the cell's largest)"""
    conc = np.maximum(np.abs(np.asarray(var_in, np.float64)), np.abs(np.asarray(var_out, np.float64)))
    nvar = conc.shape[1]
    controlled, rejected = np.zeros(nvar + 1, np.int64), np.zeros(nvar + 1, np.int64)
    cells_of = [[] for _ in range(nvar + 1)]
    kept = rej_total = 0
    for c, (species, code, _) in enumerate(rows):
        species, code = np.asarray(species, np.int64), np.asarray(code, np.int64)
        kept += len(species)
        rej = (code & 1) == 0
        rej_total += int(rej.sum())
        controlled += np.bincount(species, minlength=nvar + 1)
        rejected += np.bincount(species[rej], minlength=nvar + 1)
        for s in np.unique(species):
            cells_of[s].append(c)
    order = sorted((s for s in range(1, nvar + 1) if controlled[s]), key=lambda s: (-controlled[s], s))[:top]
    table = []
    for s in order:
        cs = cells_of[s]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = conc[cs, s - 1] / conc[cs].max(axis=1)
        table.append((s, int(controlled[s]), int(rejected[s]), len(cs), float(np.median(ratio))))
    return {"attempts": np.array([r[2] for r in rows], np.int64), "kept": kept, "rejected": rej_total, "none": int(controlled[0]), "species": table}


def format_table(t, names=None):
    a = t["attempts"]
    lines = ["attempts per cell: min %d  median %g  max %d  (%d in %d cells; %d recorded, %d of them rejected)" %
             (a.min(), np.median(a), a.max(), a.sum(), len(a), t["kept"], t["rejected"])]
    if t["kept"] < a.sum():
        lines.append("records past the capacity were dropped: the table below counts the recorded attempts only")
    if t["none"]:
        lines.append("%d recorded attempts had no positive term (species 0)" % t["none"])
    lines.append("%-14s %10s %8s %9s %6s  %s" % ("species", "controlled", "of all", "rejected", "cells", "median conc / cell max"))
    for s, n, r, cells, med in t["species"]:
        label = names[s - 1] if names and s - 1 < len(names) else "VAR(%d)" % s
        lines.append("%-14s %10d %7.1f%% %9d %6d  %.2e" % (label, n, 100.0 * n / max(t["kept"], 1), r, cells, med))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mech", choices=MECHS)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--golden", help="npz file with the cells")
    src.add_argument("--workload", type=int, help="number of cells of the synthetic workload")
    ap.add_argument("--cells", help="slice lo:hi of the batch")
    ap.add_argument("--tstart", type=float, default=0.0)
    ap.add_argument("--tend", type=float, default=10.0)
    ap.add_argument("--atol", type=float, help="scalar AbsTol (default: INTEGRATE_x's 1e-25)")
    ap.add_argument("--atol-rel", type=float, help="scalar AbsTol per cell: this factor times the cell's largest concentration")
    ap.add_argument("--rtol", type=float, help="scalar RelTol (default: INTEGRATE_x's 1e-3)")
    ap.add_argument("--cap", type=int, default=1024, help="records kept per cell")
    ap.add_argument("--top", type=int, default=8, help="species listed")
    ap.add_argument("--names", help="file with one species name per line, in VAR's order")
    ap.add_argument("--cpu", action="store_true", help="run the Python restatement instead of the GPU")
    a = ap.parse_args(argv)
    if a.atol is not None and a.atol_rel is not None:
        ap.error("--atol and --atol-rel exclude each other")
    var, fix, rconst = load_cells(a.mech, a.golden, a.workload, a.cells)
    if a.atol_rel is not None:
        opts = lambda c: options(a.mech, a.atol_rel * np.abs(var[c]).max(), a.rtol)  # noqa: E731
        what = "AbsTol = %g x the cell's largest concentration" % a.atol_rel
    else:
        opts = options(a.mech, a.atol, a.rtol)
        what = "AbsTol = %g" % opts[2][0]
    run = trace_cpu if a.cpu else trace_gpu
    out, rows = run(a.mech, var, fix, rconst, a.tstart, a.tend, opts, a.cap)
    names = [l.strip() for l in open(a.names)] if a.names else None
    print("%s, %d cells, %g -> %g s, Ros3, %s, RelTol = %g (%s)" % (a.mech, var.shape[0], a.tstart, a.tend, what, 1.0e-3 if a.rtol is None else a.rtol,
                                                                   "CPU restatement" if a.cpu else "GPU trace"))
    print(format_table(control_table(var, out, rows, a.top), names))
    return 0


if __name__ == "__main__":
    sys.exit(main())
