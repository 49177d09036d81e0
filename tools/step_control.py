#!/usr/bin/env python3
"""Which species control the step size of Rosenbrock_x (Ros3) on a batch of cells, from the step-control trace of the integrator
(mistra_chem_rosenbrock_trace_ex, include/mistra_chem.h).

    python tools/step_control.py tot --golden tests/golden/column_BTZ96.npz                 the tot cells of a captured column step, INTEGRATE_x's options
    python tools/step_control.py tot --golden tests/golden/column_BTZ96.npz --atol 1e-15     ... with a scalar AbsTol
    python tools/step_control.py tot --golden tests/golden/integrate_tot.npz --atol-rel 1e-13    AbsTol = 1e-13 x the cell's largest concentration: ONE batched
                                                                                             call with tolerances per cell (cell_atol + rosenbrock_trace_cells)
    ... --yardstick                                                                          also the distance of the end state from Rodas4 at RelTol 1e-7
    python tools/step_control.py aer --workload 4096                                         cells 0 .. 4095 of the synthetic workload (mistra_amd/workload.py)
    ... --series 4                                                                           the yardstick distance at 4 equal sub-times, not at the end only
    ... --dense 4                                                                            the same table with the run's side sampled inside ONE call (dense output)
    ... --cpu                                                                                the Python restatement (tests/ros_trace_py.py) instead of the GPU

Prints the attempts per cell and, for the species that controlled the most attempts (the species with the largest term of ros_ErrorNorm_x's sum):
the attempts it controlled, how many of those were rejected, in how many cells, and the median over those cells of its concentration relative to the
cell's largest — the concentration being max(|VAR in|, |VAR out|) of the call.  Species are numbered as in VAR (1-based); --names FILE (one name per
line, in that order) prints names, the mechanism tables carry none.

--yardstick integrates the same cells once more with Rodas4 at scalar RelTol = 1e-7 and INTEGRATE_x's AbsTol (the yardstick of
profiles/r02_hstart_reuse_study.txt; one batched call) and prints how far the run's end state lies from it: the largest relative difference over the
species above 1e-3 of their cell's maximum, and over all species with the floor 1e-12 x max|c| (tests/conftest.py: rel_diff).  These are properties of
the reference algorithm at the run's tolerances, not of this library: nothing is asserted on them.

--series K prints that distance at K equal sub-times of the interval instead: the run's options and the yardstick's each as ONE series of K legs
(mistra_chem_rosenbrock_series_ex, INTEGRATION.md §4m: K calls of Rosenbrock_x on the chained state in one launch), so the table shows where inside
the chemistry step the run leaves the yardstick.  Every leg is a call of its own — its first step is RPAR(3) again — so the last row is the distance
after K calls, not the single call's.

--dense K prints the same table with the run's side taken from ONE call of Rosenbrock_x over the whole interval, sampled at the K sub-times by the dense
output (mistra_chem_rosenbrock_dense_ex, INTEGRATION.md §4o: the cubic Hermite interpolant between the call's own accepted states).  Looking does not
perturb the integration: the last row IS the single call's end state.  The yardstick stays a Rodas4 series.  Rows a cell does not reach (IERR < 0) are
left out of the row's maximum and counted."""
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


YARDSTICK_METHOD, YARDSTICK_RTOL = 5, 1.0e-7      # Rodas4 at RelTol 1e-7, AbsTol INTEGRATE_x's 1e-25
ATOL_FLOOR = 1.0e-300                             # cell_atol's floor: a cell without a positive concentration still gets an AbsTol Rosenbrock_x accepts


def cell_atol_rows(mech, var, factor):
    """[ncell, 1]: factor x the cell's largest |concentration| (chem.cell_atol's host formula; the GPU path runs the kernel on the device instead)"""
    from mistra_amd import chem
    return chem.cell_atol(mech, var, factor, ATOL_FLOOR)


def trace_gpu(mech, var, fix, rconst, tstart, tend, opts, cap, atol_rel=None):
    """-> (var_out, [(species, code, n) per cell]) from the kernel, ONE batched call: opts = (ipar, rpar, atol, rtol) shared by the batch, or with
    atol_rel AbsTol per cell formed on the device from each cell's own state (cell_atol) and handed to rosenbrock_trace_cells without leaving it"""
    import torch
    from mistra_amd import chem
    ipar, rpar, atol, rtol = opts
    if atol_rel is None:
        res, _, tr = chem.rosenbrock_trace(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol, cap=cap, ctrl=False)
        out, species, code, n = res.var, tr.species, tr.code, tr.n
    else:
        dev = torch.device("cuda", 0)
        dv, df, dk = (torch.tensor(x, device=dev) for x in (var, fix, rconst))
        d_atol = chem.cell_atol(mech, dv, atol_rel, ATOL_FLOOR)
        d_rtol = torch.full((var.shape[0], 1), float(rtol[0]), dtype=torch.float64, device=dev)
        res, _, tr = chem.rosenbrock_trace_cells(mech, dv, df, dk, tstart, tend, ipar, rpar, d_atol, d_rtol, cap=cap, ctrl=False)
        torch.cuda.synchronize()
        out, species, code, n = (x.cpu().numpy() for x in (res.var, tr.species, tr.code, tr.n))
    rows = []
    for c in range(out.shape[0]):
        k = min(int(n[c]), cap)
        rows.append((species[c, :k].copy(), code[c, :k].copy(), int(n[c])))
    return out, rows


def trace_cpu(mech, var, fix, rconst, tstart, tend, opts, cap, atol_rel=None):
    """the same from the restatement (tests/ros_trace_py.py over the C oracle), cell by cell"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_trace_py as RT
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    ipar, rpar, atol, rtol = opts
    per_cell = None if atol_rel is None else cell_atol_rows(mech, var, atol_rel)
    out, rows = np.empty_like(var), []
    for c in range(var.shape[0]):
        at = atol if per_cell is None else np.full_like(atol, per_cell[c, 0])
        r = RT.rosenbrock_trace(o, diag, var[c], fix[c], rconst[c], ipar, rpar, at, rtol, tstart=tstart, tend=tend)
        out[c] = r[0]
        tr = r[5]
        rows.append((tr.species[:cap].copy(), tr.code[:cap].copy(), len(tr.species)))
    return out, rows


def yardstick(mech, var, fix, rconst, tstart, tend, cpu):
    """the cells' end state by Rodas4 at RelTol 1e-7 and INTEGRATE_x's AbsTol -> var_out: one batched call, or the restatement under --cpu"""
    ipar, rpar, atol, rtol = options(mech, None, YARDSTICK_RTOL)
    ipar[3] = YARDSTICK_METHOD
    if not cpu:
        from mistra_amd import chem
        return chem.rosenbrock(mech, var, fix, rconst, tstart, tend, ipar, rpar, atol, rtol)[0].var
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_methods_py as RM
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    return np.array([RM.rosenbrock(o, diag, var[c], fix[c], rconst[c], ipar, rpar, atol, rtol, tstart, tend)[0] for c in range(var.shape[0])])


def series_states(mech, var, fix, rconst, times, opts, cpu, atol_rel=None):
    """the cells' states at times[1:] by one series of Rosenbrock_x calls with opts = (ipar, rpar, atol, rtol) -> [nleg, ncell, NVAR]; atol_rel: AbsTol
    per cell from the state the series receives, for every leg.  --cpu: the restatement called leg by leg on its chained state (tests/ros_series_py.py)"""
    ipar, rpar, atol, rtol = opts
    per_cell = None if atol_rel is None else cell_atol_rows(mech, var, atol_rel)
    if not cpu:
        from mistra_amd import chem
        if per_cell is None:
            return chem.rosenbrock_series(mech, var, fix, rconst, times, ipar, rpar, atol, rtol).var
        return chem.rosenbrock_series(mech, var, fix, rconst, times, ipar, rpar, per_cell, np.full_like(per_cell, rtol[0])).var
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_methods_py as RM
    import ros_series_py as RS
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    out = np.empty((len(times) - 1,) + var.shape)
    for c in range(var.shape[0]):
        at = atol if per_cell is None else np.full_like(atol, per_cell[c, 0])
        s = RS.Series(ipar, rpar, at, rtol, np.asarray(times, np.float64), False)
        out[:, c] = RS.chain(lambda y, rp, t0, t1: RM.rosenbrock(o, diag, y, fix[c], rconst[c], ipar, rp, at, rtol, t0, t1), var[c], s)[0]
    return out


def dense_states(mech, var, fix, rconst, ts, tstart, tend, opts, cpu, atol_rel=None):
    """the cells' states at ts inside ONE call of Rosenbrock_x from tstart to tend with opts -> (samples [ns, ncell, NVAR], nout [ncell]); atol_rel: AbsTol
    per cell from the state the call receives.  --cpu: the restatement with the sampling (tests/ros_dense_py.py)"""
    ipar, rpar, atol, rtol = opts
    per_cell = None if atol_rel is None else cell_atol_rows(mech, var, atol_rel)
    if not cpu:
        from mistra_amd import chem
        if per_cell is None:
            r = chem.rosenbrock_dense(mech, var, fix, rconst, tstart, tend, ts, ipar, rpar, atol, rtol)
        else:
            r = chem.rosenbrock_dense_cells(mech, var, fix, rconst, tstart, tend, ts, ipar, rpar, per_cell, np.full_like(per_cell, rtol[0]))
        return r[2], r[3]
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_dense_py as RD
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    out, nout = np.zeros((len(ts),) + var.shape), np.zeros(var.shape[0], np.int32)
    for c in range(var.shape[0]):
        at = atol if per_cell is None else np.full_like(atol, per_cell[c, 0])
        r = RD.rosenbrock(o, diag, var[c], fix[c], rconst[c], ts, ipar, rpar, at, rtol, tstart, tend)
        out[:, c], nout[c] = r[5], r[6]
    return out, nout


def distances(got, want):
    """-> (largest relative difference over the species above 1e-3 of their cell's maximum, largest over all species with the floor 1e-12 x max|c|):
    the two measures of tests/conftest.py (rel_diff), NaN where nothing can be compared"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    top = np.abs(want).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.abs(want)
        major = np.abs(want) > 1.0e-3 * top
        a = float(rel[major].max()) if major.any() else float("nan")
        b = float((np.abs(got - want) / (np.abs(want) + 1.0e-12 * top)).max())
    return a, b


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
    ap.add_argument("--yardstick", action="store_true", help="also print the end state's distance from Rodas4 at RelTol 1e-7, INTEGRATE_x's AbsTol")
    ap.add_argument("--series", type=int, metavar="K", help="print the yardstick distance at K equal sub-times (one series of K legs each)")
    ap.add_argument("--dense", type=int, metavar="K", help="the same table, the run's side sampled at the K sub-times inside ONE call (dense output)")
    a = ap.parse_args(argv)
    if a.atol is not None and a.atol_rel is not None:
        ap.error("--atol and --atol-rel exclude each other")
    var, fix, rconst = load_cells(a.mech, a.golden, a.workload, a.cells)
    opts = options(a.mech, a.atol, a.rtol)
    what = "AbsTol = %g" % opts[2][0] if a.atol_rel is None else "AbsTol = %g x the cell's largest concentration" % a.atol_rel
    run = trace_cpu if a.cpu else trace_gpu
    out, rows = run(a.mech, var, fix, rconst, a.tstart, a.tend, opts, a.cap, a.atol_rel)
    names = [l.strip() for l in open(a.names)] if a.names else None
    print("%s, %d cells, %g -> %g s, Ros3, %s, RelTol = %g (%s)" % (a.mech, var.shape[0], a.tstart, a.tend, what, 1.0e-3 if a.rtol is None else a.rtol,
                                                                   "CPU restatement" if a.cpu else "GPU trace"))
    print(format_table(control_table(var, out, rows, a.top), names))
    if a.yardstick:
        major, every = distances(out, yardstick(a.mech, var, fix, rconst, a.tstart, a.tend, a.cpu))
        print("distance from the yardstick (Rodas4, RelTol = %g, AbsTol = 1e-25): species above 1e-3 of the cell's maximum: %.3e   all species, floor "
              "1e-12 x max|c|: %.3e" % (YARDSTICK_RTOL, major, every))
    if a.series:
        if a.series < 1:
            ap.error("--series K: K >= 1")
        times = np.linspace(a.tstart, a.tend, a.series + 1)
        yopts = options(a.mech, None, YARDSTICK_RTOL)
        yopts[0][3] = YARDSTICK_METHOD
        got = series_states(a.mech, var, fix, rconst, times, opts, a.cpu, a.atol_rel)
        want = series_states(a.mech, var, fix, rconst, times, yopts, a.cpu)
        print("distance from the yardstick at %d sub-times, each side one series of %d calls (Rodas4, RelTol = %g, AbsTol = 1e-25)" % (a.series, a.series, YARDSTICK_RTOL))
        print("%12s  %-28s %s" % ("t [s]", "species above 1e-3 of cell max", "all species, floor 1e-12 x max|c|"))
        for k in range(a.series):
            major, every = distances(got[k], want[k])
            print("%12g  %-28.3e %.3e" % (times[k + 1], major, every))
    if a.dense:
        if a.dense < 1:
            ap.error("--dense K: K >= 1")
        times = np.linspace(a.tstart, a.tend, a.dense + 1)
        yopts = options(a.mech, None, YARDSTICK_RTOL)
        yopts[0][3] = YARDSTICK_METHOD
        got, nout = dense_states(a.mech, var, fix, rconst, times[1:], a.tstart, a.tend, opts, a.cpu, a.atol_rel)
        want = series_states(a.mech, var, fix, rconst, times, yopts, a.cpu)
        print("distance from the yardstick at %d sub-times, dense output: the run's side sampled inside ONE call, the yardstick one series of %d calls "
              "(Rodas4, RelTol = %g, AbsTol = 1e-25)" % (a.dense, a.dense, YARDSTICK_RTOL))
        print("%12s  %-28s %-34s %s" % ("t [s]", "species above 1e-3 of cell max", "all species, floor 1e-12 x max|c|", "cells that reached it"))
        for k in range(a.dense):
            hit = nout > k
            major, every = distances(got[k][hit], want[k][hit]) if hit.any() else (float("nan"), float("nan"))
            print("%12g  %-28.3e %-34.3e %d" % (times[k + 1], major, every, int(hit.sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
