#!/usr/bin/env python3
"""A box run over a dawn in one launch: cells of tests/golden/integrate_<mech>.npz (night) with the rate constants and FIX blended
into cells of integrate_<mech>_day.npz (day) over `--legs` legs of `--dt` seconds — leg k integrates with (1-w)*night + w*day at w = k / (legs-1),
piecewise constant over the leg, as the model's Update_RCONST_x + INTEGRATE_x per step.  The whole ramp is ONE call of chem.rosenbrock_series_rates;
the largest species of the first cell are printed per leg.  Night and day cells are different places: the ramp is an input, not a simulation.

    python tools/box_series.py <mech> [--legs 8] [--dt 10] [--cells 3] [--species 4]
    ... --compare      the queued sequence of chem.rosenbrock calls too (leg k's rows to call k): the states compared bit for bit, both wall times
    ... --cpu          the Python restatement called leg by leg (tests/ros_series_rates_py.py) instead of the GPU
    ... --linear       the same dawn with rate constants LINEAR IN TIME over each leg: legs + 1 node blocks at w = k / legs, ONE call of
                       chem.rosenbrock_series_linrates; FIX stays the staircase's.  With --compare: the staircase of the run without --linear beside it, the
                       distance of the two states per leg and the step counts of both.  With --cpu: tests/ros_linrates_py.py's restatement"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def ramp(mech, legs, ncell):
    """-> (VAR [ncell, NVAR], FIX [legs, ncell, NFIX], RCONST [legs, ncell, NREACT])"""
    g = np.load(os.path.join(GOLDEN, "integrate_%s.npz" % mech))
    d = np.load(os.path.join(GOLDEN, "integrate_%s_day.npz" % mech))
    n = min(ncell, g["var_in"].shape[0], d["var_in"].shape[0])
    w = np.linspace(0.0, 1.0, legs) if legs > 1 else np.zeros(1)
    return (g["var_in"][:n].copy(), np.stack([(1 - x) * g["fix"][:n] + x * d["fix"][:n] for x in w]),
            np.stack([(1 - x) * g["rconst"][:n] + x * d["rconst"][:n] for x in w]))


def nodes(mech, legs, ncell):
    """-> RCONST nodes [legs + 1, ncell, NREACT]: the same blend at the leg boundaries, w = k / legs"""
    g = np.load(os.path.join(GOLDEN, "integrate_%s.npz" % mech))
    d = np.load(os.path.join(GOLDEN, "integrate_%s_day.npz" % mech))
    n = min(ncell, g["var_in"].shape[0], d["var_in"].shape[0])
    return np.stack([(1 - x) * g["rconst"][:n] + x * d["rconst"][:n] for x in np.linspace(0.0, 1.0, legs + 1)])


def run_cpu_linear(mech, V, LF, NK, times):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_linrates_py as LR
    import ros_options_py as R
    import ros_series_py as RS
    ipar, rpar, atol, rtol = R.base_options(mech)
    r = LR.chain_cells(mech, RS.Series(ipar, rpar, atol, rtol, times, False), V, LF, NK)
    return r[0], r[1], r[2]


def run_cpu(mech, V, LF, LK, times):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_methods_py as RM
    import ros_options_py as R
    import ros_series_py as RS
    import ros_series_rates_py as SR
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    ipar, rpar, atol, rtol = R.base_options(mech)
    s = RS.Series(ipar, rpar, atol, rtol, times, False)
    cells = [SR.chain_rates(lambda y, f, k, rp, t0, t1: RM.rosenbrock(o, diag, y, f, k, ipar, rp, atol, rtol, t0, t1), V[c], s, LF[:, c], LK[:, c])
             for c in range(V.shape[0])]
    return np.stack([c[0] for c in cells], axis=1), np.stack([c[1] for c in cells], axis=1), np.stack([c[2] for c in cells], axis=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mech", choices=("gas", "aer", "tot"))
    ap.add_argument("--legs", type=int, default=8)
    ap.add_argument("--dt", type=float, default=10.0)
    ap.add_argument("--cells", type=int, default=3)
    ap.add_argument("--species", type=int, default=4)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--linear", action="store_true")
    a = ap.parse_args(argv)
    V, LF, LK = ramp(a.mech, a.legs, a.cells)
    times = a.dt * np.arange(a.legs + 1)
    if a.linear:
        return main_linear(a, V, LF, LK, nodes(a.mech, a.legs, a.cells), times)
    print("%s: %d cell(s), %d legs of %g s, night -> day rows blended per leg; %s" %
          (a.mech, V.shape[0], a.legs, a.dt, "CPU restatement, leg by leg" if a.cpu else "one launch (chem.rosenbrock_series_rates)"))
    if a.cpu:
        var, ierr, stats = run_cpu(a.mech, V, LF, LK, times)
    else:
        import torch
        from mistra_amd import chem
        dev = torch.device("cuda", 0)
        chem.init(0)
        dV, dF, dK = (torch.tensor(x, device=dev) for x in (V, LF, LK))

        def series():
            return chem.rosenbrock_series_rates(a.mech, dV, dF, dK, times)

        def sequence():
            y, legs = dV, []
            for k in range(a.legs):
                y = chem.rosenbrock(a.mech, y, dF[k], dK[k], float(times[k]), float(times[k + 1]))[0].var
                legs.append(y)
            return legs

        def timed(f):
            f()      # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            return r, 1.0e3 * (time.perf_counter() - t0)
        res, t_series = timed(series)
        var, ierr, stats = res.var.cpu().numpy(), res.ierr.cpu().numpy(), res.stats.cpu().numpy()
        if a.compare:
            legs, t_seq = timed(sequence)
            same = np.stack([y.cpu().numpy() for y in legs]).tobytes() == var.tobytes()
            print("one launch %.3f ms, %d queued calls %.3f ms (wall, behind one warm-up each); the states of all legs %s" %
                  (t_series, a.legs, t_seq, "identical bit for bit" if same else "DIFFER"))
    report(a, V, times, var, ierr, stats)
    return 0


def report(a, V, times, var, ierr, stats):
    top = np.argsort(-np.abs(V[0]))[:a.species]
    print("cell 0, species (0-based) %s; IERR and Nstp of the leg over all cells" % " ".join("%d" % i for i in top))
    for k in range(a.legs):
        print("leg %d %s | t = %g s, IERR %s, Nstp %d .. %d" % (k, " ".join("%.9e" % var[k, 0, i] for i in top), times[k + 1], sorted(set(ierr[k].tolist())),
                                                             stats[k, :, 2].min(), stats[k, :, 2].max()))


def main_linear(a, V, LF, LK, NK, times):
    """--linear: the dawn with node blocks; --compare: the staircase beside it"""
    print("%s: %d cell(s), %d legs of %g s, night -> day rate constants linear in time over each leg (%d node blocks); %s" %
          (a.mech, V.shape[0], a.legs, a.dt, a.legs + 1, "CPU restatement, leg by leg" if a.cpu else "one launch (chem.rosenbrock_series_linrates)"))
    if a.cpu:
        var, ierr, stats = run_cpu_linear(a.mech, V, LF, NK, times)
        if a.compare:
            svar, sierr, sstats = run_cpu(a.mech, V, LF, LK, times)
    else:
        import torch
        from mistra_amd import chem
        dev = torch.device("cuda", 0)
        chem.init(0)
        dV, dF, dK, dN = (torch.tensor(x, device=dev) for x in (V, LF, LK, NK))
        res = chem.rosenbrock_series_linrates(a.mech, dV, dF, dN, times)
        torch.cuda.synchronize()
        var, ierr, stats = res.var.cpu().numpy(), res.ierr.cpu().numpy(), res.stats.cpu().numpy()
        if a.compare:
            res = chem.rosenbrock_series_rates(a.mech, dV, dF, dK, times)
            torch.cuda.synchronize()
            svar, sierr, sstats = res.var.cpu().numpy(), res.ierr.cpu().numpy(), res.stats.cpu().numpy()
    report(a, V, times, var, ierr, stats)
    if a.compare:
        print("the staircase (leg k with the rows at w = k / (legs - 1), piecewise constant) beside it: largest |linear - staircase| of a cell as a fraction of "
              "the cell's largest concentration, steps (accepted + rejected) of all cells")
        for k in range(a.legs):
            d = (np.abs(var[k] - svar[k]).max(axis=1) / np.abs(svar[k]).max(axis=1)).max()
            print("cmp %d distance %.3e | Nstp linear %d, staircase %d" % (k, d, stats[k, :, 2].sum(), sstats[k, :, 2].sum()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
