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
                       distance of the two states per leg and the step counts of both.  With --cpu: tests/ros_linrates_py.py's restatement
    ... --budget SPECIES[,SPECIES...] [--top N]
                       the staircase run as ONE call of chem.rosenbrock_series_flux, and per leg and species (0-based, cell 0) the
                       budget of the leg: the N reactions (1-based, KPP's numbering) that produced and destroyed most of it, S(i,r) * flux[k][r] with S =
                       mechtab.load(mech).stoich(), the gross turnover and the net change (what the trapezoid gives: Y(t_k+1) - Y(t_k) up to its
                       accuracy).  With --cpu: tests/ros_series_flux_py.py's restatement"""
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


def run_cpu_flux(mech, V, LF, LK, times):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_options_py as R
    import ros_series_flux_py as SF
    import ros_series_py as RS
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    ipar, rpar, atol, rtol = R.base_options(mech)
    s = RS.Series(ipar, rpar, atol, rtol, times, False)
    cells = [SF.chain_flux(o, diag, V[c], s, LF[:, c], LK[:, c]) for c in range(V.shape[0])]
    return tuple(np.stack([c[i] for c in cells], axis=1) for i in (0, 1, 2, 5))


def main_budget(a, V, LF, LK, times):
    """--budget: the staircase with the reaction flux of every leg, one launch; the budget of the species asked for, per leg"""
    from mistra_amd import mechtab
    species = [int(x) for x in a.budget.split(",") if x != ""]
    S = mechtab.load(a.mech).stoich()
    if not species or min(species) < 0 or max(species) >= S.shape[0]:
        raise SystemExit("--budget: species are 0-based indices below NVAR = %d" % S.shape[0])
    print("%s: %d cell(s), %d legs of %g s, night -> day rows blended per leg, with the reaction flux of every leg; %s" %
          (a.mech, V.shape[0], a.legs, a.dt, "CPU restatement, leg by leg" if a.cpu else "one launch (chem.rosenbrock_series_flux)"))
    if a.cpu:
        var, ierr, stats, flux = run_cpu_flux(a.mech, V, LF, LK, times)
    else:
        import torch
        from mistra_amd import chem
        dev = torch.device("cuda", 0)
        chem.init(0)
        res = chem.rosenbrock_series_flux(a.mech, *(torch.tensor(x, device=dev) for x in (V, LF, LK)), times)
        torch.cuda.synchronize()
        var, ierr, stats, flux = (x.cpu().numpy() for x in (res.var, res.ierr, res.stats, res.flux))
    report(a, V, times, var, ierr, stats)
    print("cell 0: budget of the leg, S(i,r) * flux[leg][r] in the state's units; reactions 1-based")
    for k in range(a.legs):
        for i in species:
            term = S[i] * flux[k, 0]
            prod, dest = term[term > 0.0].sum(), term[term < 0.0].sum()
            print("budget leg %d species %d | production %.9e destruction %.9e turnover %.9e net %.9e | Y(t_k+1) - Y(t_k) = %.9e" %
                  (k, i, prod, dest, prod - dest, prod + dest, var[k, 0, i] - (V[0, i] if k == 0 else var[k - 1, 0, i])))
            order = np.argsort(-term)
            for r in [r for r in order[:a.top] if term[r] > 0.0]:
                print("  + reaction %d %.9e" % (r + 1, term[r]))
            for r in [r for r in order[::-1][:a.top] if term[r] < 0.0]:
                print("  - reaction %d %.9e" % (r + 1, term[r]))
    return 0


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
    ap.add_argument("--budget", default=None, metavar="SPECIES[,SPECIES...]")
    ap.add_argument("--top", type=int, default=3)
    a = ap.parse_args(argv)
    V, LF, LK = ramp(a.mech, a.legs, a.cells)
    times = a.dt * np.arange(a.legs + 1)
    if a.budget is not None:
        if a.linear:
            raise SystemExit("--budget: there is no reaction flux with rate constants linear in time")
        return main_budget(a, V, LF, LK, times)
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
