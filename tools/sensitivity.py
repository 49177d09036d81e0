#!/usr/bin/env python3
"""End-state sensitivities of one cell of Rosenbrock_x (Ros3) by internal numerical differentiation: the base cell's accepted step sequence is frozen
and every perturbed copy is replayed along it (mistra_chem_rosenbrock_replay_ex, include/mistra_chem.h; chem.sensitivities).

    python tools/sensitivity.py gas --golden tests/golden/integrate_gas_day.npz --cell 0 --rconst 30,38 --var 5 --species 5,12
    ... --adaptive        also the same central differences from plain adaptive calls: the step control's noise the replay removes
    ... --restated        the Python restatement (tests/ros_replay_py.py over the C oracle) instead of the GPU

--golden takes a captured set (integrate_<mech>.npz, column_*.npz) or any .npz with var_in, fix and rconst.  Parameters and species are numbered as in
VAR, RCONST and FIX (1-based).  Prints, per parameter p, the semi-normalised sensitivity p * dy/dp of the species asked for (default: the five that
answer most), the steps of the frozen sequence and the largest Err of a perturbed copy's step: above 1 the frozen sequence no longer meets the
tolerance for that copy, and eps is too large.  eps trades truncation (eps**2) against round-off (2e-16 / eps): 1e-6 suits most parameters."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from step_control import MECHS, load_cells, options  # noqa: E402


def parse_params(var, rconst, fix):
    """the --var / --rconst / --fix lists (1-based, comma separated) -> chem.sensitivities' params (0-based)"""
    out = []
    for what, text in (("var", var), ("rconst", rconst), ("fix", fix)):
        out += [(what, int(x) - 1) for x in (text or "").split(",") if x]
    return out


def restated(mech, var, fix, rconst, tstart, tend, opts, params, eps, adaptive):
    """-> (dy replayed, dy adaptive or None, steps, largest Err of a perturbed copy) on the CPU"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ros_replay_py as RP
    import ros_trace_py as RT
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    base = RT.rosenbrock_trace(o, diag, var, fix, rconst, *opts, tstart=tstart, tend=tend)
    if base[1] != 1:
        raise SystemExit("the base cell's call returned IERR = %d: no step sequence to freeze" % base[1])
    hs = RP.accepted(base[5])
    dy = RP.sensitivity_restated(o, diag, var, fix, rconst, opts, params, eps, hs, tstart, tend)
    worst = 0.0
    cell = {"var": var, "fix": fix, "rconst": rconst}
    for what, i in params:
        for s in (1.0, -1.0):
            c = {k: v.copy() for k, v in cell.items()}
            c[what][i] = c[what][i] * (1.0 + s * eps)
            worst = max(worst, float(np.max(RP.rosenbrock_replay(o, diag, c["var"], c["fix"], c["rconst"], *opts, hs, tstart, tend)[5], initial=0.0)))
    ada = RP.sensitivity_restated(o, diag, var, fix, rconst, opts, params, eps, None, tstart, tend) if adaptive else None
    return dy, ada, len(hs), worst


def on_gpu(mech, var, fix, rconst, tstart, tend, opts, params, eps, adaptive):
    from mistra_amd import chem
    ipar, rpar, atol, rtol = opts
    s = chem.sensitivities(mech, var, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, params, eps)
    ada = None
    if adaptive:      # the same 2P cells through ONE plain adaptive call
        v, f, r, p = chem.sensitivity_cells(mech, var, fix, rconst, params, eps)
        y = chem.rosenbrock(mech, v, f, r, tstart, tend, ipar=ipar, rpar=rpar, atol=atol, rtol=rtol)[0].var
        ada = (y[1::2] - y[2::2]) / (2.0 * eps * p)[:, None]
    return s.dy, ada, s.nsteps, s.max_err


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mech", choices=MECHS)
    ap.add_argument("--golden", required=True, help="npz file with the cells")
    ap.add_argument("--cell", type=int, default=0)
    ap.add_argument("--var", help="species whose initial value is a parameter (1-based, comma separated)")
    ap.add_argument("--rconst", help="reactions whose rate constant is a parameter")
    ap.add_argument("--fix", help="fixed species whose value is a parameter")
    ap.add_argument("--species", help="species printed (default: the five that answer most to each parameter)")
    ap.add_argument("--eps", type=float, default=1.0e-6, help="relative perturbation")
    ap.add_argument("--tstart", type=float, default=0.0)
    ap.add_argument("--tend", type=float, default=10.0)
    ap.add_argument("--atol", type=float, help="scalar AbsTol (default: INTEGRATE_x's 1e-25)")
    ap.add_argument("--rtol", type=float, help="scalar RelTol (default: INTEGRATE_x's 1e-3)")
    ap.add_argument("--adaptive", action="store_true", help="also print the differences of plain adaptive calls")
    ap.add_argument("--restated", action="store_true", help="run the Python restatement instead of the GPU")
    a = ap.parse_args(argv)
    params = parse_params(a.var, a.rconst, a.fix)
    if not params:
        raise SystemExit("no parameter: give --var, --rconst or --fix")
    var, fix, rconst = (x[a.cell].copy() for x in load_cells(a.mech, a.golden))
    for what, i in params:
        v = {"var": var, "rconst": rconst, "fix": fix}[what]
        if not 0 <= i < v.size or v[i] == 0.0:
            raise SystemExit("%s %d is out of range or zero in this cell: a relative perturbation needs a value other than 0" % (what, i + 1))
    opts = options(a.mech, a.atol, a.rtol)
    run = restated if a.restated else on_gpu
    dy, ada, nsteps, worst = run(a.mech, var, fix, rconst, a.tstart, a.tend, opts, params, a.eps, a.adaptive)
    print("%s cell %d, %g -> %g s: %d frozen steps, eps %g, largest Err of a perturbed copy %.3g%s" %
          (a.mech, a.cell, a.tstart, a.tend, nsteps, a.eps, worst, "  (above 1: take a smaller eps)" if worst > 1.0 else ""))
    for k, (what, i) in enumerate(params):
        p = {"var": var, "rconst": rconst, "fix": fix}[what][i]
        semi = p * dy[k]
        which = [int(x) - 1 for x in a.species.split(",")] if a.species else np.argsort(-np.abs(semi))[:5].tolist()
        print("%s %d = %.6e" % (what, i + 1, p))
        for s in which:
            line = "    species %4d   p*dy/dp % .9e" % (s + 1, semi[s])
            if ada is not None:
                line += "   adaptive calls % .9e" % (p * ada[k][s])
            print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
