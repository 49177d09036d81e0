#!/usr/bin/env python3
"""One series against the sequence of calls it replaces (profiles/r13_series_kernels.txt, r17_series_rates_kernels.txt): per
mechanism, `--cells` cells of the synthetic workload (mistra_amd/workload.py), Ros3 at INTEGRATE_x's options, `--legs` equal legs over 0 -> 10 s — once
as ONE call of the series device entry, once as `--legs` queued calls of mistra_chem_rosenbrock_device on the chained state.  `--repeats` timed repeats
of each behind one warm-up, taken in turn.  Per repeat: the time between two events on the stream around the call(s) — the kernels and the copies of
the options blocks in front of them — and the wall time from the first call to the end of the synchronisation.  The two sides' states are compared bit
for bit first.

    python tools/bench_series.py [--cells 4096] [--legs 8] [--repeats 5] [--mechs gas aer tot]
    python tools/bench_series.py --rates            every leg with rate constants and FIX of its own (chem.rosenbrock_series_rates): leg k's rate
                                                    constants are the workload's times 1 + 0.02*k, FIX a copy per leg; the sequence passes leg k's rows
    python tools/bench_series.py --against LIB      the plain series of this tree's library against the plain series of another build of the library
                                                    (a second copy of mistra_amd/chem.py bound to LIB, in the same process), taken in turn
    python tools/bench_series.py --flux             the series with the reaction flux of every leg (chem.rosenbrock_series_flux), the legs'
                                                    rows as for --rates: ONE call against the `--legs` queued calls of chem.rosenbrock_flux it replaces, and
                                                    against the series-with-rates call without the flux.  The flux rows of the two flux sides and the end
                                                    states of all three are compared bit for bit first.  With --against LIB the two baselines are the other
                                                    build's (a parent build: what the call replaces there)"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def other_build(path):
    """a second copy of mistra_amd.chem bound to the library at `path`"""
    spec = importlib.util.spec_from_file_location("mistra_amd.chem_other", os.path.join(REPO, "mistra_amd", "chem.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(path)
    return mod


def main_flux(a, chem, other, dev):
    """--flux: one series-flux call | the queued flux calls it replaces | the series with rates without the flux"""
    import torch
    from mistra_amd import workload as W
    base = other if other is not None else chem
    times = np.linspace(0.0, 10.0, a.legs + 1)
    print("%d cells, Ros3 at INTEGRATE_x's options, %d legs of %g s, rate constants and FIX of the leg's own, with the reaction flux of every leg; "
          "%d repeats behind one warm-up; ms: median [min .. max]%s" %
          (a.cells, a.legs, 10.0 / a.legs, a.repeats, "; the two baselines run the library given with --against" if other is not None else ""))
    for mech in a.mechs:
        V, F, K = W.make_batch(mech, 0, a.cells, dev)
        scale = torch.tensor(1.0 + 0.02 * np.arange(a.legs), device=dev).view(-1, 1, 1)
        LK, LF = (K.unsqueeze(0) * scale).contiguous(), F.unsqueeze(0).repeat(a.legs, 1, 1).contiguous()

        def series_flux():
            r = chem.rosenbrock_series_flux(mech, V, LF, LK, times)
            return r.var[-1], r.flux

        def flux_calls():
            y, rows = V, []
            for k in range(a.legs):
                r = base.rosenbrock_flux(mech, y, LF[k], LK[k], float(times[k]), float(times[k + 1]))
                y = r[0].var
                rows.append(r[2])
            return y, rows

        def series_rates():
            return base.rosenbrock_series_rates(mech, V, LF, LK, times).var[-1], None

        def timed(f):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            y = f()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), 1.0e3 * (time.perf_counter() - t0), y

        sides = (("series_flux", series_flux), ("flux_calls", flux_calls), ("series_rates", series_rates))
        warm = {name: timed(f)[2] for name, f in sides}
        same_y = all(warm[n][0].cpu().numpy().tobytes() == warm["series_flux"][0].cpu().numpy().tobytes() for n in warm)
        same_f = torch.stack(warm["flux_calls"][1]).cpu().numpy().tobytes() == warm["series_flux"][1].cpu().numpy().tobytes()
        rows = {name: [] for name, _ in sides}
        for _ in range(a.repeats):
            for name, f in sides:
                rows[name].append(timed(f)[:2])
        fmt = lambda x: "%9.3f [%9.3f .. %9.3f]" % (float(np.median(x)), min(x), max(x))
        print("%s: end states of the three sides %s; flux rows of all legs, series against queued calls, %s" %
              (mech, "identical bit for bit" if same_y else "DIFFER", "identical bit for bit" if same_f else "DIFFER"))
        med = {}
        for name, _ in sides:
            ev, wall = np.array([r[0] for r in rows[name]]), np.array([r[1] for r in rows[name]])
            med[name] = (np.median(ev), np.median(wall), (ev.max() - ev.min()) / np.median(ev), (wall.max() - wall.min()) / np.median(wall))
            print("  %-12s stream %s   wall %s" % (name, fmt(ev), fmt(wall)))
        for name in ("flux_calls", "series_rates"):
            print("  series_flux / %s: stream %.4f, wall %.4f (medians); %s's own spread (max - min) / median: stream %.4f, wall %.4f" %
                  (name, med["series_flux"][0] / med[name][0], med["series_flux"][1] / med[name][1], name, med[name][2], med[name][3]))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--legs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mechs", nargs="+", default=["gas", "aer", "tot"])
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--against", metavar="LIB")
    ap.add_argument("--flux", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from mistra_amd import chem
    from mistra_amd import workload as W
    dev = torch.device("cuda", 0)
    chem.init(0)
    other = None
    if a.against:
        other = other_build(a.against)
        other.init(0)
    if a.flux:
        return main_flux(a, chem, other, dev)
    times = np.linspace(0.0, 10.0, a.legs + 1)
    print("%d cells, Ros3 at INTEGRATE_x's options, %d legs of %g s%s; %d repeats behind one warm-up; ms: median [min .. max]" %
          (a.cells, a.legs, 10.0 / a.legs, ", rate constants and FIX of the leg's own" if a.rates else "", a.repeats))
    for mech in a.mechs:
        V, F, K = W.make_batch(mech, 0, a.cells, dev)
        if a.rates:
            scale = torch.tensor(1.0 + 0.02 * np.arange(a.legs), device=dev).view(-1, 1, 1)
            LK, LF = (K.unsqueeze(0) * scale).contiguous(), F.unsqueeze(0).repeat(a.legs, 1, 1).contiguous()

        def series():
            if a.rates:
                return chem.rosenbrock_series_rates(mech, V, LF, LK, times).var[-1]
            return chem.rosenbrock_series(mech, V, F, K, times).var[-1]

        def sequence():
            if other is not None:
                return other.rosenbrock_series(mech, V, F, K, times).var[-1]
            y = V
            for k in range(a.legs):
                y = chem.rosenbrock(mech, y, LF[k] if a.rates else F, LK[k] if a.rates else K, float(times[k]), float(times[k + 1]))[0].var
            return y

        def timed(f):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            y = f()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), 1.0e3 * (time.perf_counter() - t0), y

        a_name, b_name = ("this", "other") if other is not None else ("series", "sequence")
        ys, yq = timed(series)[2], timed(sequence)[2]      # warm-up
        same = ys.cpu().numpy().tobytes() == yq.cpu().numpy().tobytes()
        rows = {a_name: [], b_name: []}
        for _ in range(a.repeats):
            rows[a_name].append(timed(series)[:2])
            rows[b_name].append(timed(sequence)[:2])
        fmt = lambda x: "%9.3f [%9.3f .. %9.3f]" % (float(np.median(x)), min(x), max(x))
        print("%s: end states of the two sides %s" % (mech, "identical bit for bit" if same else "DIFFER"))
        for side in (a_name, b_name):
            ev, wall = [r[0] for r in rows[side]], [r[1] for r in rows[side]]
            print("  %-9s stream %s   wall %s" % (side, fmt(ev), fmt(wall)))
        ev_s, ev_q = np.array([r[0] for r in rows[a_name]]), np.array([r[0] for r in rows[b_name]])
        wl_s, wl_q = np.array([r[1] for r in rows[a_name]]), np.array([r[1] for r in rows[b_name]])
        print("  %s / %s: stream %.4f, wall %.4f (medians); the %s's own spread (max - min) / median: stream %.4f, wall %.4f" %
              (a_name, b_name, np.median(ev_s) / np.median(ev_q), np.median(wl_s) / np.median(wl_q), b_name if other is None else "other build",
               (ev_q.max() - ev_q.min()) / np.median(ev_q), (wl_q.max() - wl_q.min()) / np.median(wl_q)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
