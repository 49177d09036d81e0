#!/usr/bin/env python3
"""The dense-output call against the call it does not change and against the series it replaces for looking inside a step (INTEGRATION.md §4o;
profiles/r15_dense_kernels.txt): per mechanism, `--cells` cells of the synthetic workload (mistra_amd/workload.py), Ros3 at INTEGRATE_x's options,
0 -> 10 s — once as mistra_chem_rosenbrock_device (the sibling), once as the dense-output device entry with `--samples` equal sample times, once as a
series of `--samples` legs over the same times.  `--repeats` timed repeats of each behind one warm-up, taken in turn.  Per repeat: the time between two
events on the stream around the call — the kernel and the copy of the options block in front of it.  The dense call's end state is compared with the
sibling's bit for bit first.  Nothing is asserted on the times.

    python tools/bench_dense.py [--cells 4096] [--samples 8] [--repeats 7] [--mechs gas aer tot]"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--mechs", nargs="+", default=["gas", "aer", "tot"])
    a = ap.parse_args(argv)
    import torch
    from mistra_amd import chem
    from mistra_amd import workload as W
    dev = torch.device("cuda", 0)
    chem.init(0)
    times = np.linspace(0.0, 10.0, a.samples + 1)
    print("%d cells, Ros3 at INTEGRATE_x's options, 0 -> 10 s, %d sample times / legs; %d repeats behind one warm-up; stream ms: median [min .. max]" %
          (a.cells, a.samples, a.repeats))
    for mech in a.mechs:
        V, F, K = W.make_batch(mech, 0, a.cells, dev)
        sides = {"sibling": lambda: chem.rosenbrock(mech, V, F, K, 0.0, 10.0)[0].var,
                 "dense": lambda: chem.rosenbrock_dense(mech, V, F, K, 0.0, 10.0, times[1:])[0].var,
                 "series": lambda: chem.rosenbrock_series(mech, V, F, K, times).var[-1]}

        def timed(f):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = f()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), y

        warm = {k: timed(f)[1] for k, f in sides.items()}
        same = warm["dense"].cpu().numpy().tobytes() == warm["sibling"].cpu().numpy().tobytes()
        rows = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, f in sides.items():
                rows[k].append(timed(f)[0])
        print("%s: end state of the dense call and of the sibling %s" % (mech, "identical bit for bit" if same else "DIFFER"))
        for k in sides:
            print("  %-8s %9.3f [%9.3f .. %9.3f]" % (k, float(np.median(rows[k])), min(rows[k]), max(rows[k])))
        med = {k: float(np.median(v)) for k, v in rows.items()}
        sib = np.array(rows["sibling"])
        print("  dense / sibling %.4f   dense / series %.4f   (medians); the sibling's own spread (max - min) / median %.4f" %
              (med["dense"] / med["sibling"], med["dense"] / med["series"], (sib.max() - sib.min()) / med["sibling"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
