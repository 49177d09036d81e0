#!/usr/bin/env python3
"""The flux kernel beside its sibling (profiles/r14_flux_kernels.txt): per mechanism, `--cells` cells of the synthetic workload
(mistra_amd/workload.py), Ros3 at INTEGRATE_x's options, 0 -> 10 s — once through mistra_chem_rosenbrock_flux_device, once through
mistra_chem_rosenbrock_device.  `--repeats` timed repeats of each behind one warm-up, taken in turn; per repeat the time between two events on the
stream around the call (the kernel and the copy of the options block in front of it).  The two sides' end states are compared bit for bit first.

    python tools/bench_flux.py [--cells 4096] [--repeats 5] [--mechs gas aer tot] [--method 2]"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mechs", nargs="+", default=["gas", "aer", "tot"])
    ap.add_argument("--method", type=int, default=2)
    a = ap.parse_args(argv)
    import torch
    from mistra_amd import chem
    from mistra_amd import workload as W
    dev = torch.device("cuda", 0)
    chem.init(0)
    ipar = np.zeros(20, np.int32)
    ipar[1], ipar[3] = 1, a.method
    print("%d cells, method %d at INTEGRATE_x's other options, 0 -> 10 s; %d repeats behind one warm-up; ms: median [min .. max]" % (a.cells, a.method, a.repeats))
    for mech in a.mechs:
        V, F, K = W.make_batch(mech, 0, a.cells, dev)

        def timed(f):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f(mech, V, F, K, 0.0, 10.0, ipar)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), out

        yf, ys = timed(chem.rosenbrock_flux)[1], timed(chem.rosenbrock)[1]      # warm-up
        same = yf[0].var.cpu().numpy().tobytes() == ys[0].var.cpu().numpy().tobytes() and bool((yf[0].stats == ys[0].stats).all())
        rows = {"flux": [], "sibling": []}
        for _ in range(a.repeats):
            rows["flux"].append(timed(chem.rosenbrock_flux)[0])
            rows["sibling"].append(timed(chem.rosenbrock)[0])
        fmt = lambda x: "%9.3f [%9.3f .. %9.3f]" % (float(np.median(x)), min(x), max(x))      # noqa: E731
        print("%s: end states and counters of the two sides %s; attempts per cell %.1f" %
              (mech, "identical bit for bit" if same else "DIFFER", float(ys[0].stats[:, 2].double().mean())))
        for side in ("flux", "sibling"):
            print("  %-8s stream %s" % (side, fmt(rows[side])))
        s = np.array(rows["sibling"])
        print("  flux / sibling: %.4f (medians); the sibling's own spread (max - min) / median: %.4f" %
              (np.median(rows["flux"]) / np.median(s), (s.max() - s.min()) / np.median(s)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
