#!/usr/bin/env python3
"""Generates tests/golden/drive_edges_{gas,aer,tot}.npz: the budget states of tests/drive_cases.py (NB seeded states whose products round, plus states with a
species at +0.0 / -0.0 / negative / NaN, an Inf rate constant, products that underflow and overflow, dt = 10 / 0 / 0.1, cumulative columns starting from
zero, seeded values and Inf, the unset accumulated slot non-zero on entry) and the bg / bgs the COMPILED REFERENCE makes of them (oracle/_ref/libmistra_ref.so:
bud_gas_ / bud_aer_ / bud_tot_ and bud_s_gas_ / bud_s_aer_ / bud_s_tot_, flang -O2 -ffp-contract=off: the formula lists of bud_x.f and bud_s_x.f, not the
mechanism tables), for tests/test_drive_cases.py (the restatement, CPU) and tests/test_gpu_drive_edges.py (budgets_kernel).  Same pattern as
make_rates_edges_golden.py.  The fixture holds recorded results, the names of the states and a SHA-256 of the inputs tests/drive_cases.py generates — no
inputs: the tests regenerate them and compare the hash.  Where both columns of bg would make a file larger than the mechanism's drive_<mech>.npz, only the
instantaneous one is stored (`bg1`), after checking that the reference's cumulative column is in + dt*inst bit for bit.  Run in the build container (needs
the compiled reference).  Writes the same bytes every time."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from oracle.oracle import Reference  # noqa: E402
import drive_cases  # noqa: E402
from make_rates_edges_golden import save_npz  # noqa: E402

MAX_FILE = 1 << 20


def main():
    info = "; ".join(l for l in open(os.path.join(HERE, "..", "..", "oracle", "_ref", "BUILD_INFO")).read().split("\n") if l.startswith(("compiler:", "flags:")))
    for mech in drive_cases.MECHS:
        c = drive_cases.budget_cases(mech)
        ref = Reference(mech)
        out = [ref.budgets(c["C"][i], c["rconst"][i], float(c["dt"][i]), c["bg_in"][i], c["bgs_in"][i]) for i in range(len(c["names"]))]
        bg, bgs = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        path = os.path.join(HERE, "drive_edges_%s.npz" % mech)
        limit = min(os.path.getsize(os.path.join(HERE, "drive_%s.npz" % mech)), MAX_FILE)
        common = dict(bgs=bgs, names=np.array(c["names"]), input_sha256=np.array(drive_cases.input_sha256(mech)),
                      provenance=np.array("tests/golden/make_drive_edges_golden.py from tests/drive_cases.py (seed %d, NB %d); " % (drive_cases.SEED, drive_cases.NB) + info))
        save_npz(path, bg=bg, **common)
        form = "both columns of bg"
        if os.path.getsize(path) > limit:
            with np.errstate(all="ignore"):
                cum = c["bg_in"][:, :, 1] + c["dt"][:, None] * bg[:, :, 0]
            assert drive_cases.same(cum, bg[:, :, 1]), "the reference's cumulative bg is not in + dt*inst: keep both columns"
            save_npz(path, bg1=np.ascontiguousarray(bg[:, :, 0]), **common)
            form = "the instantaneous column of bg"
        print(path, os.path.getsize(path), "bytes (drive_%s.npz: %d), %s;" % (mech, limit, form), len(c["names"]), "states;",
              int(np.isnan(bg).sum() + np.isnan(bgs).sum()), "NaN,", int(np.isinf(bg).sum() + np.isinf(bgs).sum()), "Inf")
        assert os.path.getsize(path) <= limit


if __name__ == "__main__":
    main()
