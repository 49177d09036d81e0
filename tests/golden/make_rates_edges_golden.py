#!/usr/bin/env python3
"""Generates tests/golden/rates_edges_{gas,aer,tot}.npz: the edge cases of tests/rates_cases.py (input vectors of Update_RCONST_x that sit on the
guards of the rate laws: zero, -0.0 and negative water-content factors and concentrations, thresholds met exactly, empty and cancelling aerosol
sums, every switch setting, 180 K and 330 K, night, a NaN and an Inf) and the RCONST the COMPILED REFERENCE makes of them (oracle/_ref/libmistra_ref.so:
update_rconst_x_ and the rate laws of kpp.f90, flang -O2 -ffp-contract=off), for tests/test_rates_cases.py (the restatement, CPU) and
tests/test_gpu_rates_edges.py (the device evaluator).  Same pattern as make_rates_golden.py.  Run in the build container (needs the compiled
reference); the fixture is data.  Writes the same bytes every time: the zip members carry a fixed date instead of the time of writing."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle.oracle import Reference  # noqa: E402
import rates_cases  # noqa: E402


def save_npz(path, **arrays):
    """np.savez_compressed without the clock: np.load reads it the same"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zi, buf.getvalue())


def main():
    # (compiler and flags of the reference build; not its date: the same build recipe gives the same file)
    info = "; ".join(l for l in open(os.path.join(HERE, "..", "..", "oracle", "_ref", "BUILD_INFO")).read().split("\n") if l.startswith(("compiler:", "flags:")))
    for mech in rates_cases.MECHS:
        c = rates_cases.cases(mech)
        names = rates_cases.env_info(mech)[0]
        ref = Reference(mech)
        rconst = np.stack([ref.update_rconst(names, e) for e in c["env"]])
        path = os.path.join(HERE, "rates_edges_%s.npz" % mech)
        save_npz(path, env=c["env"], rconst=rconst, names=np.array(c["names"]),
                 provenance=np.array("tests/golden/make_rates_edges_golden.py from tests/rates_cases.py; " + info))
        limit = os.path.getsize(os.path.join(HERE, "rates_%s.npz" % mech))
        print(path, os.path.getsize(path), "bytes (rates_%s.npz: %d);" % (mech, limit), len(c["names"]), "cases;",
              int(np.isnan(rconst).sum()), "NaN,", int(np.isinf(rconst).sum()), "Inf")
        assert os.path.getsize(path) <= limit


if __name__ == "__main__":
    main()
