#!/usr/bin/env python3
"""Generate tests/golden/ros_series_rates_<mech>.npz: what the COMPILED reference's Rosenbrock_x (gas.f:777 | aer.f | tot.f) returns when it is called
leg by leg on its own chained state with COMMON /GDATA_x/ holding the LEG's FIX and RCONST — Update_RCONST_x + INTEGRATE_x, four times — for the sets
of tests/ros_series_rates_py.py: Ros3, Ros3 with the previous leg's RPAR(12) as the next leg's RPAR(3), Rodas4, Ros2 with FIX the leg's own and the
rate constants shared, and Ros3 with Max_no_steps = 3 where every leg ends with IERR = -6.  The rows are the ramp of that module: cells 0, n/2, n-1 of
tests/golden/integrate_<mech>.npz blended into cells 0, n/2, n-1 of integrate_<mech>_day.npz at w = 0, .25, .5, 1 over times 0, 2.5, 5, 7.5, 10.
No set had to be replaced by a shorter one: no re-association of the oracle moves IERR or a counter in any leg of any of them
(tests/test_ros_series_rates.py).

Provenance: as tests/golden/make_ros_series_golden.py — oracle/build_ref.sh lib compiles the reference's own Fortran sources into
oracle/_ref/libmistra_ref.so (flang -O2 -ffp-contract=off); this script calls its rosenbrock_x_ through ctypes, once per leg and cell.  Per set, leg
and cell it stores VAR, IERR, IPAR(11:18) and RPAR(11:12) as the routine leaves them, and once per mechanism the input rows of the legs (leg_fix,
leg_rconst) and the times.  The file holds results, input rows and names: the fixtures are DATA.

    python tests/golden/make_ros_series_rates_golden.py [--check]      --check: compare with the committed files instead of writing them
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ros_series_rates_py as SR  # noqa: E402
from oracle.oracle import Reference  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_ros_options_golden", os.path.join(HERE, "make_ros_options_golden.py"))
_opt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_opt)      # call(): one Rosenbrock_x call on the compiled reference; to_bytes(): the reproducible .npz

PROVENANCE = ("rosenbrock_x_ of oracle/_ref/libmistra_ref.so (oracle/build_ref.sh lib) called leg by leg on its own chained state with the leg's FIX and "
              "RCONST, the ramp and the sets of tests/ros_series_rates_py.py; tests/golden/make_ros_series_rates_golden.py")


def record(mech):
    """-> {array name: array}: times [nleg + 1], leg_fix [nleg, 3, NFIX], leg_rconst [nleg, 3, NREACT], and for every set <name>_var [nleg, 3, NVAR],
    <name>_ierr [nleg, 3], <name>_ipar [nleg, 3, 8], <name>_rpar [nleg, 3, 2]"""
    ref = Reference(mech)
    V, LF, LK = SR.ramp(mech)
    out = {"provenance": np.array(PROVENANCE), "sets": np.array(SR.SET_NAMES), "times": np.array(SR.TIMES), "leg_fix": LF, "leg_rconst": LK}
    for name in SR.SET_NAMES:
        s, _, _ = SR.series_set(mech, name)
        F, K = SR.leg_rows(name, mech, LF, LK)

        def one(c):
            def call(y, f, k, rpar, t0, t1):
                var, ierr, ip, rp = _opt.call(ref, y, f, k, s.ipar, rpar, s.atol, s.rtol, t0, t1)
                return var, ierr, ip, rp[0], rp[1]
            return SR.chain_rates(call, V[c], s, F[:, c] if F.ndim == 3 else F[c], K[:, c] if K.ndim == 3 else K[c])
        rows = [one(c) for c in range(V.shape[0])]
        out[name + "_var"] = np.stack([r[0] for r in rows], axis=1)
        out[name + "_ierr"] = np.stack([r[1] for r in rows], axis=1).astype(np.int32)
        out[name + "_ipar"] = np.stack([r[2] for r in rows], axis=1).astype(np.int32)
        out[name + "_rpar"] = np.stack([np.stack([r[3], r[4]], axis=-1) for r in rows], axis=1)
    return out


def main():
    check = "--check" in sys.argv
    for mech in SR.MECHS:
        path = os.path.join(HERE, "ros_series_rates_%s.npz" % mech)
        raw = _opt.to_bytes(record(mech))
        if check:
            same = os.path.exists(path) and open(path, "rb").read() == raw
            print("%s: %s" % (os.path.basename(path), "identical" if same else "DIFFERS"))
            if not same:
                sys.exit(1)
        else:
            open(path, "wb").write(raw)
            print("%s: %d bytes" % (os.path.basename(path), len(raw)))


if __name__ == "__main__":
    main()
