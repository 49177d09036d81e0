#!/usr/bin/env python3
"""Generate tests/golden/ros_series_<mech>.npz: what the COMPILED reference's Rosenbrock_x (gas.f:777 | aer.f | tot.f) returns when it is called leg by
leg on its own chained state, for the sets of tests/ros_series_py.py — Ros3 at INTEGRATE_x's options over 8 legs, Ros3 over unequal legs without and
with the previous leg's RPAR(12) as the next leg's RPAR(3), Rodas4 at RelTol 1e-7 over 4 legs, Ros2 with vector tolerances over 3 legs, a descending
grid, and Max_no_steps = 3 where every leg ends with IERR = -6 — on cells 0, n/2, n-1 of tests/golden/integrate_<mech>.npz.

Provenance: as tests/golden/make_ros_options_golden.py — oracle/build_ref.sh lib compiles the reference's own Fortran sources into
oracle/_ref/libmistra_ref.so (flang -O2 -ffp-contract=off); this script calls its rosenbrock_x_ through ctypes, once per leg and cell, each call on the
VAR the previous call left, with Tstart and Tend the leg's.  Per set, leg and cell it stores VAR, IERR, IPAR(11:18) and RPAR(11:12) as the routine
leaves them (they enter every call as zeros).  The file holds results, names and the times: the fixtures are DATA.

    python tests/golden/make_ros_series_golden.py [--check]      --check: compare with the committed files instead of writing them
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ros_series_py as RS  # noqa: E402
from oracle.oracle import Reference  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_ros_options_golden", os.path.join(HERE, "make_ros_options_golden.py"))
_opt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_opt)      # call(): one Rosenbrock_x call on the compiled reference; to_bytes(): the reproducible .npz

PROVENANCE = ("rosenbrock_x_ of oracle/_ref/libmistra_ref.so (oracle/build_ref.sh lib) called leg by leg on its own chained state, cells 0, n/2, n-1 of "
              "integrate_<mech>.npz, sets of tests/ros_series_py.py; tests/golden/make_ros_series_golden.py")


def record(mech):
    """-> {array name: array}: for every set <name>_times [nleg + 1], <name>_var [nleg, 3, NVAR], <name>_ierr [nleg, 3], <name>_ipar [nleg, 3, 8],
    <name>_rpar [nleg, 3, 2]"""
    ref = Reference(mech)
    g = np.load(os.path.join(HERE, "integrate_%s.npz" % mech))
    cells = RS.cells_of(g["var_in"].shape[0])
    out = {"cells": np.array(cells, np.int32), "provenance": np.array(PROVENANCE), "sets": np.array(RS.SET_NAMES)}
    for name in RS.SET_NAMES:
        s = RS.series_set(mech, name)

        def one(c):
            def call(y, rpar, t0, t1):
                var, ierr, ip, rp = _opt.call(ref, y, g["fix"][c], g["rconst"][c], s.ipar, rpar, s.atol, s.rtol, t0, t1)
                return var, ierr, ip, rp[0], rp[1]
            return RS.chain(call, g["var_in"][c], s)
        rows = [one(c) for c in cells]
        out[name + "_times"] = s.times
        out[name + "_var"] = np.stack([r[0] for r in rows], axis=1)
        out[name + "_ierr"] = np.stack([r[1] for r in rows], axis=1).astype(np.int32)
        out[name + "_ipar"] = np.stack([r[2] for r in rows], axis=1).astype(np.int32)
        out[name + "_rpar"] = np.stack([np.stack([r[3], r[4]], axis=-1) for r in rows], axis=1)
    return out


def main():
    check = "--check" in sys.argv
    for mech in RS.MECHS:
        path = os.path.join(HERE, "ros_series_%s.npz" % mech)
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
