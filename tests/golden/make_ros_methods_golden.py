#!/usr/bin/env python3
"""Generate tests/golden/ros_methods_<mech>.npz: what the COMPILED reference's Rosenbrock_x (gas.f:777 | aer.f | tot.f) returns for the sets of
tests/ros_methods_py.py — its methods Ros2, Ros4 (as IPAR(4) = 3 and = 0), Rodas3 and Rodas4 at INTEGRATE_x's other options, the same autonomous,
Rodas3 and Rodas4 under four option sets of tests/ros_options_py.py, Rodas3 backward in time and one refused set — on cells 0, n/2, n-1 of
tests/golden/integrate_<mech>.npz over 0 -> 10 s (the backward set: 10 -> 0 s).

Provenance: as tests/golden/make_ros_options_golden.py — oracle/build_ref.sh lib compiles the reference's own Fortran sources into
oracle/_ref/libmistra_ref.so (flang -O2 -ffp-contract=off); this script calls its rosenbrock_x_ through ctypes with FunTemplate_x / JacTemplate_x and
COMMON /GDATA_x/ holding the cell's FIX and RCONST.  Per set and cell it stores VAR, IERR, IPAR(11:18) and RPAR(11:12) as the routine leaves them
(they enter as zeros; a refusal returns before they are written).  The fixtures are DATA.

    python tests/golden/make_ros_methods_golden.py [--check]      --check: compare with the committed files instead of writing them
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ros_methods_py as RM  # noqa: E402
from oracle.oracle import Reference  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_ros_options_golden", os.path.join(HERE, "make_ros_options_golden.py"))
_opt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_opt)      # call(): one Rosenbrock_x call on the compiled reference; to_bytes(): the reproducible .npz

PROVENANCE = ("rosenbrock_x_ of oracle/_ref/libmistra_ref.so (oracle/build_ref.sh lib) on cells 0, n/2, n-1 of integrate_<mech>.npz, 0 -> 10 s (backward: "
              "10 -> 0 s), sets of tests/ros_methods_py.py; tests/golden/make_ros_methods_golden.py")


def record(mech):
    """-> {array name: array}: for every set <name>_var [3, NVAR], <name>_ierr [3], <name>_ipar [3, 8], <name>_rpar [3, 2]"""
    ref = Reference(mech)
    g = np.load(os.path.join(HERE, "integrate_%s.npz" % mech))
    cells = RM.cells_of(g["var_in"].shape[0])
    out = {"cells": np.array(cells, np.int32), "provenance": np.array(PROVENANCE), "sets": np.array(RM.SET_NAMES)}
    for name in RM.SET_NAMES:
        ipar, rpar, atol, rtol, tstart, tend = RM.method_set(mech, name)
        rows = [_opt.call(ref, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, atol, rtol, tstart, tend) for c in cells]
        for i, part in enumerate(("var", "ierr", "ipar", "rpar")):
            out["%s_%s" % (name, part)] = np.array([r[i] for r in rows])
    return out


def main():
    check = "--check" in sys.argv
    for mech in RM.MECHS:
        path = os.path.join(HERE, "ros_methods_%s.npz" % mech)
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
