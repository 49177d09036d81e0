#!/usr/bin/env python3
"""Generate tests/golden/ros_celltol_<mech>.npz: what the COMPILED reference's Rosenbrock_x (gas.f:777 | aer.f | tot.f) returns for the sets of
tests/ros_celltol_py.py — tolerances that differ from cell to cell — called ONCE PER CELL with that cell's row, on cells 0, n/2, n-1 of
tests/golden/integrate_<mech>.npz over 0 -> 10 s.

Provenance: as tests/golden/make_ros_options_golden.py — oracle/build_ref.sh lib compiles the reference's own Fortran sources into
oracle/_ref/libmistra_ref.so (flang -O2 -ffp-contract=off); this script calls its rosenbrock_x_ through ctypes (make_ros_options_golden.call).  Per set
and cell it stores VAR, IERR, IPAR(11:18) and RPAR(11:12) as the routine leaves them (they enter as zeros; a refusal returns before they are
written).  The fixtures are DATA.

    python tests/golden/make_ros_celltol_golden.py [--check]      --check: compare with the committed files instead of writing them
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ros_celltol_py as RC  # noqa: E402
from oracle.oracle import Reference  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_ros_options_golden", os.path.join(HERE, "make_ros_options_golden.py"))
_opt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_opt)      # call(): one Rosenbrock_x call on the compiled reference; to_bytes(): the reproducible .npz

PROVENANCE = ("rosenbrock_x_ of oracle/_ref/libmistra_ref.so (oracle/build_ref.sh lib), one call per cell with the cell's tolerance row, on cells 0, n/2, "
              "n-1 of integrate_<mech>.npz, 0 -> 10 s, sets of tests/ros_celltol_py.py; tests/golden/make_ros_celltol_golden.py")


def record(mech):
    """-> {array name: array}: for every set <name>_var [3, NVAR], <name>_ierr [3], <name>_ipar [3, 8], <name>_rpar [3, 2]"""
    ref = Reference(mech)
    g = np.load(os.path.join(HERE, "integrate_%s.npz" % mech))
    cells = list(RC.cells_of(g["var_in"].shape[0]))
    nvar = g["var_in"].shape[1]
    out = {"cells": np.array(cells, np.int32), "provenance": np.array(PROVENANCE), "sets": np.array(RC.SET_NAMES)}
    for name in RC.SET_NAMES:
        ipar, rpar, atol, rtol = RC.celltol_set(mech, name, g["var_in"][cells])
        rows = [_opt.call(ref, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, RC.full_row(atol[i], nvar), RC.full_row(rtol[i], nvar))
                for i, c in enumerate(cells)]
        for i, part in enumerate(("var", "ierr", "ipar", "rpar")):
            out["%s_%s" % (name, part)] = np.array([r[i] for r in rows])
    return out


def main():
    check = "--check" in sys.argv
    for mech in RC.MECHS:
        path = os.path.join(HERE, "ros_celltol_%s.npz" % mech)
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
