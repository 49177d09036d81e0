#!/usr/bin/env python3
"""Generate tests/golden/ros_options_<mech>.npz: what the COMPILED reference's Rosenbrock_x (gas.f:777 | aer.f | tot.f) returns for the option sets
of tests/ros_options_py.py — the nine sets that run, the six it refuses and the one with a zero tolerance it never looks at — on cells 0, n/2, n-1
of tests/golden/integrate_<mech>.npz over 0 -> 10 s.

Provenance: oracle/build_ref.sh lib compiles the reference's own Fortran sources into oracle/_ref/libmistra_ref.so (flang -O2 -ffp-contract=off); this
script calls its rosenbrock_x_ through ctypes with FunTemplate_x / JacTemplate_x, as oracle/oracle.py: Reference.rosenbrock does for IPAR(3), with
COMMON /GDATA_x/ holding the cell's FIX and RCONST.  Per set and cell it stores VAR, IERR, IPAR(11:18) and RPAR(11:12) as the routine leaves them
(IPAR(11:18) and RPAR(11:12) enter as zeros, as INTEGRATE_x passes them; a refusal returns before they are written).  The fixtures are DATA.

    python tests/golden/make_ros_options_golden.py [--check]      --check: compare with the committed files instead of writing them
"""
import ctypes as C
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ros_options_py as R  # noqa: E402
from oracle.oracle import SFX, Reference, _d, _i  # noqa: E402

PROVENANCE = ("rosenbrock_x_ of oracle/_ref/libmistra_ref.so (oracle/build_ref.sh lib) on cells 0, n/2, n-1 of integrate_<mech>.npz, 0 -> 10 s, option sets "
              "of tests/ros_options_py.py; tests/golden/make_ros_options_golden.py")


def call(ref, var, fix, rconst, ipar, rpar, atol, rtol, tin=R.TIN, tout=R.TOUT):
    g, s = ref.gdata, SFX[ref.mech]
    np.ctypeslib.as_array(g.c)[:ref.nvar] = var
    np.ctypeslib.as_array(g.c)[ref.nvar:] = fix
    np.ctypeslib.as_array(g.rconst)[:] = rconst
    y = np.array(var, np.float64)
    ip, rp = np.array(ipar, np.int32), np.array(rpar, np.float64)
    at, rt = np.array(atol, np.float64), np.array(rtol, np.float64)
    t0, t1, ierr = C.c_double(tin), C.c_double(tout), C.c_int32(0)
    getattr(ref.lib, "rosenbrock_%s_" % s)(_d(y), C.byref(t0), C.byref(t1), _d(at), _d(rt), getattr(ref.lib, "funtemplate_%s_" % s),
                                           getattr(ref.lib, "jactemplate_%s_" % s), _d(rp), _i(ip), C.byref(ierr))
    return y, ierr.value, ip[10:18].copy(), rp[10:12].copy()


def record(mech):
    """-> {array name: array}: for every set <name>_var [3, NVAR], <name>_ierr [3], <name>_ipar [3, 8], <name>_rpar [3, 2]"""
    ref = Reference(mech)
    g = np.load(os.path.join(HERE, "integrate_%s.npz" % mech))
    cells = R.cells_of(g["var_in"].shape[0])
    out = {"cells": np.array(cells, np.int32), "provenance": np.array(PROVENANCE)}
    for name in R.SET_NAMES + R.REFUSED_NAMES + R.ACCEPTED_EXTRA:
        ipar, rpar, atol, rtol = R.any_set(mech, name)
        rows = [call(ref, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, atol, rtol) for c in cells]
        for i, part in enumerate(("var", "ierr", "ipar", "rpar")):
            out["%s_%s" % (name, part)] = np.array([r[i] for r in rows])
    return out


def to_bytes(arrays):
    """the .npz as bytes, reproducibly (np.savez stamps no times into its members)"""
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def main():
    check = "--check" in sys.argv
    sys.stdout.flush()
    for mech in R.MECHS:
        path = os.path.join(HERE, "ros_options_%s.npz" % mech)
        raw = to_bytes(record(mech))
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
