"""A series of Rosenbrock_x calls with the reaction flux of every leg (mistra_chem_rosenbrock_series_flux_ex), CPU side: the chained
restatement (tests/ros_series_flux_py.py) against the two restatements it is made of, the refusals the four entries make before a device is touched,
the kernel units that hold the VARIANT 11 kernels, and tools/box_series.py --cpu --budget."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ros_flux_py as RF
import ros_series_flux_py as SF
import ros_series_rates_py as SR
from conftest import MECHS, REPO

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.mark.parametrize("mech", MECHS)
def test_restatement_is_the_series_with_rates_plus_the_flux_of_each_leg_alone(mech):
    """On every set of tests/ros_series_rates_py.py: VAR, IERR, the counters, Texit and Hexit of every leg are the bytes of that module's restatement;
    leg k's flux row is the bytes of ros_flux_py.rosenbrock called ALONE on leg k's start state with leg k's rows and the leg's RPAR (nothing is carried
    from one leg's sum into the next).  The Max_no_steps set has a non-zero flux in its failed legs — the sum closed at Texit — and the leg behind a
    failed leg equals its stand-alone call like any other."""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    want = SR.restated(mech)
    got = SF.restated(mech)
    o, diag = Oracle(mech), mechtab.load(mech).diag
    V, LF, LK = SF.ramp(mech)
    for name in SF.SET_NAMES:
        for i in range(5):
            assert got[name][i].tobytes() == want[name][i].tobytes(), (name, i)
        s, _, _ = SF.series_set(mech, name)
        F, K = SF.leg_rows(name, mech, LF, LK)
        flux, start, rpars = got[name][5:8]
        nleg = len(s.times) - 1
        assert flux.shape == (nleg, V.shape[0], o.nreact)
        assert start[0].tobytes() == V.tobytes() and start[1:].tobytes() == got[name][0][:-1].tobytes()
        for k in range(nleg):
            for c in (0, V.shape[0] - 1):      # (the first and the last cell: every leg of both)
                f, kk = (F[k, c] if F.ndim == 3 else F[c]), (K[k, c] if K.ndim == 3 else K[c])
                alone = RF.rosenbrock(o, diag, start[k, c], f, kk, s.ipar, rpars[k, c], s.atol, s.rtol, float(s.times[k]), float(s.times[k + 1]))
                assert alone[5].tobytes() == flux[k, c].tobytes(), (name, k, c)
                assert alone[0].tobytes() == got[name][0][k, c].tobytes() and alone[1] == got[name][1][k, c]
        assert np.isfinite(flux).all()
        if name in SF.FAILING_SETS:
            assert (got[name][1] == -6).all() and all(np.abs(flux[k, c]).max() > 0.0 for k in range(nleg) for c in range(V.shape[0])), name
    # the carried first step reaches the flux: leg 0 equal, a later leg not
    a, b = got["ros3"][5], got["ros3_carry"][5]
    assert a[0].tobytes() == b[0].tobytes() and a[-1].tobytes() != b[-1].tobytes()


def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """A null flux_series, nleg out of range, a repeated time, a bad rconst_legs, a bad ntol, an unknown mechanism and both user slots: each fails with
    its own text through all four entries, with every data pointer NULL and no device initialised — never the 'no HIP device' path.  (Fails where the
    library has no series-flux entries: the symbols do not exist.)"""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    for form in ("ex", "device", "cells_ex", "cells_device"):
        assert hasattr(L, "mistra_chem_rosenbrock_series_flux_" + form), form
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    ipar = np.array([0, 1, 0, 2] + [0] * 16, np.int32)
    out, fl = np.zeros(4), np.zeros(4)      # never written: every call below is refused

    def entries(mid, nleg, times, flux, nlr=1, nlf=1, ntol=nvar):
        tp, vs = None if times is None else _P(times), _P(out)
        fp = None if flux is None else _P(flux)
        head = (mid, 1, None, None, None, nlr, nlf, nleg, tp)
        dv, df = C.cast(vs, C.c_void_p), None if fp is None else C.cast(fp, C.c_void_p)
        return {
            "ex": lambda: L.mistra_chem_rosenbrock_series_flux_ex(*head, _P(tol), _P(tol), _P(rpar), _P(ipar), 0, None, vs, None, None, None, fp),
            "device": lambda: L.mistra_chem_rosenbrock_series_flux_device(*head, _P(tol), _P(tol), _P(rpar), _P(ipar), dv, None, None, None, 0, None, None, df),
            "cells_ex": lambda: L.mistra_chem_rosenbrock_series_flux_cells_ex(*head, _P(tol), _P(tol), ntol, _P(rpar), _P(ipar), 0, None, vs, None, None, None, fp),
            "cells_device": lambda: L.mistra_chem_rosenbrock_series_flux_cells_device(*head, C.cast(_P(tol), C.c_void_p), C.cast(_P(tol), C.c_void_p), ntol,
                                                                                      _P(rpar), _P(ipar), dv, None, None, None, 0, None, None, df),
        }

    def refused(calls, text):
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    good = np.array([0.0, 1.0, 2.0, 3.0])
    long_times = np.arange(chem.SERIES_MAX_LEGS + 2, dtype=np.float64)
    refused(entries(0, 3, good, None), "series: null flux_series pointer (flux_series: [nleg][ncell][NREACT])")
    refused(entries(0, 0, good, fl), "nleg = 0: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, chem.SERIES_MAX_LEGS + 1, long_times, fl), "nleg = 4097: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, 2, np.array([0.0, 1.0, 1.0]), fl), "times[2] repeats times[1]")
    for bad in (0, 2, 4, -1):
        refused(entries(0, 3, good, fl, nlr=bad), "series: rconst_legs = %d: rconst has 1 block (shared by all legs) or nleg = 3 blocks" % bad)
    refused(entries(0, 3, good, fl, nlf=2), "series: fix_legs = 2: fix has 1 block (shared by all legs) or nleg = 3 blocks")
    cells = {k: v for k, v in entries(0, 2, good, fl, ntol=2).items() if "cells" in k}
    refused(cells, "ntol = 2: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    refused(entries(9, 2, good, fl), "unknown mechanism id")
    names = chem.user_mechs()
    assert len(names) == 2      # the library this repository builds has both
    for i in range(2):          # both user slots: the slot's existing text of the flux entries
        refused(entries(3 + i, 2, good, fl), "user mechanism slot %d (%s) has no reaction-flux entries: a user slot integrates" % (i, names[i]))
    # the Python surface passes the refusals on, without init()
    V, LF, LK = SF.ramp("gas")
    with pytest.raises(chem.MistraChemError, match="rconst_legs = 4: rconst has 1 block .* or nleg = 2 blocks"):
        chem.rosenbrock_series_flux("gas", V, LF[0], LK, [0.0, 1.0, 2.0])
    for times, text in (([0.0], "nleg = 0"), ([0.0, 1.0, 1.0], "repeats"), (np.arange(chem.SERIES_MAX_LEGS + 2.0), "nleg = 4097")):
        with pytest.raises(chem.MistraChemError, match=text):
            chem.rosenbrock_series_flux("gas", V, LF[0], LK[0], times)
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_series_flux_cells("gas", V, LF, LK, SF.TIMES, None, None, np.ones((3, 5)), np.ones((3, 5)))
    with pytest.raises(chem.MistraChemError, match="unknown mechanism"):
        chem.rosenbrock_series_flux("nope", V, LF, LK, SF.TIMES)
    for i in range(2):
        nv, nf, nr, _ = chem.DIMS[names[i]]
        with pytest.raises(chem.MistraChemError, match="has no reaction-flux entries"):
            chem.rosenbrock_series_flux(names[i], np.ones((1, nv)), np.ones((1, nf)), np.ones((1, nr)), [0.0, 1.0])


def test_the_kernels_live_in_the_method_and_trace_units():
    """No unit of their own: the unit list is what it was (45).  The gas trace unit holds the VARIANT 4, 8, 9, 10 and 11 kernels, the gas Ros2 method unit
    the VARIANT 3, 10 and 11 kernels; both pass the register-ring and hazard reports the build runs on every unit."""
    from mistra_amd import build as B
    assert len(B.VARIANT_UNITS) == 45 and sorted(B.VARIANT_METHODS) == [3, 4, 5, 6]
    with pytest.raises(ValueError, match="no kernel unit"):
        B.unit_build(B.Unit(11, 0, 2))
    for unit, method, variants in ((B.Unit(4, 0, 2), 2, (4, 8, 9, 10, 11)), (B.Unit(3, 0, 1), 1, (3, 10, 11))):
        rep = B.ring_register_report(unit=unit)
        assert B.isa_hazard_report(rep["__isa_text__"]) == []
        kernels = sorted(k for k in rep if "ros3_integrate_kernel" in k)
        assert kernels == sorted("_ZN6mistra21ros3_integrate_kernelINS_9GasTraitsELi64ELi%dELi%dEEEvNS_10KernelArgsE" % (v, method) for v in variants), kernels


def test_tool_box_series_budget_on_the_cpu():
    """tools/box_series.py gas --cpu --budget: per leg and species a table of the top producing and destroying reactions, the gross turnover and the net
    change.  Asserted: one block per leg and species, well-formed numbers, production >= 0 >= destruction, and net = production + destruction as printed."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "box_series.py"), "gas", "--cpu", "--legs", "2", "--cells", "1", "--budget", "33,49",
                        "--top", "2"], check=True, capture_output=True, text=True, timeout=300)
    assert "CPU restatement" in r.stdout
    heads = [l.split() for l in r.stdout.split("\n") if l.startswith("budget ")]
    # budget leg K species I | production P destruction D turnover G net N
    assert [(int(h[2]), int(h[4])) for h in heads] == [(0, 33), (0, 49), (1, 33), (1, 49)], r.stdout
    for h in heads:
        p, d, g, n = (float(h[i]) for i in (7, 9, 11, 13))
        assert np.isfinite([p, d, g, n]).all() and p >= 0.0 >= d and abs(g - (p - d)) <= 1e-8 * max(g, 1e-300) and abs(n - (p + d)) <= 1e-8 * max(g, 1e-300), h
    rows = [l.split() for l in r.stdout.split("\n") if l.startswith(("  + ", "  - "))]
    assert rows and all(len(x) == 4 and x[1] == "reaction" and int(x[2]) >= 1 and np.isfinite(float(x[3])) for x in rows), r.stdout
    assert all((float(x[3]) > 0.0) == (x[0] == "+") for x in rows)
