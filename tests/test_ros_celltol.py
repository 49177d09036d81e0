"""Tolerances per cell, CPU side: the fixture recorded from the compiled reference called once per cell with the cell's row
(tests/golden/ros_celltol_<mech>.npz), the restatement per cell (tests/ros_celltol_py.py), the bounds of the GPU tests (tests/ros_celltol_bounds.py),
what the entries refuse before they look for a device, the host formula of cell_atol and tools/step_control.py --atol-rel --yardstick."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ros_celltol_py as RC
from conftest import MECHS, REPO, load_golden
from oracle.oracle import Reference

GOLDEN = os.path.join(REPO, "tests", "golden")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def fixture(mech):
    return dict(np.load(os.path.join(GOLDEN, "ros_celltol_%s.npz" % mech)))


def test_the_sets_are_the_ones_the_fixture_needs():
    assert len(RC.SET_NAMES) == 9 and set(RC.BAD_CELLS) <= set(RC.SET_NAMES) and set(RC.TRACE_SETS) <= set(RC.SET_NAMES)
    assert [RC.method_of(n) for n in RC.SET_NAMES] == [2, 2, 2, 4, 5, 1, 2, 2, 2]
    for mech in MECHS:
        z = fixture(mech)
        assert list(z["sets"]) == list(RC.SET_NAMES)
        assert os.path.getsize(os.path.join(GOLDEN, "ros_celltol_%s.npz" % mech)) <= 100 * 1024
        g = load_golden(mech)
        V = g["var_in"][list(RC.cells_of(g["var_in"].shape[0]))]
        nvar = V.shape[1]
        shapes = {n: RC.celltol_set(mech, n, V)[2].shape for n in RC.SET_NAMES}
        assert shapes["rel_1e-13"] == (3, 1) and shapes["rel_1e-10_ntolN"] == (3, nvar) and shapes["vector_rows"] == (3, nvar)
        ipar, _, atol, rtol = RC.celltol_set(mech, "rel_1e-10_ntolN", V)
        assert ipar[1] == 1 and not atol[:, 1:].any() and not rtol[:, 1:].any() and (atol[:, 0] > 0).all()
        # the rows differ from cell to cell: that is what the sets are for
        for n in ("rel_1e-13", "vector_rows"):
            a = RC.celltol_set(mech, n, V)[2]
            assert len({a[c].tobytes() for c in range(3)}) == 3, n
        iv, _, av, _ = RC.celltol_set(mech, "bad_cell_vector", V)
        isc, _, asc, _ = RC.celltol_set(mech, "bad_cell_scalar", V)
        assert iv[1] == 0 and isc[1] == 1 and av.tobytes() == asc.tobytes() and av[1, 50] == 0.0 and (av[[0, 2]] > 0).all()
        assert RC.celltol_set(mech, "bad_rtol_cell", V)[3].ravel().tolist() == [1.0e-3, 1.0e-3, 1.0]


@pytest.mark.parametrize("mech", MECHS)
def test_restatement_per_cell_equals_the_compiled_rosenbrock(mech):
    """Bit for bit on every (set, cell): VAR, IERR, IPAR(11:18), Texit, Hexit.  The refused cells are the ones BAD_CELLS names and leave as a refusal
    leaves; every other cell runs; the sets are told apart by their counters where the mechanism reacts to the tolerances at all."""
    g, z = load_golden(mech), fixture(mech)
    cells = list(RC.cells_of(g["var_in"].shape[0]))
    assert np.array_equal(z["cells"], cells)
    r = RC.restated(mech, g)
    for name in RC.SET_NAMES:
        var, ierr, st, te, he = r[name]
        assert np.array_equal(ierr, z[name + "_ierr"]), name
        assert np.array_equal(st, z[name + "_ipar"]), name
        assert var.tobytes() == z[name + "_var"].tobytes(), name
        assert np.array_equal(te, z[name + "_rpar"][:, 0]) and np.array_equal(he, z[name + "_rpar"][:, 1]), name
        bad = RC.BAD_CELLS.get(name, ())
        for c in range(3):
            if c in bad:
                assert ierr[c] == -5 and var[c].tobytes() == g["var_in"][cells[c]].tobytes() and not st[c].any() and te[c] == 0.0 and he[c] == 0.0, (name, c)
            else:
                assert ierr[c] == 1 and st[c, 2] > 0, (name, c)
    # a cell beside a refused one is the cell of the set without the zero
    for c in (0, 2):
        assert z["bad_cell_vector_var"][c].tobytes() == z["vector_rows_var"][c].tobytes()
    if mech != "gas":      # (gas takes its seven steps whatever the tolerance)
        assert not np.array_equal(z["rel_1e-13_ipar"], z["rel_1e-10_ntolN_ipar"]) and not np.array_equal(z["vector_rows_ipar"], z["bad_cell_scalar_ipar"])
    # the trace's restatement per cell gives the same results on its sets
    t = RC.traced(mech, g, ("rel_1e-13",))["rel_1e-13"]
    for c in range(3):
        assert t[c][0].tobytes() == z["rel_1e-13_var"][c].tobytes() and np.array_equal(t[c][2], z["rel_1e-13_ipar"][c])


@pytest.mark.skipif(not Reference.available(), reason="compiled reference (oracle/_ref) not present")
def test_fixture_regenerates_to_the_committed_files():
    """tests/golden/make_ros_celltol_golden.py on the compiled reference gives the committed files, byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ros_celltol_golden", os.path.join(GOLDEN, "make_ros_celltol_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for mech in MECHS:
        raw = mod._opt.to_bytes(mod.record(mech))
        assert raw == open(os.path.join(GOLDEN, "ros_celltol_%s.npz" % mech), "rb").read(), mech


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_celltol_bounds.py: no re-association of the oracle changes IERR or the counters on any (set, cell) of the fixture — so none is left
    out of the GPU comparison; the constants are within [10x, 100x] of the spread measured now, or are the floor.  Measured: VAR gas 2.75e-16, aer
    1.45e-6, tot 3.73e-8; Texit / Hexit gas 0, aer 9.69e-5, tot 3.59e-8."""
    import parity_bounds as pb
    import ros_celltol_bounds as cb
    s_var, s_th, moved = cb.measure_spread(mech, load_golden(mech))
    print("%s: VAR spread %.3e, exit time / last step size spread %.3e" % (mech, s_var, s_th))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    pb.check_constant("CELLTOL_RTOL[%s]" % mech, cb.CELLTOL_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("CELLTOL_TH_RTOL[%s]" % mech, cb.CELLTOL_TH_RTOL[mech], s_th, floor=pb.PARITY_FLOOR)


@pytest.mark.parametrize("mech", MECHS)
def test_trace_bounds_cover_the_sets_they_are_used_on(mech):
    """tests/ros_trace_bounds.py is used as it is: on every (mechanism, set) of ros_celltol_bounds.TRACE_RECORD_SETS 10x the restated records' own
    movement lies inside its constants, and no variant changes a record count, code or species there."""
    import ros_celltol_bounds as cb
    import ros_trace_bounds as tb
    for name in cb.TRACE_RECORD_SETS[mech]:
        assert name in RC.TRACE_SETS
        (s_t, s_h, s_err, s_share), moved = cb.measure_trace_spread(mech, load_golden(mech), name)
        print("%s %s: T %.3e, H %.3e, Err %.3e, share %.3e" % (mech, name, s_t, s_h, s_err, s_share))
        assert not moved, moved
        assert 10.0 * s_t <= tb.TRACE_T_TOL[mech] and 10.0 * s_h <= tb.TRACE_H_RTOL[mech], name
        assert 10.0 * s_err <= tb.TRACE_ERR_RTOL[mech] and 10.0 * s_share <= tb.TRACE_SHARE_TOL[mech], name


def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """ntol, NULL tolerance arrays, a negative cell count, cell_atol's factor and floor, and what a user slot does not have: each fails with its own
    text through all four cells entries, with every data pointer NULL and no device initialised — never the 'no HIP device' or an unknown-symbol path."""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    scalar, vector = np.array([0, 1, 0, 2] + [0] * 16, np.int32), np.array([0, 0, 0, 2] + [0] * 16, np.int32)

    def entries(mid, ncell, at, rt, ntol, ipar):
        head = (mid, ncell, None, None, None, 0.0, 10.0, at, rt, ntol, _P(rpar), None if ipar is None else _P(ipar))
        return {
            "cells_ex": lambda: L.mistra_chem_rosenbrock_cells_ex(*head, None, None, None, None),
            "cells_device": lambda: L.mistra_chem_rosenbrock_cells_device(*head, None, None, None, None, None, None),
            "trace_cells_ex": lambda: L.mistra_chem_rosenbrock_trace_cells_ex(*head, None, None, None, None, 0, None, None, None, None),
            "trace_cells_device": lambda: L.mistra_chem_rosenbrock_trace_cells_device(*head, None, None, None, None, None, None, 0, None, None, None, None),
        }

    def refused(calls, text):
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    for ntol in (0, 2, nvar + 1):
        refused(entries(0, 1, _P(tol), _P(tol), ntol, scalar), "ntol = %d: a tolerance row holds 1 or NVAR = %d entries" % (ntol, nvar))
    refused(entries(0, 1, _P(tol), _P(tol), 1, vector), "vector tolerances (ipar[1] = 0) need rows of NVAR = %d entries, ntol = 1" % nvar)
    refused(entries(0, 1, None, _P(tol), nvar, scalar), "null tolerance array")
    refused(entries(0, 1, _P(tol), None, nvar, scalar), "null tolerance array")
    refused(entries(0, -1, _P(tol), _P(tol), nvar, scalar), "negative cell count")
    refused(entries(9, 1, _P(tol), _P(tol), nvar, scalar), "unknown mechanism id")
    refused(entries(0, 1, _P(tol), _P(tol), nvar, None), "null options pointer")
    for factor, floor, text in ((0.0, 1e-30, "factor"), (-1.0, 1e-30, "factor"), (np.nan, 1e-30, "factor"), (1e-13, 0.0, "floor"), (1e-13, np.inf, "floor")):
        for mid in (0, 3):
            assert L.mistra_chem_cell_atol_device(mid, 1, None, factor, floor, None, None) != 0
            assert ("cell_atol: %s must be finite and positive" % text) in L.mistra_chem_last_error().decode()
        with pytest.raises(chem.MistraChemError, match="cell_atol: %s must be finite and positive" % text):
            chem.cell_atol("gas", np.ones((1, nvar)), factor, floor)
    # a user slot: Ros3 is its only method and it has no trace — the slot's text, as its existing entries give it
    for i, name in enumerate(chem.user_mechs()):
        mid = 3 + i
        nv = chem.DIMS[name][0]
        t = np.full((1, nv), 1.0e-3)
        rodas3 = np.array([0, 1, 0, 4] + [0] * 16, np.int32)
        slot_text = "user mechanism slot %d (%s) has no " % (i, name)
        e = entries(mid, 1, _P(t), _P(t), nv, rodas3)
        refused({k: e[k] for k in ("cells_ex", "cells_device")}, slot_text + "kernel for this Rosenbrock method")
        e = entries(mid, 1, _P(t), _P(t), nv, scalar)
        refused({k: e[k] for k in ("trace_cells_ex", "trace_cells_device")}, slot_text + "step-control trace")
    # the Python surface: the shapes it can tell without the library
    g = load_golden("gas")
    V, F, K = g["var_in"][:2], g["fix"][:2], g["rconst"][:2]
    with pytest.raises(chem.MistraChemError, match="atol / rtol"):
        chem.rosenbrock_cells("gas", V, F, K, 0.0, 10.0, None, None, np.ones(2), np.ones(2))
    with pytest.raises(chem.MistraChemError, match="atol / rtol"):
        chem.rosenbrock_cells("gas", V, F, K, 0.0, 10.0, None, None, np.ones((3, 1)), np.ones((3, 1)))
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_cells("gas", V, F, K, 0.0, 10.0, None, None, np.ones((2, 5)), np.ones((2, 5)))
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_trace_cells("gas", V, F, K, 0.0, 10.0, None, None, np.ones((2, 5)), np.ones((2, 5)))


@pytest.mark.parametrize("mech", MECHS)
def test_cell_atol_host_formula_on_the_edge_rows(mech):
    """chem.cell_atol on numpy arrays: max(floor, factor * max |v|) as the header states it, on every kind of edge row — NaN ignored, all zero and
    -0.0 give the floor, negative values count by magnitude, an Inf stays an Inf — bit for bit against the formula written in plain Python and
    against the restatement the issue of the device kernel is held to."""
    from mistra_amd import chem
    nvar = chem.DIMS[mech][0]
    v = RC.atol_edge_rows(nvar, 27)
    for factor, floor in ((1.0e-13, 1.0e-30), (1.0e-16, 1.0e-3), (0.3, 1.0e-300)):
        got = chem.cell_atol(mech, v, factor, floor)
        assert got.shape == (27, 1) and got.dtype == np.float64
        assert got.tobytes() == RC.cell_atol_plain(v, factor, floor).tobytes()
        with np.errstate(invalid="ignore"):
            want = np.array([max(floor, factor * np.fmax.reduce(np.abs(row))) for row in v]).reshape(-1, 1)
        assert got.tobytes() == want.tobytes()
        kinds = [RC.ATOL_EDGE_KINDS[c % 9] for c in range(27)]
        for c, kind in enumerate(kinds):
            if kind in ("all_zero", "minus_zero"):
                assert got[c, 0] == floor
            elif kind == "inf":
                assert np.isinf(got[c, 0])
            elif kind in ("max_lane0", "max_lane63", "max_last"):
                assert got[c, 0] == max(floor, factor * 3.0e13)
            else:
                assert np.isfinite(got[c, 0]) and got[c, 0] >= floor
    assert not np.isnan(chem.cell_atol(mech, np.full((1, nvar), np.nan), 1.0, 1e-30)).any()


def test_tool_one_call_and_yardstick_on_the_cpu():
    """step_control.py --cpu --atol-rel 1e-13 --yardstick on two gas cells: runs without a GPU, names its AbsTol rule and prints the two distances from
    the yardstick (Rodas4 at RelTol 1e-7, INTEGRATE_x's AbsTol) that tests/conftest.py defines."""
    path = os.path.join(GOLDEN, "integrate_gas.npz")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "step_control.py"), "gas", "--golden", path, "--cells", "0:2", "--cpu", "--atol-rel",
                        "1e-13", "--yardstick"], check=True, capture_output=True, text=True, timeout=300)
    assert "CPU restatement" in r.stdout and "AbsTol = 1e-13 x the cell's largest concentration" in r.stdout
    assert "attempts per cell" in r.stdout
    line = [l for l in r.stdout.split("\n") if l.startswith("distance from the yardstick")]
    assert len(line) == 1 and "Rodas4" in line[0] and "RelTol = 1e-07" in line[0], r.stdout
    import re
    m = re.search(r"species above 1e-3 of the cell's maximum: (\S+)\s+all species, floor 1e-12 x max\|c\|: (\S+)", r.stdout)
    assert m, r.stdout
    a, b = float(m.group(1)), float(m.group(2))
    assert 0.0 <= a < 1.0 and 0.0 <= b < 1.0
