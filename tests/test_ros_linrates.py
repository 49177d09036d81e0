"""A series of Rosenbrock_x calls with rate constants linear in time over each leg, CPU side: the restatement that defines it
(tests/ros_linrates_py.py) against the series-with-rates restatement where the two must agree, what the time derivative is worth, the bounds of the GPU
tests (tests/ros_linrates_bounds.py) and the refusals the four entries make before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import ros_linrates_py as LR
import ros_methods_py as RM
import ros_series_py as RS
from conftest import MECHS, rel_diff

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def cell_max_diff(got, want):
    """largest |got - want| of a cell as a fraction of the cell's largest concentration.  The measure of the two tests below that compare integrations
    with DIFFERENT step sequences at RelTol = 1e-3: species by species (conftest's rel_diff) such runs differ by the tolerance itself in the minor
    species, whatever the rate constants do — the figures are printed beside it."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    return float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())


def test_the_sets_and_the_nodes_are_the_ones_the_issue_names():
    assert LR.TIMES == (0.0, 2.5, 5.0, 7.5, 10.0) and LR.W_NODES == (0.0, 0.25, 0.5, 0.75, 1.0)
    assert LR.METHOD_SETS == ("m1", "m2", "m3", "m4", "m5") and [LR.series_set("gas", n)[0].ipar[3] for n in LR.METHOD_SETS] == [1, 2, 3, 4, 5]
    assert all(LR.series_set("gas", n)[0].ipar[0] == 0 for n in LR.SET_NAMES) and LR.series_set("gas", "ros3_autonomous_flag")[0].ipar[0] == 1
    assert LR.set_names("gas")[-1] == "ros3_autonomous_flag" and "ros3_autonomous_flag" not in LR.set_names("aer") + LR.set_names("tot")
    for name in ("ros3_carry", "ros3_fix_per_leg", "ros3_equal_nodes", "ros3_descending"):
        assert name in LR.SET_NAMES
    for mech in MECHS:
        V, LF, NK = LR.nodes(mech)
        assert NK.shape[:2] == (5, 3) and LF.shape[:2] == (4, 3)
        assert all(not np.array_equal(NK[k], NK[k + 1]) for k in range(4))
        s, _, F, K = LR.set_rows(mech, "ros3_descending")
        assert list(s.times) == [10.0, 7.5, 5.0, 2.5, 0.0] and K.tobytes() == NK[::-1].tobytes() and F.ndim == 2
        s, _, F, K = LR.set_rows(mech, "ros3_fix_per_leg")
        assert F.tobytes() == LF.tobytes() and K.tobytes() == NK.tobytes()
        _, _, _, K = LR.set_rows(mech, "ros3_equal_nodes")
        assert all(K[k].tobytes() == NK[0].tobytes() for k in range(5))
    # the rate constants as the definition rounds them: equal nodes give the node at every time, the ends give the nodes
    k0 = np.array([1.0e-11, 3.0, 0.1]); d0 = np.zeros(3)
    assert all(LR.rate_at(k0, d0, 2.5, 1.0 / 2.5, t).tobytes() == k0.tobytes() for t in (2.5, 3.1, 4.999, 5.0))
    k1 = np.array([2.0e-11, 1.0, 0.1])
    assert LR.rate_at(k0, k1 - k0, 2.5, 1.0 / 2.5, 2.5).tobytes() == k0.tobytes() and np.allclose(LR.rate_at(k0, k1 - k0, 2.5, 1.0 / 2.5, 5.0), k1, rtol=1e-15)


@pytest.mark.parametrize("mech", MECHS)
def test_equal_nodes_are_the_series_with_rates_on_the_shared_block(mech):
    """ros3_equal_nodes and its Rodas4 twin against tests/ros_series_py.py's chain over tests/ros_methods_py.py's Rosenbrock_x with the night rows, bit for
    bit in every leg: VAR, IERR, IPAR(11:18), Texit, Hexit.  (dFdT is a zero in both: a sum of zero products here, a difference of equal values there.)"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle(mech), mechtab.load(mech).diag
    r = LR.restated(mech, 0, LR.EQUAL_SETS)
    for name in LR.EQUAL_SETS:
        s, V, F, NK = LR.set_rows(mech, name)
        assert F.ndim == 2
        for c in range(3):
            want = RS.chain(lambda y, rpar, t0, t1: RM.rosenbrock(o, diag, y, F[c], NK[0, c], s.ipar, rpar, s.atol, s.rtol, t0, t1), V[c], s)
            got = [x[:, c] for x in r[name]]
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (name, c)
            assert got[0].tobytes() == want[0].tobytes(), (name, c)
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), (name, c)
            assert (want[1] == 1).all()


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_linrates_bounds.py: no re-association of the oracle changes IERR or a counter in any leg of any (set, cell); the constants are within
    [10x, 100x] of the spread measured now, or are the floor.  What the sets are there for holds: the descending one ends every leg with -7 having
    made steps, every other leg with 1; linear differs from the staircase of the same rows."""
    import parity_bounds as pb
    import ros_linrates_bounds as lb
    s_var, s_th, moved = lb.measure_spread(mech)
    print("%s: VAR spread %.3e, exit time / last step size spread %.3e" % (mech, s_var, s_th))
    assert not moved, "re-association changes IERR or the counters: %s" % moved
    pb.check_constant("LINRATES_RTOL[%s]" % mech, lb.LINRATES_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("LINRATES_TH_RTOL[%s]" % mech, lb.LINRATES_TH_RTOL[mech], s_th, floor=pb.PARITY_FLOOR)
    r = LR.restated(mech)
    for name in LR.set_names(mech):
        assert (r[name][1] == LR.FAILING_IERR.get(name, 1)).all(), name
    assert (r["ros3_descending"][2][..., 3] >= 1).all()
    assert r["m2"][0][0].tobytes() == r["ros3_carry"][0][0].tobytes() and r["m2"][0][-1].tobytes() != r["ros3_carry"][0][-1].tobytes()
    assert r["m2"][0][0].tobytes() == r["ros3_fix_per_leg"][0][0].tobytes() and r["m2"][0][1].tobytes() != r["ros3_fix_per_leg"][0][1].tobytes()
    assert all(r["m2"][0][k].tobytes() != r["ros3_equal_nodes"][0][k].tobytes() for k in range(4))


def _one_cell_gas():
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    V, LF, NK = LR.nodes("gas")
    return Oracle("gas"), mechtab.load("gas").diag, V[0], LF[0, 0], NK[0, 0], NK[4, 0]


def test_refining_the_midpoint_staircase_converges_to_the_linear_leg():
    """gas, one cell, Ros3 with the carried first step: n piecewise-constant legs over 0 .. 10 s, leg j with the rate constants at its midpoint, against
    ONE leg with the rate constants linear from the night row at 0 to the day row at 10.  The distance of the end states (cell_max_diff) shrinks at
    least 4x from 4 to 16 sub-legs — second order would be 16x; measured 4.9e-12 -> 2.9e-13, 17x.  (conftest's rel_diff of the same states: 6.2e-2 ->
    1.6e-2, the step control's own noise in the minor species.)"""
    o, diag, v, f, ka, kb = _one_cell_gas()
    ipar, rpar, atol, rtol = LR.R.base_options("gas")
    lin = LR.rosenbrock(o, diag, v, f, ka, kb, ipar, rpar, atol, rtol, 0.0, 10.0)
    assert lin[1] == 1
    dist = {}
    for n in (4, 16):
        times = np.linspace(0.0, 10.0, n + 1)
        s = RS.Series(ipar, rpar, atol, rtol, times, True)
        mid = iter(0.5 * (times[:-1] + times[1:]))
        stair = RS.chain(lambda y, rp, t0, t1: RM.rosenbrock(o, diag, y, f, LR.rate_at(ka, kb - ka, 0.0, 1.0 / 10.0, next(mid)), ipar, rp, atol, rtol, t0, t1), v, s)
        assert (stair[1] == 1).all()
        dist[n] = cell_max_diff(stair[0][-1], lin[0])
        print("%d sub-legs: cell_max_diff %.3e, rel_diff %.3e" % (n, dist[n], float(rel_diff(stair[0][-1], lin[0]).max())))
    print("distance from the linear leg: 4 sub-legs %.3e, 16 sub-legs %.3e, ratio %.1f" % (dist[4], dist[16], dist[4] / dist[16]))
    assert dist[16] > 0.0 and dist[4] >= 4.0 * dist[16]


def test_without_the_time_derivative_the_controller_pays():
    """ros3_autonomous_flag on gas: IPAR(1) = 1 leaves the HG*dFdT terms out while the rates still move.  The error estimator sees the missing time
    derivative: at least 10x the steps of m2 in leg 0 in every cell, for an end state within 1e-9 of m2's as a fraction of the cell's largest
    concentration (cell_max_diff; measured 3.3e-12.  conftest's rel_diff of the same states is 2.0e-3: two step sequences at RelTol = 1e-3)."""
    r = LR.restated("gas", 0, ("m2", "ros3_autonomous_flag"))
    with_terms, without = r["m2"], r["ros3_autonomous_flag"]
    print("Nstp in leg 0: with the terms %s, without %s" % (with_terms[2][0, :, 2].tolist(), without[2][0, :, 2].tolist()))
    assert (without[2][0, :, 2] >= 10 * with_terms[2][0, :, 2]).all()
    d = cell_max_diff(without[0][-1], with_terms[0][-1])
    print("end states: cell_max_diff %.3e, rel_diff %.3e" % (d, float(rel_diff(without[0][-1], with_terms[0][-1]).max())))
    assert d <= 1.0e-9
    # Nfun counts the derivative's Fun call where it is made: Ros3 evaluates once per attempt (stage 2) and once per step (Fcn0), plus dFdT per step
    for st, per_step in ((with_terms[2], 2), (without[2], 1)):
        assert np.array_equal(st[..., 0], per_step * st[..., 3] + st[..., 2])


def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """fix_legs, a null rconst_nodes, the series' own refusals, both user slots and an unknown mechanism: each fails with its own text through all four
    entries, with no device initialised — never the 'no HIP device' or an unknown-symbol path."""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    ipar = np.array([0, 1, 0, 2] + [0] * 16, np.int32)
    out = np.zeros(4)      # never written: every call below is refused
    some = np.zeros(4)     # a non-null rconst_nodes, never read

    def entries(mid, nleg, times, var_series, nlf=1, ntol=nvar, nodes=some):
        tp, vs = None if times is None else _P(times), None if var_series is None else _P(var_series)
        kp = None if nodes is None else _P(nodes)
        head = (mid, 1, None, None, kp, nlf, nleg, tp)
        dhead = (mid, 1, None, None, None if kp is None else C.cast(kp, C.c_void_p), nlf, nleg, tp)
        dv = None if vs is None else C.cast(vs, C.c_void_p)
        return {
            "ex": lambda: L.mistra_chem_rosenbrock_series_linrates_ex(*head, _P(tol), _P(tol), _P(rpar), _P(ipar), 0, None, vs, None, None, None),
            "device": lambda: L.mistra_chem_rosenbrock_series_linrates_device(*dhead, _P(tol), _P(tol), _P(rpar), _P(ipar), dv, None, None, None, 0, None, None),
            "cells_ex": lambda: L.mistra_chem_rosenbrock_series_linrates_cells_ex(*head, _P(tol), _P(tol), ntol, _P(rpar), _P(ipar), 0, None, vs, None, None, None),
            "cells_device": lambda: L.mistra_chem_rosenbrock_series_linrates_cells_device(*dhead, C.cast(_P(tol), C.c_void_p), C.cast(_P(tol), C.c_void_p), ntol,
                                                                                          _P(rpar), _P(ipar), dv, None, None, None, 0, None, None),
        }

    def refused(calls, text):
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    good = np.array([0.0, 1.0, 2.0, 3.0])
    for bad in (0, 2, 4, -1):
        refused(entries(0, 3, good, out, nlf=bad), "series: fix_legs = %d: fix has 1 block (shared by all legs) or nleg = 3 blocks" % bad)
    for nlf in (1, 3):
        refused(entries(0, 3, good, out, nlf=nlf, nodes=None), "series: null rconst_nodes pointer (rconst_nodes: [nleg + 1][ncell][NREACT]")
    long_times = np.arange(chem.SERIES_MAX_LEGS + 2, dtype=np.float64)
    refused(entries(0, 0, good, out), "nleg = 0: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, chem.SERIES_MAX_LEGS + 1, long_times, out), "nleg = 4097: a series has 1 .. MISTRA_SERIES_MAX_LEGS = 4096 legs")
    refused(entries(0, 2, np.array([0.0, np.nan, 2.0]), out), "times[1] is not finite")
    refused(entries(0, 2, np.array([0.0, 1.0, 1.0]), out), "times[2] repeats times[1]")
    refused(entries(0, 2, np.array([0.0, 1.0, 0.5]), out), "the times change direction at times[2]")
    refused(entries(0, 2, None, out), "null times pointer")
    refused(entries(0, 2, good, None), "null var_series pointer")
    refused(entries(9, 2, good, out), "unknown mechanism id")
    cells = {k: v for k, v in entries(0, 2, good, out, ntol=2).items() if "cells" in k}
    refused(cells, "ntol = 2: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    names = chem.user_mechs()
    assert len(names) == 2      # the library this repository builds has both
    for i in range(2):          # both user slots: the slot's existing text
        refused(entries(3 + i, 2, good, out), "user mechanism slot %d (%s) has no series of Rosenbrock_x calls: a user slot integrates" % (i, names[i]))
    # the Python surface passes the refusals on, without init()
    V, LF, NK = LR.nodes("gas")
    with pytest.raises(chem.MistraChemError, match="rconst_nodes: a 3-D .nleg \\+ 1, ncell, NREACT. array expected"):
        chem.rosenbrock_series_linrates("gas", V, LF[0], NK[:4], LR.TIMES)
    with pytest.raises(chem.MistraChemError, match="rconst_nodes: a 3-D"):
        chem.rosenbrock_series_linrates("gas", V, LF[0], NK[0], LR.TIMES)
    with pytest.raises(chem.MistraChemError, match="fix_legs = 3: fix has 1 block .* or nleg = 4 blocks"):
        chem.rosenbrock_series_linrates("gas", V, LF[:3], NK, LR.TIMES)
    with pytest.raises(chem.MistraChemError, match="cell counts of var / fix / rconst differ"):
        chem.rosenbrock_series_linrates("gas", V, LF[:, :2], NK, LR.TIMES)
    for times, text in (([0.0, 1.0, 1.0], "repeats"), ([0.0, 2.0, 1.0], "change direction"), ([0.0, np.nan], "not finite")):
        with pytest.raises(chem.MistraChemError, match=text):
            chem.rosenbrock_series_linrates("gas", V, LF[0], NK[:len(times)], times)
    with pytest.raises(chem.MistraChemError, match="nleg = 0"):
        chem.rosenbrock_series_linrates("gas", V, LF[0], NK[:1], [0.0])
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_series_linrates("gas", V, LF, NK, LR.TIMES, atol=np.ones((3, 5)), rtol=np.ones((3, 5)))


def test_series_linrates_needs_a_device():
    """Without a GPU a well-formed call raises 'no HIP device' (there is no CPU path), through the shared-pair and the cells form."""
    import torch
    from mistra_amd import chem
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    V, LF, NK = LR.nodes("gas")
    for F in (LF, LF[0]):
        with pytest.raises(chem.MistraChemError, match="no HIP device"):
            chem.rosenbrock_series_linrates("gas", V, F, NK, LR.TIMES)
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_series_linrates("gas", V, LF, NK, LR.TIMES, atol=np.full((3, 1), 1.0e-20), rtol=np.full((3, 1), 1.0e-3))


def test_tool_box_series_linear_on_the_cpu():
    """tools/box_series.py gas --cpu --linear --compare: the dawn with node blocks through the restatement, the staircase beside it.  Nothing is asserted
    on the figures but that they are numbers, that there is one line per leg of each kind and that the two runs differ."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "box_series.py"), "gas", "--cpu", "--linear", "--compare", "--legs", "2", "--cells", "1"],
                       check=True, capture_output=True, text=True, timeout=300)
    assert "linear in time over each leg (3 node blocks); CPU restatement" in r.stdout
    rows = [l.split("|")[0].split() for l in r.stdout.split("\n") if l.startswith("leg ")]
    assert [int(x[1]) for x in rows] == [0, 1] and all(np.isfinite([float(v) for v in x[2:]]).all() for x in rows), r.stdout
    cmp_rows = [l.split() for l in r.stdout.split("\n") if l.startswith("cmp ")]
    assert [int(x[1]) for x in cmp_rows] == [0, 1] and all(float(x[3]) > 0.0 for x in cmp_rows), r.stdout
