"""The replay, CPU side: the fixed-sequence restatement (tests/ros_replay_py.py) against the restated trace (tests/ros_trace_py.py), the bounds of the
GPU tests (tests/ros_replay_bounds.py), chem.accepted_steps, the C entries' argument refusals (no device is needed for them), the internal-differentiation
property on the restatement and tools/sensitivity.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_bounds as pb
import ros_options_py as R
import ros_replay_bounds as rb
import ros_replay_py as RP
import ros_trace_py as RT
from conftest import MECHS, REPO, load_golden

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
ENTRIES = ("mistra_chem_rosenbrock_replay_ex", "mistra_chem_rosenbrock_replay_device", "mistra_chem_rosenbrock_replay_cells_ex",
           "mistra_chem_rosenbrock_replay_cells_device")


@pytest.mark.parametrize("mech", MECHS)
def test_replay_of_the_accepted_steps_is_the_adaptive_call(mech):
    """Every set and cell: VAR and Texit of the restated replay equal the restated adaptive call's bit for bit, its Err list the accepted records' Err;
    Nstp = Nacc = Ndec = the call's Nacc, Njac equal, Nsol = 3 Nacc, Nrej = Nsng = 0, Nfun = the call's less one per rejected attempt; Hexit is the
    last step made."""
    g = load_golden(mech)
    base, rp = RT.restated(mech, g), RP.restated(mech, g)
    rejected = 0
    for name in RT.SET_NAMES:
        for c, (b, x) in enumerate(zip(base[name], rp[name])):
            tr, st = b[5], b[2]
            acc = (tr.code & 1) == 1
            assert b[1] == 1 and x[1] == 1 and st[7] == 0, (name, c)
            assert x[0].tobytes() == b[0].tobytes() and np.float64(x[3]).tobytes() == np.float64(b[3]).tobytes(), (name, c)
            assert x[5].tobytes() == np.ascontiguousarray(tr.err[acc]).tobytes(), (name, c)
            nacc = int(st[3])
            assert x[2].tolist() == [st[0] - (st[2] - st[3]), st[1], nacc, nacc, 0, nacc, 3 * nacc, 0], (name, c, x[2], st)
            assert x[4] == tr.h[acc][-1], (name, c)
            rejected += int(st[2] - st[3])
    assert mech == "gas" or rejected > 0      # (the property is held on calls that reject steps, gas's seven-step calls apart)


def test_replay_edges_of_the_restatement():
    """no step: the state untouched, IERR 1, zeros; a step of 1e-30: -7 with the steps made so far; a refused option set: its code, nothing made"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    g = load_golden("gas")
    o, diag = Oracle("gas"), mechtab.load("gas").diag
    cell = (g["var_in"][0], g["fix"][0], g["rconst"][0])
    opts = R.base_options("gas")
    y, ierr, st, t, hexit, errs = RP.rosenbrock_replay(o, diag, *cell, *opts, [])
    assert ierr == 1 and y.tobytes() == cell[0].tobytes() and not st.any() and t == R.TIN and hexit == 0.0 and errs.size == 0
    y, ierr, st, t, hexit, errs = RP.rosenbrock_replay(o, diag, *cell, *opts, [0.5, 1.0e-30, 0.5])
    one = RP.rosenbrock_replay(o, diag, *cell, *opts, [0.5])
    assert ierr == -7 and y.tobytes() == one[0].tobytes() and st.tolist() == one[2].tolist() and t == 0.5 and hexit == 0.5 and errs.size == 1
    ipar, rpar, atol, rtol = opts
    bad = rpar.copy()
    bad[0] = -1.0
    y, ierr, st, t, hexit, errs = RP.rosenbrock_replay(o, diag, *cell, ipar, bad, atol, rtol, [0.5])
    assert ierr == -3 and y.tobytes() == cell[0].tobytes() and not st.any() and errs.size == 0


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restated_replays_own_movement(mech):
    """tests/ros_replay_bounds.py: no re-association of the oracle changes IERR, a counter or Texit of a replay along the frozen sequence; the
    constants are within [10x, 100x] of the spread measured now, or are the floor.  Measured: VAR gas 4.36e-17, aer 1.81e-6, tot 5.23e-8; Err gas
    4.61e-5, aer 1.08e-2, tot 3.54e-7."""
    s_var, s_err, moved = rb.measure_spread(mech, load_golden(mech))
    print("%s: VAR spread %.3e (bound %.1e), Err spread %.3e (bound %.1e)" % (mech, s_var, rb.REPLAY_RTOL[mech], s_err, rb.REPLAY_ERR_RTOL[mech]))
    assert not moved, moved
    pb.check_constant("REPLAY_RTOL[%s]" % mech, rb.REPLAY_RTOL[mech], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("REPLAY_ERR_RTOL[%s]" % mech, rb.REPLAY_ERR_RTOL[mech], s_err, floor=pb.PARITY_FLOOR)


def test_accepted_steps_on_a_hand_made_trace():
    """three cells, capacity 4: accepted records only, in order, padded with zeros; a cell with no attempt; records behind ntrace are not looked at;
    a log that overflowed is refused"""
    from mistra_amd import chem
    td = np.zeros((3, 4, 4))
    ti = np.zeros((3, 4, 2), np.int32)
    td[0, :, 1] = [0.1, 0.2, 0.4, 0.8]
    ti[0, :, 1] = [1, 0, 3, 1]               # accepted, rejected, accepted behind a zero pivot, accepted
    td[1, :, 1] = [7.0, 7.0, 7.0, 7.0]       # stale rows: ntrace = 0
    ti[1, :, 1] = [1, 1, 1, 1]
    td[2, :, 1] = [0.5, 0.25, 9.0, 9.0]
    ti[2, :, 1] = [2, 1, 1, 1]               # rejected with a zero pivot, accepted; two stale rows
    hs, ns = chem.accepted_steps(td, ti, np.array([4, 0, 2], np.int32))
    assert hs.shape == (3, 4) and ns.dtype == np.int32 and ns.tolist() == [3, 0, 1]
    assert hs.tolist() == [[0.1, 0.4, 0.8, 0.0], [0.0, 0.0, 0.0, 0.0], [0.25, 0.0, 0.0, 0.0]]
    with pytest.raises(chem.MistraChemError, match="larger cap"):
        chem.accepted_steps(td, ti, np.array([4, 0, 5], np.int32))
    with pytest.raises(chem.MistraChemError, match="expected"):
        chem.accepted_steps(td[:, :, :3], ti, np.array([4, 0, 2], np.int32))


def test_entries_are_declared_exported_and_refuse_bad_arguments_without_a_device():
    """The four replay entries: in the header, in the library, and each refusal of the step table, a method other than Ros3 and a user slot fail with
    their text before a device is looked for (the calls below would otherwise fail with another text, or reach a GPU) — through C and through chem."""
    from mistra_amd import chem
    header = open(os.path.join(REPO, "include", "mistra_chem.h")).read()
    L = chem.lib()
    for entry in ENTRIES:
        assert "int %s(" % entry in header
        assert hasattr(L, entry)
    L.mistra_chem_last_error.restype = C.c_char_p
    mech, mid = "gas", 0
    g = load_golden(mech)
    ncell = 2
    V, F, K = (np.ascontiguousarray(g[k][:ncell]) for k in ("var_in", "fix", "rconst"))
    ipar, rpar, atol, rtol = R.base_options(mech)
    nvar = V.shape[1]
    out, ierr, stats, th = np.zeros_like(V), np.zeros(ncell, np.int32), np.zeros((ncell, 8), np.int32), np.zeros((ncell, 3))
    err = np.full((ncell, 4), -7.25)
    hs, ns = np.full((ncell, 4), 0.5), np.full(ncell, 4, np.int32)
    cat, crt = np.full((ncell, 1), 1.0e-25), np.full((ncell, 1), 1.0e-3)

    def every(ip, cap, hrows, h, n, m=mid, device=True, host=True):
        """the four entries (device False: the two host entries; host False: the two device entries) -> their texts (host addresses in place of device ones: the entries must refuse
        before they look at them)"""
        q = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        table = (cap, hrows, q(h), q(n))
        shared = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ip.ctypes.data_as(_ip))
        cells = (cat.ctypes.data_as(_dp), crt.ctypes.data_as(_dp), 1, rpar.ctypes.data_as(_dp), ip.ctypes.data_as(_ip))
        dcells = (cat.ctypes.data, crt.ctypes.data, 1, rpar.ctypes.data_as(_dp), ip.ctypes.data_as(_ip))
        head = (m, ncell, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), 0.0, 10.0)
        dhead = (m, ncell, V.ctypes.data, F.ctypes.data, K.ctypes.data, 0.0, 10.0)
        res = (out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp), err.ctypes.data_as(_dp))
        dres = (out.ctypes.data, ierr.ctypes.data, stats.ctypes.data, None, err.ctypes.data, None)
        texts = []
        calls = [(L.mistra_chem_rosenbrock_replay_ex, head + shared + table + res), (L.mistra_chem_rosenbrock_replay_cells_ex, head + cells + table + res)]
        if not host:
            calls = []
        if device:
            calls += [(L.mistra_chem_rosenbrock_replay_device, dhead + shared + table + dres),
                      (L.mistra_chem_rosenbrock_replay_cells_device, dhead + dcells + table + dres)]
        for fn, args in calls:
            assert fn(*args) != 0
            texts.append(L.mistra_chem_last_error().decode())
        return texts

    for text in every(ipar, -1, ncell, hs, ns):
        assert "negative step capacity" in text
    for hrows in (0, 3, -1):
        for text in every(ipar, 4, hrows, hs, ns):
            assert "neither 1" in text and "nor ncell" in text
    for text in every(ipar, 4, ncell, None, ns):
        assert "null hsteps" in text
    for text in every(ipar, 4, ncell, hs, None) + every(ipar, 0, 1, None, None):
        assert "null nsteps" in text
    # a count outside 0 .. cap: where the counts are host arrays (both host entries; the device entries' shared form)
    for bad in (np.array([4, 5], np.int32), np.array([-1, 0], np.int32)):
        for text in every(ipar, 4, ncell, hs, bad, device=False):
            assert "lies outside 0 .. cap" in text
    for text in every(ipar, 4, 1, hs, np.array([5], np.int32)):
        assert "nsteps[0] = 5 lies outside 0 .. cap = 4" in text
    # a shared sequence of the device entries longer than the call's block takes, by its count (the capacity may be larger; the host entries have no
    # such limit and are not called here: they would run)
    texts = every(ipar, 5000, 1, np.full((1, 5000), 0.5), np.array([4097], np.int32), host=False)
    assert len(texts) == 2
    for text in texts:
        assert "nsteps[0] = 4097" in text and "MISTRA_REPLAY_MAX_SHARED = 4096" in text
    for method in (0, 1, 3, 4, 5):
        ip = ipar.copy()
        ip[3] = method
        for text in every(ip, 4, ncell, hs, ns):
            assert "replay" in text and "Ros3" in text and "only" in text
    for slot in range(chem.lib().mistra_chem_user_mechs()):
        for text in every(ipar, 4, ncell, hs, ns, m=3 + slot):
            assert "user mechanism slot %d" % slot in text and "replay entries" in text
    for text in every(ipar, 4, ncell, hs, ns, m=17):
        assert "unknown mechanism id" in text
    assert (err == -7.25).all() and not out.any() and not stats.any()
    # ... and through chem
    with pytest.raises(chem.MistraChemError, match="neither 1"):
        chem.rosenbrock_replay(mech, V, F, K, 0.0, 10.0, np.full((3, 4), 0.5), np.full(3, 4, np.int32))
    with pytest.raises(chem.MistraChemError, match="lies outside 0 .. cap"):
        chem.rosenbrock_replay(mech, V, F, K, 0.0, 10.0, hs[0], [5])
    with pytest.raises(chem.MistraChemError, match="null nsteps"):
        chem.rosenbrock_replay(mech, V, F, K, 0.0, 10.0, hs, None)
    with pytest.raises(chem.MistraChemError, match="Ros3"):
        chem.rosenbrock_replay(mech, V, F, K, 0.0, 10.0, hs, ns, ipar=[0, 1, 0, 5])
    with pytest.raises(chem.MistraChemError, match="lies outside 0 .. cap"):
        chem.rosenbrock_replay_cells(mech, V, F, K, 0.0, 10.0, hs, [4, 9], None, None, cat, crt)
    with pytest.raises(chem.MistraChemError, match="other than 0"):
        chem.sensitivities(mech, V[0], F[0], K[0], 0.0, 10.0, atol, rtol, rpar, ipar, [("var", int(np.flatnonzero(V[0] == 0.0)[0]))], 1.0e-6)
    with pytest.raises(chem.MistraChemError, match="inside the mechanism's sizes"):
        chem.sensitivities(mech, V[0], F[0], K[0], 0.0, 10.0, atol, rtol, rpar, ipar, [("rconst", 331)], 1.0e-6)
    assert chem.Sensitivities._fields == ("dy", "var", "max_err", "ierr", "nsteps")
    v, f, r, p = chem.sensitivity_cells(mech, V[0], F[0], K[0], [("fix", 1), ("rconst", 2)], 0.5)
    assert v.shape == (5, nvar) and (v == V[0]).all() and p.tolist() == [F[0, 1], K[0, 2]]
    assert f[:, 1].tolist() == [F[0, 1], 1.5 * F[0, 1], 0.5 * F[0, 1], F[0, 1], F[0, 1]] and (np.delete(f, 1, axis=1) == np.delete(F[0], 1)).all()
    assert r[:, 2].tolist() == [K[0, 2]] * 3 + [1.5 * K[0, 2], 0.5 * K[0, 2]] and (np.delete(r, 2, axis=1) == np.delete(K[0], 2)).all()


def test_internal_differentiation_removes_the_step_controls_noise():
    """tests/ros_replay_bounds.py's case on the restatement: central differences at eps and eps / 10 of three parameters of one daylight gas cell.
    Replayed along the base cell's accepted steps the pair agrees within IND_REPLAY_TOL — held to [10x, 100x] of its disagreement measured now — and
    better than the pair from adaptive calls.  Measured: replayed 1.163e-3, adaptive 2.58."""
    rep, ada = rb.measure_ind(load_golden("gas", rb.IND_SET))
    print("internal differentiation: replayed pair %.4e (bound %.1e), adaptive pair %.4e" % (rep, rb.IND_REPLAY_TOL, ada))
    pb.check_constant("IND_REPLAY_TOL", rb.IND_REPLAY_TOL, rep)
    assert rep <= rb.IND_REPLAY_TOL
    assert rep < ada


def test_tool_runs_on_the_restatement():
    """tools/sensitivity.py --restated --adaptive on the bounds file's cell: the command runs without a GPU and prints p*dy/dp of the species asked
    for as the restatement gives it"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    path = os.path.join(REPO, "tests", "golden", "integrate_gas%s.npz" % rb.IND_SET)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "sensitivity.py"), "gas", "--golden", path, "--cell", str(rb.IND_CELL), "--rconst", "30",
                        "--var", "5", "--species", "5,12", "--eps", "1e-4", "--rtol", "1e-4", "--restated", "--adaptive"],
                       check=True, capture_output=True, text=True, timeout=120)
    g = load_golden("gas", rb.IND_SET)
    o, diag = Oracle("gas"), mechtab.load("gas").diag
    cell = (g["var_in"][rb.IND_CELL], g["fix"][rb.IND_CELL], g["rconst"][rb.IND_CELL])
    opts = rb.ind_options()
    hs = RP.accepted(RT.rosenbrock_trace(o, diag, *cell, *opts)[5])
    dy = RP.sensitivity_restated(o, diag, *cell, opts, [("var", 4), ("rconst", 29)], 1.0e-4, hs)
    lines = r.stdout.splitlines()
    assert "%d frozen steps" % len(hs) in lines[0], r.stdout
    assert lines[1].startswith("var 5 = ") and lines[4].startswith("rconst 30 = "), r.stdout
    for line, k, p, s in ((lines[2], 0, cell[0][4], 4), (lines[3], 0, cell[0][4], 11), (lines[5], 1, cell[2][29], 4), (lines[6], 1, cell[2][29], 11)):
        assert "species %4d" % (s + 1) in line and "% .9e" % (p * dy[k][s]) in line and "adaptive calls" in line, (line, p * dy[k][s])
