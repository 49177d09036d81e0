"""The step-control trace, CPU side: the restatement with the record (tests/ros_trace_py.py) against the pinned restatement of Rosenbrock_x
(tests/ros_methods_py.py), the record's invariants, the bounds of the GPU tests (tests/ros_trace_bounds.py), the two C entries' argument refusals
(no device is needed for them) and tools/step_control.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ros_methods_py as RM
import ros_options_py as R
import ros_trace_py as RT
from conftest import MECHS, REPO, load_golden

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
# every set the restatement is used on: the trace tests' own and the other option sets that run (a max_steps exit among them)
PINNED_SETS = RT.SET_NAMES + ("factors", "hmin_0.05", "autonomous", "max_steps_5")


def _set(mech, name):
    return RT.trace_set(mech, name) if name in RT.SET_NAMES else R.option_set(mech, name)


@pytest.mark.parametrize("mech", MECHS)
def test_restatement_is_the_pinned_one_and_the_record_adds_up(mech):
    """VAR, IERR, counters, Texit, Hexit equal ros_methods_py.rosenbrock's bit for bit on every set used; records = Nstp, accepted records = Nacc,
    rejected records behind the first accepted one = Nrej, ctrl = the histogram of species, share in [0, 1], T and H as the loop had them."""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    g = load_golden(mech)
    o, diag = Oracle(mech), mechtab.load(mech).diag
    own = RT.restated(mech, g)
    for name in PINNED_SETS:
        for k, c in enumerate(RT.cells_of(g["var_in"].shape[0])):
            args = (o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c]) + tuple(_set(mech, name))
            want = RM.rosenbrock(*args)
            got = own[name][k] if name in RT.SET_NAMES else RT.rosenbrock_trace(*args)
            assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and np.array_equal(got[2], want[2]), (name, c)
            assert got[3] == want[3] and got[4] == want[4], (name, c)
            tr, st = got[5], got[2]
            acc = (tr.code & 1) == 1
            assert len(tr.t) == st[2] and acc.sum() == st[3], (name, c)
            first = int(np.argmax(acc)) if acc.any() else len(acc)
            assert (~acc[first:]).sum() == st[4], (name, c)
            assert (tr.code >> 1).sum() == st[7] and st[7] == 0
            assert np.array_equal(tr.ctrl, np.bincount(tr.species, minlength=len(tr.ctrl) + 1)[1:]) and (tr.species >= 1).all()
            assert ((tr.share > 0.0) & (tr.share <= 1.0 + 1e-12)).all(), (name, c)
            # T of a record is the sum of the accepted steps before it, H of the last accepted record is Hexit (the step as attempted)
            t = 0.0
            for i in range(len(tr.t)):
                assert tr.t[i] == t
                if acc[i]:
                    t = t + tr.h[i]
            if got[1] == 1:
                assert t == got[3] and tr.h[np.nonzero(acc)[0][-1]] <= got[4]
    assert all(r[1] == -6 for r in (RT.rosenbrock_trace(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *R.option_set(mech, "max_steps_5"))
                                    for c in RT.cells_of(g["var_in"].shape[0])[:1]))
    # a refusal: no record
    r = RT.rosenbrock_trace(o, diag, g["var_in"][0], g["fix"][0], g["rconst"][0], *R.refused_set(mech, "rpar1_-1"))
    assert r[1] == -3 and len(r[5].t) == 0 and not r[5].ctrl.any()


def test_largest_term_rules():
    """ties go to the lowest species, a NaN never wins, no positive term gives species 0 and share 0"""
    nan = float("nan")
    assert RT.largest_term(np.array([1.0, 4.0, 4.0, 2.0])) == (2, 4.0)
    assert RT.largest_term(np.array([nan, 1.0, nan, 3.0, 3.0])) == (4, 3.0)
    assert RT.largest_term(np.array([nan, nan])) == (0, 0.0)
    assert RT.largest_term(np.array([0.0, 0.0])) == (0, 0.0)
    assert RT.largest_term(np.array([0.0, float("inf"), float("inf")])) == (2, float("inf"))
    assert RT.share_of(0.0, 0.0, 3) == 0.0 and RT.share_of(3.0, 1.0, 3) == 1.0


@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restated_traces_own_movement(mech):
    """tests/ros_trace_bounds.py: no re-association of the oracle changes the number of records, a code or a species on any (set, cell, attempt) —
    although attempts with a runner-up within 0.9 of the top term exist; the constants are within [10x, 100x] of the spread measured now, or are the
    floor.  Measured: T gas 0, aer 1.01e-6, tot 3.03e-8; H gas 0, aer 3.13e-6, tot 1.03e-7; Err gas 4.61e-5, aer 1.88e-2, tot 4.38e-7; share gas
    2.18e-5, aer 1.49e-2, tot 7.11e-7."""
    import parity_bounds as pb
    import ros_trace_bounds as tb
    g = load_golden(mech)
    (s_t, s_h, s_err, s_share), moved = tb.measure_spread(mech, g)
    print("%s: T spread %.3e, H %.3e, Err %.3e, share %.3e" % (mech, s_t, s_h, s_err, s_share))
    assert not moved, "re-association changes the record count, a code or a species: %s" % moved
    pb.check_constant("TRACE_T_TOL[%s]" % mech, tb.TRACE_T_TOL[mech], s_t, floor=pb.PARITY_FLOOR)
    pb.check_constant("TRACE_H_RTOL[%s]" % mech, tb.TRACE_H_RTOL[mech], s_h, floor=pb.PARITY_FLOOR)
    pb.check_constant("TRACE_ERR_RTOL[%s]" % mech, tb.TRACE_ERR_RTOL[mech], s_err, floor=pb.PARITY_FLOOR)
    pb.check_constant("TRACE_SHARE_TOL[%s]" % mech, tb.TRACE_SHARE_TOL[mech], s_share, floor=pb.PARITY_FLOOR)
    close = 0
    for rows in RT.restated(mech, g).values():
        for r in rows:
            top2 = np.sort(r[5].terms, axis=1)[:, -2:]
            close += int((top2[:, 0] > 0.9 * top2[:, 1]).sum())
    print("%s: attempts with a runner-up within 0.9 of the top term: %d" % (mech, close))
    assert close >= 1, "the species premise is only worth holding where close runner-ups exist"


def test_entries_are_declared_exported_and_refuse_bad_arguments_without_a_device():
    """mistra_chem_rosenbrock_trace_ex / _device: in the header, in the library, and cap < 0, a missing ntrace, cap > 0 with a missing log array and
    ipar[3] /= 2 each fail with their text before a device is looked for (the calls below would otherwise fail with another text, or reach a GPU)."""
    from mistra_amd import chem
    header = open(os.path.join(REPO, "include", "mistra_chem.h")).read()
    L = chem.lib()
    for entry in ("mistra_chem_rosenbrock_trace_ex", "mistra_chem_rosenbrock_trace_device"):
        assert "int %s(" % entry in header
        assert hasattr(L, entry)
    L.mistra_chem_last_error.restype = C.c_char_p
    mech, mid = "gas", 0
    g = load_golden(mech)
    V, F, K = (np.ascontiguousarray(g[k][:1]) for k in ("var_in", "fix", "rconst"))
    ipar, rpar, atol, rtol = R.base_options(mech)
    out, ierr, stats, th = np.zeros_like(V), np.zeros(1, np.int32), np.zeros((1, 8), np.int32), np.zeros((1, 3))
    td, ti, nt = np.full((1, 4, 4), -7.25), np.full((1, 4, 2), 77, np.int32), np.full(1, 77, np.int32)

    def both(ip, cap, d, i, n):
        opts = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ip.ctypes.data_as(_ip))
        p = lambda x, t: None if x is None else x.ctypes.data_as(t)  # noqa: E731
        texts = []
        rc = L.mistra_chem_rosenbrock_trace_ex(mid, 1, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), 0.0, 10.0, *opts,
                                               out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp),
                                               cap, p(d, _dp), p(i, _ip), p(n, _ip), None)
        assert rc != 0
        texts.append(L.mistra_chem_last_error().decode())
        # (host addresses in place of device ones: the entry must refuse before it looks at them)
        q = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        rc = L.mistra_chem_rosenbrock_trace_device(mid, 1, V.ctypes.data, F.ctypes.data, K.ctypes.data, 0.0, 10.0, *opts, out.ctypes.data,
                                                   ierr.ctypes.data, stats.ctypes.data, None, None, None, cap, q(d), q(i), q(n), None)
        assert rc != 0
        texts.append(L.mistra_chem_last_error().decode())
        return texts

    for text in both(ipar, -1, td, ti, nt):
        assert "negative trace capacity" in text
    for text in both(ipar, 4, td, ti, None):
        assert "null ntrace" in text
    for text in both(ipar, 4, None, ti, nt) + both(ipar, 4, td, None, nt):
        assert "null trace_d or trace_i" in text
    for method in (0, 1, 3, 4, 5):
        ip = ipar.copy()
        ip[3] = method
        for text in both(ip, 4, td, ti, nt):
            assert "Ros3" in text and "only" in text
    assert (td == -7.25).all() and (ti == 77).all() and nt[0] == 77 and not out.any()
    with pytest.raises(chem.MistraChemError, match="negative trace capacity"):
        chem.rosenbrock_trace(mech, V, F, K, 0.0, 10.0, cap=-1)
    assert chem.Trace._fields == ("t", "h", "err", "share", "species", "code", "n", "ctrl")


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("step_control", os.path.join(REPO, "tools", "step_control.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_table_on_a_hand_made_trace():
    """two cells, four species, seven records: counts, rejected counts, cells, medians, the order (most controlled first, ties to the lower
    number), the capacity note and the names"""
    sc = _tool()
    var_in = np.array([[1.0, 1e-3, 0.0, 4.0], [2.0, 1e-6, 8.0, 0.5]])
    var_out = np.array([[2.0, 1e-4, 0.0, 4.0], [1.0, 2e-6, 4.0, 0.5]])
    rows = [(np.array([2, 2, 4, 2]), np.array([1, 0, 1, 3]), 4),       # cell 0: species 2 controls 3 (1 rejected), species 4 one
            (np.array([2, 3, 3]), np.array([0, 1, 0]), 5)]             # cell 1: 5 attempts, 3 kept: species 2 one (rejected), species 3 two (1 rejected)
    t = sc.control_table(var_in, var_out, rows, top=3)
    assert t["attempts"].tolist() == [4, 5] and t["kept"] == 7 and t["rejected"] == 3 and t["none"] == 0
    assert [r[:4] for r in t["species"]] == [(2, 4, 2, 2), (3, 2, 1, 1), (4, 1, 0, 1)]
    med = [r[4] for r in t["species"]]
    assert med[0] == np.median([1e-3 / 4.0, 2e-6 / 8.0]) and med[1] == 1.0 and med[2] == 1.0
    text = sc.format_table(t, names=["A", "B", "C"])
    assert "min 4" in text and "max 5" in text and "9 in 2 cells; 7 recorded, 3 of them rejected" in text and "dropped" in text
    lines = text.split("\n")
    assert lines[-3].split()[:2] == ["B", "4"] and lines[-2].split()[:2] == ["C", "2"] and lines[-1].split()[:2] == ["VAR(4)", "1"]
    assert "57.1%" in lines[-3]
    # a record without a positive term is counted apart
    t0 = sc.control_table(var_in[:1], var_out[:1], [(np.array([0, 1]), np.array([0, 1]), 2)])
    assert t0["none"] == 1 and [r[:3] for r in t0["species"]] == [(1, 1, 0)]


def test_tool_cpu_path_gives_the_restated_histogram():
    """step_control.py --cpu on two gas cells of the captured set: the command runs without a GPU and prints the table control_table gives for the
    restated trace."""
    sc = _tool()
    path = os.path.join(REPO, "tests", "golden", "integrate_gas.npz")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "step_control.py"), "gas", "--golden", path, "--cells", "0:2", "--cpu", "--atol",
                        "1e-15"], check=True, capture_output=True, text=True, timeout=120)
    g = load_golden("gas")
    rows, outs = [], []
    own = RT.restated("gas", g, 0, ("atol_1e-15",))["atol_1e-15"][0]      # cell 0
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, diag = Oracle("gas"), mechtab.load("gas").diag
    for c in (0, 1):
        x = own if c == 0 else RT.rosenbrock_trace(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], *RT.trace_set("gas", "atol_1e-15"))
        rows.append((x[5].species, x[5].code, len(x[5].species)))
        outs.append(x[0])
    want = sc.format_table(sc.control_table(g["var_in"][:2], np.array(outs), rows))
    assert want in r.stdout, r.stdout
    assert "CPU restatement" in r.stdout and "AbsTol = 1e-15" in r.stdout
