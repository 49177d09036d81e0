"""The replay on the GPU (-m gpu): mistra_chem_rosenbrock_replay_ex / _device and their cells forms run Ros3 along a prescribed step sequence, every step
accepted.  The exact oracle: a replay of a traced call's accepted steps IS that call, bit for bit.  Against the restatement (tests/ros_replay_py.py)
within tests/ros_replay_bounds.py, measured on the reference side (tests/test_ros_replay.py).  Cells 0, n/2, n-1 of integrate_<mech>.npz unless a test
says otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ros_options_py as R
import ros_replay_bounds as rb
import ros_replay_py as RP
import ros_trace_py as RT
from conftest import MECHS, REPO, load_golden

pytestmark = pytest.mark.gpu
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}
GAMMA1 = R.ROS_GAMMA[0]
CAP = 256
DRIVER = os.path.join(REPO, "shim", "shim_driver")


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    yield c
    for mech in MECHS:
        c.clear_options(mech)


def _cells(mech):
    g = load_golden(mech)
    c = list(RT.cells_of(g["var_in"].shape[0]))
    return np.ascontiguousarray(g["var_in"][c]), np.ascontiguousarray(g["fix"][c]), np.ascontiguousarray(g["rconst"][c])


def _T(x, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(x, dtype), device=torch.device("cuda", 0))


def _np(res):
    """(IntegrateResult, th, ...) of either kind -> (var, ierr, stats, Texit/Hexit [n, 2], *rest) as numpy arrays"""
    import torch
    torch.cuda.synchronize()
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)  # noqa: E731
    r, th = res[0], host(res[1])
    return (host(r.var), host(r.ierr), host(r.stats), np.ascontiguousarray(th[:, :2])) + tuple(host(x) for x in res[2:])


def _traced(chem, mech, V, F, K, opts, device, tstart=R.TIN, tend=R.TOUT):
    """a traced call -> (its results as _np gives them, hsteps [n, CAP], nsteps [n], the accepted records' Err per cell)"""
    args = (_T(V), _T(F), _T(K)) if device else (V, F, K)
    res = chem.rosenbrock_trace(mech, *args, tstart, tend, *opts, cap=CAP, ctrl=False)
    out = _np(res[:2])
    tr = res[2]
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)  # noqa: E731
    td = np.stack([host(tr.t), host(tr.h), host(tr.err), host(tr.share)], axis=-1)
    ti = np.stack([host(tr.species), host(tr.code)], axis=-1)
    nt = host(tr.n)
    hs, ns = chem.accepted_steps(td, ti, nt)
    errs = [td[c, :nt[c], 2][(ti[c, :nt[c], 1] & 1) == 1] for c in range(V.shape[0])]
    return out, hs, ns, errs


def _replay(chem, mech, V, F, K, opts, hs, ns, device, tstart=R.TIN, tend=R.TOUT, err_log=None):
    """device: the cell data as tensors; rows per cell (hs 2-D with one row per cell, more than one cell) as tensors too, a shared row stays numpy"""
    if not device:
        return _np(chem.rosenbrock_replay(mech, V, F, K, tstart, tend, hs, ns, *opts, err_log=err_log))
    own = np.ndim(hs) == 2 and np.shape(hs)[0] == V.shape[0] and V.shape[0] > 1
    h, n = (_T(hs, np.float64), _T(ns, np.int32)) if own else (hs, ns)
    return _np(chem.rosenbrock_replay(mech, _T(V), _T(F), _T(K), tstart, tend, h, n, *opts, err_log=None if err_log is None else _T(err_log)))


def _counters_of_a_replay(stats, traced_stats):
    """Nstp = Nacc = Ndec = the call's Nacc, Njac equal, Nsol = 3 Nacc, Nrej = Nsng = 0, Nfun = the call's less one per rejected attempt"""
    for st, ts in zip(stats, traced_stats):
        nacc = int(ts[3])
        assert ts[7] == 0
        assert st.tolist() == [ts[0] - (ts[2] - ts[3]), ts[1], nacc, nacc, 0, nacc, 3 * nacc, 0], (st, ts)


@pytest.mark.parametrize("name", RT.SET_NAMES)
@pytest.mark.parametrize("mech", MECHS)
def test_p1_replay_of_the_traced_steps_is_the_traced_call(chem, mech, name):
    """Per mechanism and option set, host and device form: the replay of the device trace's accepted steps with rows per cell gives var_out and Texit of
    the traced call bit for bit, err_log its accepted records' Err, the counters as derived, Hexit the last step; entries of err_log past a cell's
    count are untouched.  One shared row (cell c's, for every c): cell c again the traced call, and every cell equal to its run with that row as its
    own.  Then along the RESTATED trace's steps, against the restated replay: VAR and Err within the bounds file, counters and Texit identical."""
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, name)
    n = V.shape[0]
    for dev in (False, True):
        (tv, tierr, tstats, tth), hs, ns, errs = _traced(chem, mech, V, F, K, opts, dev)
        assert (tierr == 1).all() and (ns > 0).all() and (ns <= CAP).all()
        log = np.full((n, CAP), -7.25)
        var, ierr, stats, th, err = _replay(chem, mech, V, F, K, opts, hs, ns, dev, err_log=log)
        assert var.tobytes() == tv.tobytes() and th[:, 0].tobytes() == tth[:, 0].tobytes() and (ierr == 1).all(), (dev, "rows per cell")
        _counters_of_a_replay(stats, tstats)
        for c in range(n):
            assert err[c, :ns[c]].tobytes() == np.ascontiguousarray(errs[c]).tobytes(), (dev, c)
            assert (err[c, ns[c]:] == -7.25).all() and th[c, 1] == hs[c, ns[c] - 1], (dev, c)
        for c in range(n):      # cell c's sequence shared by all three cells
            shared = _replay(chem, mech, V, F, K, opts, hs[c], ns[c:c + 1], dev)
            assert shared[0][c].tobytes() == tv[c].tobytes() and shared[3][c, 0] == tth[c, 0] and shared[4][c, :ns[c]].tobytes() == err[c, :ns[c]].tobytes()
            own = _replay(chem, mech, V, F, K, opts, np.tile(hs[c], (n, 1)), np.full(n, ns[c], np.int32), dev)
            for a, b in zip(shared, own):
                assert a.tobytes() == b.tobytes(), (dev, c, "shared row against the same row per cell")
    g = load_golden(mech)
    want = RP.restated(mech, g, 0, (name,))[name]
    cap = max(len(w[5]) for w in want)
    hs, ns = np.full((n, cap), np.nan), np.zeros(n, np.int32)      # (NaN behind every row's count: never read)
    for c, (w, b) in enumerate(zip(want, RT.restated(mech, g, 0, (name,))[name])):
        h = RP.accepted(b[5])
        hs[c, :h.size], ns[c] = h, h.size
    got = {dev: _replay(chem, mech, V, F, K, opts, hs, ns, dev) for dev in (False, True)}
    for a, b in zip(got[False], got[True]):      # (one kernel on the same arguments)
        assert a.tobytes() == b.tobytes(), "host against device form"
    var, ierr, stats, th, err = got[True]
    worst_v, worst_e = 0.0, 0.0
    for c, w in enumerate(want):
        assert ierr[c] == w[1] == 1 and np.array_equal(stats[c], w[2]) and th[c, 0] == w[3] and th[c, 1] == w[4], (c, stats[c], w[2])
        worst_v = max(worst_v, rb.var_diff(var[c], w[0]))
        worst_e = max(worst_e, rb.err_diff(err[c, :ns[c]], w[5]))
    print("%s %s: VAR %.3e (bound %.1e), Err %.3e (bound %.1e), steps %s" % (mech, name, worst_v, rb.REPLAY_RTOL[mech], worst_e, rb.REPLAY_ERR_RTOL[mech], ns.tolist()))
    assert worst_v <= rb.REPLAY_RTOL[mech] and worst_e <= rb.REPLAY_ERR_RTOL[mech]


def test_p2_table_edges_and_batch_edges(chem):
    """gas.  A shared count of 0, 1 and cap; rows per cell with counts 0, 1 and full in one batch, and the same batch reversed; batches of 1, 3 and 65:
    every cell is its own single-cell replay of that many steps, bit for bit, host and device form.  No step: var_out = var_in, ierr 1, zeros."""
    mech = "gas"
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, "atol_1e-15")
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, False)
    cap = int(ns.max())
    hs = np.ascontiguousarray(hs[:, :cap])
    single = {}      # (cell, count) -> the single-cell host replay along the first `count` steps of the cell's own row

    def one(c, k):
        if (c, k) not in single:
            single[c, k] = _replay(chem, mech, V[c:c + 1], F[c:c + 1], K[c:c + 1], opts, hs[c], np.array([k], np.int32), False)
        return single[c, k]

    none = one(0, 0)
    assert none[0].tobytes() == V[:1].tobytes() and none[1][0] == 1 and not none[2].any() and none[3][0, 0] == R.TIN and none[3][0, 1] == 0.0 and not none[4].any()
    for dev in (False, True):
        row = np.ascontiguousarray(hs[0, :ns[0]])      # shared: cell 0's row, cut to its count so that the last case is nstep = cap
        for k in (0, 1, int(ns[0])):
            got = _replay(chem, mech, V, F, K, opts, row, np.array([k], np.int32), dev)
            ref = _replay(chem, mech, V[:1], F[:1], K[:1], opts, row, np.array([k], np.int32), False)
            assert all(a[:1].tobytes() == b.tobytes() for a, b in zip(got, ref)), (dev, k)
            assert (got[2][:, 2] == k).all()
        for order in ((0, 1, 2), (2, 1, 0)):
            idx = np.array(order)
            counts = np.array([0, 1, ns[idx[2]]], np.int32)
            got = _replay(chem, mech, V[idx], F[idx], K[idx], opts, hs[idx], counts, dev)
            for r, c in enumerate(idx):
                ref = one(int(c), int(counts[r]))
                k = int(counts[r])
                assert got[0][r].tobytes() == ref[0][0].tobytes() and got[1][r] == 1 and np.array_equal(got[2][r], ref[2][0]), (dev, order, r)
                assert got[3][r].tobytes() == ref[3][0].tobytes() and got[4][r, :k].tobytes() == ref[4][0, :k].tobytes() and not got[4][r, k:].any(), (dev, order, r)
        for n in (1, 3, 65):
            idx = np.arange(n) % 3
            counts = np.array([ns[c] - (r // 3) % 2 for r, c in enumerate(idx)], np.int32)      # every other triple one step short
            got = _replay(chem, mech, V[idx], F[idx], K[idx], opts, hs[idx], counts, dev)
            for r, c in enumerate(idx):
                ref = one(int(c), int(counts[r]))
                assert got[0][r].tobytes() == ref[0][0].tobytes() and np.array_equal(got[2][r], ref[2][0]) and got[3][r].tobytes() == ref[3][0].tobytes(), (dev, n, r)


@pytest.mark.parametrize("mech", MECHS)
def test_p3_buffers(chem, mech):
    """Through C, host and device form, three cells with rows per cell in arrays of four rows: hsteps NaN behind every count, err_log poisoned — its
    entries behind a count and every array's spare row keep their poison; var_in aliasing var_out gives the same bits."""
    import torch
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, "base")
    ipar, rpar, atol, rtol = opts
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, False)
    n, nvar, cap = 3, V.shape[1], int(ns.max()) + 2
    ref = _replay(chem, mech, V, F, K, opts, hs, ns, False)
    H = np.full((n + 1, cap), np.nan)
    for c in range(n):
        H[c, :ns[c]] = hs[c, :ns[c]]
    N = np.concatenate([ns, [cap]]).astype(np.int32)
    L = chem.lib()
    o = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip))
    for dev in (False, True):
        for alias in (False, True):
            pad = lambda x: np.concatenate([x, np.full((1,) + x.shape[1:], -3.5)])  # noqa: E731
            host = {"var": pad(V), "out": np.full((n + 1, nvar), -1.5), "ierr": np.full(n + 1, -70, np.int32), "stats": np.full((n + 1, 8), -90, np.int32),
                    "th": np.full((n + 1, 2 if dev else 3), -3.25), "err": np.full((n + 1, cap), -7.25)}
            if dev:
                d = {k: _T(v) for k, v in host.items()}
                dF, dK, dH, dN = _T(pad(F)), _T(pad(K)), _T(H), _T(N)
                out = d["var"] if alias else d["out"]
                rc = L.mistra_chem_rosenbrock_replay_device(MID[mech], n, d["var"].data_ptr(), dF.data_ptr(), dK.data_ptr(), R.TIN, R.TOUT, *o, cap, n, dH.data_ptr(),
                                                            dN.data_ptr(), out.data_ptr(), d["ierr"].data_ptr(), d["stats"].data_ptr(), d["th"].data_ptr(),
                                                            d["err"].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, L.mistra_chem_last_error()
                torch.cuda.synchronize()
                got = {k: v.cpu().numpy() for k, v in d.items()}
            else:
                got = host
                out = got["var"] if alias else got["out"]
                rc = L.mistra_chem_rosenbrock_replay_ex(MID[mech], n, got["var"].ctypes.data_as(_dp), pad(F).ctypes.data_as(_dp), pad(K).ctypes.data_as(_dp), R.TIN, R.TOUT,
                                                        *o, cap, n, H.ctypes.data, N.ctypes.data, out.ctypes.data_as(_dp), got["ierr"].ctypes.data_as(_ip),
                                                        got["stats"].ctypes.data_as(_ip), got["th"].ctypes.data_as(_dp), got["err"].ctypes.data_as(_dp))
                assert rc == 0, L.mistra_chem_last_error()
            res = got["var"] if alias else got["out"]
            what = (dev, alias)
            assert res[:n].tobytes() == ref[0].tobytes() and np.array_equal(got["ierr"][:n], ref[1]) and np.array_equal(got["stats"][:n], ref[2]), what
            assert np.ascontiguousarray(got["th"][:n, :2]).tobytes() == ref[3].tobytes(), what
            if not dev:
                assert np.array_equal(got["th"][:n, 2], got["th"][:n, 1]), what
            for c in range(n):
                assert got["err"][c, :ns[c]].tobytes() == ref[4][c, :ns[c]].tobytes() and (got["err"][c, ns[c]:] == -7.25).all(), (what, c)
            assert (got["err"][n] == -7.25).all() and (got["ierr"][n] == -70) and (got["stats"][n] == -90).all() and (got["th"][n] == -3.25).all(), what
            assert (res[n] == (-3.5 if alias else -1.5)).all() and (alias or got["var"].tobytes() == pad(V).tobytes()), what


def test_p3_rows_per_cell_from_host_memory(chem):
    """gas, cells on the device and the table in host memory.  Through chem (what accepted_steps returns, passed straight on): the table is uploaded, the
    bytes are those of the call with tensors.  Through C: host addresses with hrows = ncell are refused with a text, no kernel runs and nothing is written."""
    import torch
    mech = "gas"
    V, F, K = _cells(mech)
    opts = ipar, rpar, atol, rtol = RT.trace_set(mech, "base")
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, True)
    want = _replay(chem, mech, V, F, K, opts, hs, ns, True)
    got = _np(chem.rosenbrock_replay(mech, _T(V), _T(F), _T(K), R.TIN, R.TOUT, hs, ns, *opts))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    dV, dF, dK = _T(V), _T(F), _T(K)
    out, ierr, stats = _T(np.full(V.shape, -7.25)), _T(np.full(3, 77, np.int32)), _T(np.full((3, 8), 77, np.int32))
    err = _T(np.full(hs.shape, -7.25))
    L = chem.lib()
    for h, n in ((hs.ctypes.data, ns.ctypes.data), (_T(hs).data_ptr(), ns.ctypes.data), (hs.ctypes.data, _T(ns, np.int32).data_ptr())):
        rc = L.mistra_chem_rosenbrock_replay_device(MID[mech], 3, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), R.TIN, R.TOUT, atol.ctypes.data_as(_dp),
                                                    rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip), hs.shape[1], 3, h, n, out.data_ptr(),
                                                    ierr.data_ptr(), stats.data_ptr(), None, err.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0 and b"not device arrays" in L.mistra_chem_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.25).all() and (ierr.cpu().numpy() == 77).all() and (err.cpu().numpy() == -7.25).all()


def test_p3_a_capacity_above_the_shared_limit_with_a_short_sequence(chem):
    """gas, device form: a shared row in a table of capacity 5000 (above MISTRA_REPLAY_MAX_SHARED) whose count is a handful of steps runs — only the
    steps travel — and gives the bytes of the call with the row cut to its count; NaN behind the count is never read"""
    mech = "gas"
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, "base")
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, True)
    k = int(ns[0])
    want = _replay(chem, mech, V, F, K, opts, np.ascontiguousarray(hs[0, :k]), ns[:1], True)
    got = _replay(chem, mech, V, F, K, opts, np.concatenate([hs[0, :k], np.full(5000 - k, np.nan)]), ns[:1], True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], want[:4]))
    assert got[4].shape == (3, 5000) and got[4][:, :k].tobytes() == want[4].tobytes() and not got[4][:, k:].any()


@pytest.mark.parametrize("mech", MECHS)
def test_p9_nothing_else_moved(chem, mech):
    """The step-control trace and the operators, host entries, three cells with INTEGRATE_x's options (tests/ros_parent_bits.py): every output has the
    bytes the library gave before the trace units held the replay kernel (tests/golden/parent_bits_<mech>.npz, taken on an MI355X at the parent commit)"""
    import ros_parent_bits as PB
    want = np.load(os.path.join(REPO, "tests", "golden", "parent_bits_%s.npz" % mech))
    got = PB.compute(chem, mech, load_golden(mech))
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.ascontiguousarray(got[k]).tobytes() == want[k].tobytes(), k
    assert (want["trace_ierr"] == 1).all() and (want["trace_n"] > 0).all() and not want["ops_ising"].any() and np.abs(want["ops_x"]).max() > 0.0


def _first_order_losses(t):
    """(reaction, species) for reactions A = k*V(s) whose only effect on s is the loss -A: Jac0(s,s) gets exactly -k from it (as
    tests/test_gpu_ros_trace.py::test_t5 crafts its cell)"""
    out = []
    for r in range(t.nreact):
        fac = t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]]
        if len(fac) != 1 or fac[0] >= t.nvar:
            continue
        s = int(fac[0])
        terms = [(int(t.vd_idx[p]), float(t.vd_coef[p])) for p in range(t.vd_ptr[s], t.vd_ptr[s + 1])]
        if (r, -1.0) in terms:
            out.append((r, s))
    return out


@pytest.mark.parametrize("mech", MECHS)
def test_p4_error_exits(chem, mech):
    """A step of 1e-30 behind two good ones: -7 with the state, T, Hexit and counters of the two.  The first-order-loss cell of
    test_gpu_ros_trace.py::test_t5 at its singular H as the second step: -8, Nsng = 1, Ndec one more than Nacc, the row in singular_rows, the state the
    first step's.  A row of tolerances refused with -5 among good ones (cells form): unchanged, zeros, its err_log row untouched."""
    from mistra_amd import mechtab
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, "base")
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, False)
    for dev in (False, True):
        seq = np.array([hs[0, 0], hs[0, 1], 1.0e-30, hs[0, 2]])
        two = _replay(chem, mech, V, F, K, opts, seq[:2], np.array([2], np.int32), dev)
        got = _replay(chem, mech, V, F, K, opts, seq, np.array([4], np.int32), dev, err_log=np.full((3, 4), -7.25))
        assert (got[1] == -7).all() and (two[1] == 1).all() and got[0].tobytes() == two[0].tobytes() and np.array_equal(got[2], two[2]), dev
        assert got[3].tobytes() == two[3].tobytes() and got[4][:, :2].tobytes() == two[4].tobytes() and (got[4][:, 2:] == -7.25).all(), dev
    t = mechtab.load(mech)
    r, s = _first_order_losses(t)[0]
    V1, F1 = V[:1], F[:1]
    K1 = np.zeros((1, t.nreact))
    hsing = 1.0e-3
    K1[0, r] = -1.0 / (hsing * GAMMA1)
    for dev in (False, True):
        seq = np.array([0.25e-3, hsing, 0.25e-3])
        first = _replay(chem, mech, V1, F1, K1, opts, seq[:1], np.array([1], np.int32), dev, tend=1.5e-3)
        got = _replay(chem, mech, V1, F1, K1, opts, seq, np.array([3], np.int32), dev, tend=1.5e-3, err_log=np.full((1, 3), -7.25))
        assert first[1][0] == 1 and got[1][0] == -8 and got[0].tobytes() == first[0].tobytes() and got[3].tobytes() == first[3].tobytes(), (dev, got[1], got[2])
        # (the failing step has made its Fun_x calls in front of the matrix: a whole step's less stage 2's)
        assert got[2][0].tolist() == [first[2][0, 0] + (first[2][0, 0] - 1), 2, 1, 1, 0, 2, 3, 1], (dev, got[2], first[2])
        assert got[4][0, 0] == first[4][0, 0] and (got[4][0, 1:] == -7.25).all(), dev
        if not dev:
            assert chem.singular_rows(mech, 0)[0] == s + 1
    at, rt = np.full((3, 1), 1.0e-25), np.full((3, 1), 1.0e-3)
    rt[1, 0] = 1.0
    ipar, rpar = opts[0], opts[1]
    for dev in (False, True):
        args = (_T(V), _T(F), _T(K)) if dev else (V, F, K)
        tol = (_T(at), _T(rt)) if dev else (at, rt)
        rows = (_T(hs), _T(ns, np.int32)) if dev else (hs, ns)
        log = np.full((3, hs.shape[1]), -7.25)
        got = _np(chem.rosenbrock_replay_cells(mech, *args, R.TIN, R.TOUT, *rows, ipar, rpar, *tol, err_log=_T(log) if dev else log))
        ref = _replay(chem, mech, V, F, K, opts, hs, ns, dev)
        assert got[1].tolist() == [1, -5, 1] and got[0][1].tobytes() == V[1].tobytes() and not got[2][1].any() and not got[3][1].any(), dev
        assert (got[4][1] == -7.25).all(), dev
        for c in (0, 2):
            assert got[0][c].tobytes() == ref[0][c].tobytes() and np.array_equal(got[2][c], ref[2][c]) and got[4][c, :ns[c]].tobytes() == ref[4][c, :ns[c]].tobytes(), (dev, c)


def test_p5_two_queued_calls_keep_their_own_sequences(chem):
    """tot, two device calls with different shared sequences queued back to back on one stream before any synchronisation: each equals its own
    synchronous call, the two differ"""
    import torch
    mech = "tot"
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, "base")
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, True)
    seqs = [(hs[0], ns[0:1]), (hs[2], ns[2:3])]
    want = [_replay(chem, mech, V, F, K, opts, h, n, True) for h, n in seqs]
    assert want[0][0].tobytes() != want[1][0].tobytes()
    dV, dF, dK = _T(V), _T(F), _T(K)
    queued = [chem.rosenbrock_replay(mech, dV, dF, dK, R.TIN, R.TOUT, h, n, *opts) for h, n in seqs]
    torch.cuda.synchronize()
    for q, w in zip(queued, want):
        for a, b in zip(_np(q), w):
            assert a.tobytes() == b.tobytes()


def test_p6_two_device_slots_split_65_cells(chem):
    """init_devices([0, 0]): 65 tot cells, ragged over two slots, rows per cell with counts that differ, give the one-device results bit for bit; the
    shared row and the cells form (one row refused with -5 in the second slot's block) likewise"""
    mech = "tot"
    V3, F3, K3 = _cells(mech)
    opts = RT.trace_set(mech, "rtol_1e-2_atol_1e-12")
    _, hs3, ns3, _ = _traced(chem, mech, V3, F3, K3, opts, False)
    idx = np.arange(65) % 3
    V, F, K = (np.ascontiguousarray(x[idx]) for x in (V3, F3, K3))
    hs = np.ascontiguousarray(hs3[idx][:, :int(ns3.max())])
    ns = np.array([ns3[c] - (r // 3) % 3 for r, c in enumerate(idx)], np.int32)
    at, rt = np.full((65, 1), 1.0e-12), np.full((65, 1), 1.0e-2)
    rt[40, 0] = 1.0
    calls = {"rows per cell": lambda: _replay(chem, mech, V, F, K, opts, hs, ns, False),
             "shared row": lambda: _replay(chem, mech, V, F, K, opts, hs3[1], ns3[1:2], False),
             "cells form": lambda: _np(chem.rosenbrock_replay_cells(mech, V, F, K, R.TIN, R.TOUT, hs, ns, opts[0], opts[1], at, rt))}
    one = {k: f() for k, f in calls.items()}
    assert (one["rows per cell"][1] == 1).all() and np.array_equal(one["rows per cell"][2][:, 2], ns) and one["cells form"][1][40] == -5
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    for k, f in calls.items():
        for a, b in zip(f(), one[k]):
            assert a.tobytes() == b.tobytes(), k


def test_p7_sensitivities(chem):
    """chem.sensitivities on the bounds file's daylight gas cell: its one launch of 2P+1 cells equals 2P+1 single-cell replays bit for bit, the base
    state is the traced call's, and dy lies within the state bound divided by eps*|p| of the restatement's."""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    mech = "gas"
    g = load_golden(mech, rb.IND_SET)
    c = rb.IND_CELL
    cell = (g["var_in"][c], g["fix"][c], g["rconst"][c])
    ipar, rpar, atol, rtol = opts = rb.ind_options()
    params, eps = list(rb.IND_PARAMS), rb.IND_EPS
    s = chem.sensitivities(mech, *cell, R.TIN, R.TOUT, atol, rtol, rpar, ipar, params, eps)
    assert s.dy.shape == (3, cell[0].size) and (s.ierr == 1).all() and s.nsteps > 0 and 0.0 < s.max_err
    (tv, _, _, _), hs, ns, _ = _traced(chem, mech, *(x[None, :] for x in cell), opts, False)
    assert s.var.tobytes() == tv[0].tobytes() and s.nsteps == ns[0]
    v, f, r, p = chem.sensitivity_cells(mech, *cell, params, eps)
    ends = np.stack([_replay(chem, mech, v[k:k + 1], f[k:k + 1], r[k:k + 1], opts, hs[0], ns[:1], False)[0][0] for k in range(2 * len(params) + 1)])
    assert ((ends[1::2] - ends[2::2]) / (2.0 * eps * p)[:, None]).tobytes() == s.dy.tobytes() and ends[0].tobytes() == s.var.tobytes()
    # against the restatement, along the restated trace's steps on both sides
    o, diag = Oracle(mech), mechtab.load(mech).diag
    hr = RP.accepted(RT.rosenbrock_trace(o, diag, *cell, *opts)[5])
    want = RP.sensitivity_restated(o, diag, *cell, opts, params, eps, hr)
    got = _replay(chem, mech, v, f, r, opts, hr, np.array([hr.size], np.int32), True)[0]
    dy = (got[1::2] - got[2::2]) / (2.0 * eps * p)[:, None]
    base = RP.rosenbrock_replay(o, diag, *cell, *opts, hr)[0]
    for k in range(len(params)):
        bound = rb.dy_bound(mech, base, p[k], eps)
        worst = float((np.abs(dy[k] - want[k]) / bound).max())
        print("parameter %s: largest |dy - restated| / bound %.3e" % (params[k], worst))
        assert worst <= 1.0, (params[k], worst)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_p8_from_fortran(chem, tmp_path):
    """shim/shim_driver LT: ROSENBROCK_BATCH_REPLAY_t with rows per cell and with one shared row, and ROSENBROCK_BATCH_REPLAY_CELLS_t — the host entry's
    bytes, ERRLOG included and untouched behind every count; a step of 1e-30 gives ros_ErrorMsg_t's lines on unit 6 for every cell"""
    mech = "tot"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, F, K = _cells(mech)
    opts = ipar, rpar, atol, rtol = RT.trace_set(mech, "rtol_1e-2_atol_1e-12")
    _, hs, ns, _ = _traced(chem, mech, V, F, K, opts, False)
    n, nvar = V.shape
    cap = int(ns.max()) + 1
    hs = np.ascontiguousarray(hs[:, :cap])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    bad = hs[:1].copy()
    bad[0, 2] = 1.0e-30
    for what, ntol, rows, counts, lines in (("rows per cell", 0, hs, ns, 0), ("shared row", 0, hs[1:2], ns[1:2], 0), ("cells form", 1, hs, ns, 0),
                                            ("a step too small", 0, bad, ns[:1], n)):
        log = np.full((n, cap), -7.25)
        want = _replay(chem, mech, V, F, K, opts, rows if rows.shape[0] > 1 else rows[0], counts, False, err_log=log)
        with open(fin, "wb") as f:
            np.concatenate([ipar.astype(np.float64), rpar, atol, rtol, [R.TIN, R.TOUT, float(n), float(ntol), float(cap), float(rows.shape[0])],
                            rows.ravel(), counts.astype(np.float64)]).tofile(f)
            for i in range(n):
                np.concatenate([V[i], F[i], K[i]]).tofile(f)
        r = subprocess.run([DRIVER, "LT", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
        got = np.fromfile(fout, np.float64).reshape(n, nvar + 2 + 9 + cap)
        assert got[:, :nvar].tobytes() == want[0].tobytes() and got[:, nvar:nvar + 2].tobytes() == want[3].tobytes(), what
        assert np.array_equal(got[:, nvar + 2].astype(np.int32), want[1]) and np.array_equal(got[:, nvar + 3:nvar + 11].astype(np.int32), want[2]), what
        assert got[:, nvar + 11:].tobytes() == want[4].tobytes() and (want[4][:, -1] == -7.25).all(), what
        assert (want[1] == (-7 if lines else 1)).all(), what
        assert r.stdout.count("Forced exit from Rosenbrock_t") == lines and r.stdout.count("Step size too small") == lines, r.stdout
