"""The step-control trace on the GPU (-m gpu): mistra_chem_rosenbrock_trace_ex / _device run Rosenbrock_x (Ros3) in a kernel that also records every
attempt that reaches ros_ErrorNorm_x.  Results: bit-identical to mistra_chem_rosenbrock_ex / _device.  Records: against the restatement
(tests/ros_trace_py.py) within tests/ros_trace_bounds.py, measured on the reference side (tests/test_ros_trace.py).  Cells 0, n/2, n-1 of
integrate_<mech>.npz unless a test says otherwise.  Every buffer handed to the library has one spare row behind the batch and a poison of its own
in every entry."""
import ctypes as C

import numpy as np
import pytest

import ros_options_py as R
import ros_trace_bounds as tb
import ros_trace_py as RT
from conftest import MECHS, load_golden

pytestmark = pytest.mark.gpu
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}
GAMMA1 = R.ROS_GAMMA[0]


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


def _poison(shape, dtype, base):
    """every entry its own value, none of them one a record could hold"""
    n = int(np.prod(shape))
    return (-(base + np.arange(n))).astype(dtype).reshape(shape)


class Call:
    """One call of an entry on n cells with buffers of n + 1 rows; numpy arrays afterwards whichever entry ran"""

    def __init__(self, chem, mech, V, F, K, opts, cap=None, device=False, tstart=R.TIN, tend=R.TOUT, ctrl=True, sync=True):
        import torch
        self.n, self.nvar, self.cap, self.device = V.shape[0], V.shape[1], cap, device
        n, nvar = self.n, self.nvar
        rows = max(cap or 0, 0)
        ipar, rpar, atol, rtol = opts
        self.keep = (ipar, rpar, atol, rtol)
        o = (atol.ctypes.data_as(_dp), rtol.ctypes.data_as(_dp), rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip))
        host = {"out": _poison((n + 1, nvar), np.float64, 1.5), "ierr": _poison(n + 1, np.int32, 70), "stats": _poison((n + 1, 8), np.int32, 90),
                "th": _poison((n + 1, 2 if device else 3), np.float64, 3.5), "td": _poison((n + 1, rows, 4), np.float64, 1000.25),
                "ti": _poison((n + 1, rows, 2), np.int32, 5), "nt": _poison(n + 1, np.int32, 40), "ct": _poison((n + 1, nvar), np.int32, 7)}
        self.poison = {k: v.copy() for k, v in host.items()}
        L = chem.lib()
        if device:
            T = lambda x: torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))  # noqa: E731
            self.dev = {k: T(v) for k, v in host.items()}
            self.inputs = (T(V), T(F), T(K))
            d = self.dev
            args = [MID[mech], n] + [x.data_ptr() for x in self.inputs] + [tstart, tend, *o, d["out"].data_ptr(), d["ierr"].data_ptr(),
                                                                        d["stats"].data_ptr(), d["th"].data_ptr(), None,
                                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)]
            if cap is None:
                rc = L.mistra_chem_rosenbrock_device(*args)
            else:
                rc = L.mistra_chem_rosenbrock_trace_device(*args, cap, d["td"].data_ptr() if rows else None, d["ti"].data_ptr() if rows else None,
                                                           d["nt"].data_ptr(), d["ct"].data_ptr() if ctrl else None)
            assert rc == 0, chem.lib().mistra_chem_last_error()
            if sync:
                self.fetch()
        else:
            h = host
            args = [MID[mech], n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), tstart, tend, *o, h["out"].ctypes.data_as(_dp),
                    h["ierr"].ctypes.data_as(_ip), h["stats"].ctypes.data_as(_ip), h["th"].ctypes.data_as(_dp)]
            if cap is None:
                rc = L.mistra_chem_rosenbrock_ex(*args)
            else:
                rc = L.mistra_chem_rosenbrock_trace_ex(*args, cap, h["td"].ctypes.data_as(_dp) if rows else None,
                                                       h["ti"].ctypes.data_as(_ip) if rows else None, h["nt"].ctypes.data_as(_ip),
                                                       h["ct"].ctypes.data_as(_ip) if ctrl else None)
            assert rc == 0, chem.lib().mistra_chem_last_error()
            self.__dict__.update(host)

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        self.__dict__.update({k: v.cpu().numpy() for k, v in self.dev.items()})
        return self

    def result_bytes(self):
        n = self.n
        return self.out[:n].tobytes(), self.ierr[:n].tobytes(), self.stats[:n].tobytes(), self.th[:n, :2].tobytes()

    def spare_rows_untouched(self, traced=True):
        names = ("out", "ierr", "stats", "th") + (("td", "ti", "nt", "ct") if traced else ())
        return all(np.array_equal(getattr(self, k)[self.n], self.poison[k][self.n]) for k in names)

    def check_log(self, ctrl=True):
        """ntrace = Nstp; rows past min(ntrace, cap) keep their poison, rows before it hold none; ctrl is the histogram of the log where the log
        is complete, and sums to ntrace less the records without a species anyway"""
        n, cap = self.n, self.cap
        assert np.array_equal(self.nt[:n], self.stats[:n, 2]), (self.nt[:n], self.stats[:n, 2])
        for c in range(n):
            k = min(int(self.nt[c]), cap)
            assert np.array_equal(self.td[c, k:], self.poison["td"][c, k:]) and np.array_equal(self.ti[c, k:], self.poison["ti"][c, k:]), c
            if k:
                assert not np.isin(self.ti[c, :k], self.poison["ti"]).any() and (self.ti[c, :k, 0] >= 0).all() and (self.ti[c, :k, 0] <= self.nvar).all(), c
            if ctrl:
                assert (self.ct[c] >= 0).all() and self.ct[c].sum() <= self.nt[c], c
                if k == self.nt[c]:
                    assert np.array_equal(self.ct[c], np.bincount(self.ti[c, :k, 0], minlength=self.nvar + 1)[1:]), c
            else:
                assert np.array_equal(self.ct[c], self.poison["ct"][c]), c
        assert self.spare_rows_untouched()


def _against_restatement(mech, call, want, tstart=R.TIN, tend=R.TOUT, label=""):
    """the kept records of every cell against the restated trace (want: rosenbrock_trace's tuple per cell)"""
    worst = [0.0, 0.0, 0.0, 0.0]
    for c, w in enumerate(want):
        tr = w[5]
        k = min(int(call.nt[c]), call.cap)
        assert call.ierr[c] == w[1] and np.array_equal(call.stats[c], w[2]), (label, c, call.ierr[c], w[1], call.stats[c], w[2])
        assert call.nt[c] == len(tr.t), (label, c)
        assert np.array_equal(call.ti[c, :k, 1], tr.code[:k]), (label, c, call.ti[c, :k, 1], tr.code[:k])
        d = tb.record_diff(tuple(call.td[c, :k, j] for j in range(4)), (tr.t[:k], tr.h[:k], tr.err[:k], tr.share[:k]), tstart, tend)
        worst = [max(a, b) for a, b in zip(worst, d)]
        # species: one whose restated term lies within twice the Err bound of the restated top term; different from the restated top in at most
        # 10 % of the cell's attempts
        got, differ = call.ti[c, :k, 0], 0
        for i in range(k):
            if got[i] == tr.species[i]:
                continue
            differ += 1
            assert got[i] >= 1 and tr.species[i] >= 1, (label, c, i, got[i], tr.species[i])
            top = tr.terms[i, tr.species[i] - 1]
            assert tr.terms[i, got[i] - 1] >= top * (1.0 - 2.0 * tb.TRACE_ERR_RTOL[mech]), (label, c, i, got[i], tr.species[i])
        assert differ <= 0.1 * k, (label, c, differ, k)
    print("%s %s: T %.3e (bound %.1e), H %.3e (%.1e), Err %.3e (%.1e), share %.3e (%.1e), attempts %s" %
          (mech, label, worst[0], tb.TRACE_T_TOL[mech], worst[1], tb.TRACE_H_RTOL[mech], worst[2], tb.TRACE_ERR_RTOL[mech], worst[3],
           tb.TRACE_SHARE_TOL[mech], call.nt[:call.n].tolist()))
    assert worst[0] <= tb.TRACE_T_TOL[mech] and worst[1] <= tb.TRACE_H_RTOL[mech], (label, worst)
    assert worst[2] <= tb.TRACE_ERR_RTOL[mech] and worst[3] <= tb.TRACE_SHARE_TOL[mech], (label, worst)


@pytest.mark.parametrize("name", RT.SET_NAMES)
@pytest.mark.parametrize("mech", MECHS)
def test_t1_results_are_the_untraced_calls_and_records_the_restatements(chem, mech, name):
    """Per mechanism and option set, host and device entry, cap = 0, 5 and 256: VAR, ierr, stats, Texit, Hexit bit-identical to the untraced entry;
    ntrace = Nstp also past cap; codes identical to the restatement's, T, H, Err, share within the bounds file, species by the rule above; ctrl the
    histogram of the log; untouched rows keep their poison; the Python surface returns the same arrays."""
    import torch
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, name)
    want = RT.restated(mech, load_golden(mech), 0, (name,))[name]
    plain = {dev: Call(chem, mech, V, F, K, opts, None, dev) for dev in (False, True)}
    assert plain[False].result_bytes() == plain[True].result_bytes()
    assert plain[False].spare_rows_untouched(False) and plain[True].spare_rows_untouched(False)
    full = {}
    for dev in (False, True):
        for cap in (0, 5, 256):
            call = Call(chem, mech, V, F, K, opts, cap, dev)
            assert call.result_bytes() == plain[dev].result_bytes(), (dev, cap)
            call.check_log()
            _against_restatement(mech, call, want, label="%s %s cap %d" % (name, "device" if dev else "host", cap))
            if cap == 5:
                assert (call.nt[:call.n] > cap).all()      # every one of these cells takes more than five attempts
            full[dev] = call
        assert (full[dev].nt[:3] <= 256).all()
    for k in ("td", "ti", "nt", "ct"):
        assert np.array_equal(getattr(full[False], k), getattr(full[True], k), equal_nan=(k == "td")), k
    # without ctrl: nothing is written there; through the Python surface: the same arrays, numpy and torch
    Call(chem, mech, V, F, K, opts, 5, True, ctrl=False).check_log(ctrl=False)
    ref = full[False]
    res, th, tr = chem.rosenbrock_trace(mech, V, F, K, R.TIN, R.TOUT, *opts, cap=256)
    dres, dth, dtr = chem.rosenbrock_trace(mech, *(torch.tensor(x, device="cuda:0") for x in (V, F, K)), R.TIN, R.TOUT, *opts, cap=256)
    torch.cuda.synchronize()
    for r, t, x in ((res, th, tr), (dres, dth, dtr)):
        host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a  # noqa: E731
        assert (host(r.var).tobytes(), host(r.ierr).tobytes(), host(r.stats).tobytes(), np.ascontiguousarray(host(t)[:, :2]).tobytes()) == ref.result_bytes()
        assert np.array_equal(host(x.n), ref.nt[:3]) and np.array_equal(host(x.ctrl), ref.ct[:3])
        for c in range(3):
            k = int(ref.nt[c])
            for j, f in enumerate((x.t, x.h, x.err, x.share)):
                assert np.array_equal(host(f)[c, :k], ref.td[c, :k, j]), (c, j)
                assert not host(f)[c, k:].any()
            assert np.array_equal(host(x.species)[c, :k], ref.ti[c, :k, 0]) and np.array_equal(host(x.code)[c, :k], ref.ti[c, :k, 1])


def test_t2_batch_edges(chem):
    """gas, ncell = 1, 3 and 65 (the three cells tiled): every row's results and records are those of its cell in the batch of three, bit for bit,
    through both entries"""
    mech = "gas"
    V, F, K = _cells(mech)
    opts = RT.trace_set(mech, "atol_1e-15")
    three = Call(chem, mech, V, F, K, opts, 16)
    three.check_log()
    for n in (1, 3, 65):
        idx = np.arange(n) % 3
        for dev in (False, True):
            call = Call(chem, mech, np.ascontiguousarray(V[idx]), np.ascontiguousarray(F[idx]), np.ascontiguousarray(K[idx]), opts, 16, dev)
            call.check_log()
            assert call.out[:n].tobytes() == three.out[idx].tobytes() and np.array_equal(call.stats[:n], three.stats[idx]), (n, dev)
            assert np.array_equal(call.nt[:n], three.nt[idx]) and np.array_equal(call.ct[:n], three.ct[idx]), (n, dev)
            for r, c in enumerate(idx):
                k = int(three.nt[c])
                assert call.td[r, :k].tobytes() == three.td[c, :k].tobytes() and np.array_equal(call.ti[r, :k], three.ti[c, :k]), (n, dev, r)


@pytest.mark.parametrize("mech", MECHS)
def test_t3_a_refusal_gives_no_attempts_and_writes_nothing(chem, mech):
    """options Rosenbrock_x refuses (IERR -3, -5): the result is the untraced entry's, ntrace = 0, the logs and ctrl keep their poison"""
    V, F, K = _cells(mech)
    for name in ("rpar1_-1", "atol51_0_vector"):
        opts = R.refused_set(mech, name)
        for dev in (False, True):
            plain, call = Call(chem, mech, V, F, K, opts, None, dev), Call(chem, mech, V, F, K, opts, 8, dev)
            assert call.result_bytes() == plain.result_bytes() and (call.ierr[:3] == R.REFUSED_IERR[name]).all(), (name, dev)
            assert not call.nt[:3].any() and call.nt[3] == call.poison["nt"][3]
            for k in ("td", "ti", "ct"):
                assert np.array_equal(getattr(call, k), call.poison[k]), (name, dev, k)


@pytest.mark.parametrize("mech", MECHS)
def test_t4_max_steps_exit(chem, mech):
    """IPAR(3) = 5: IERR -6 after six attempts' worth of steps; the records are the restatement's first ones, ntrace counts them all at cap 4"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    V, F, K = _cells(mech)
    opts = R.option_set(mech, "max_steps_5")
    o, diag = Oracle(mech), mechtab.load(mech).diag
    want = [RT.rosenbrock_trace(o, diag, V[c], F[c], K[c], *opts) for c in range(3)]
    assert all(w[1] == -6 for w in want)
    for cap in (4, 64):
        for dev in (False, True):
            call = Call(chem, mech, V, F, K, opts, cap, dev)
            assert (call.ierr[:3] == -6).all() and call.result_bytes() == Call(chem, mech, V, F, K, opts, None, dev).result_bytes()
            call.check_log()
            _against_restatement(mech, call, want, label="max_steps_5 cap %d" % cap)
    assert (call.nt[:3] > 4).all()


def _first_order_losses(t):
    """(reaction, species) for reactions A = k*V(s) whose only effect on s is the loss -A: Jac0(s,s) gets exactly -k from it"""
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
def test_t5_zero_pivots_show_in_code_and_h(chem, mech):
    """A first-order loss with the negative rate constant k = -1/(H*gamma) puts an exact zero on Ghimj's diagonal at step size H (as
    tests/test_gpu_phases.py crafts it).  One such reaction at H = 1e-3: the first attempt's code carries one halving and its H is 0.5e-3.  Three
    of them, at H, H/2, H/4: three halvings, H = 1.25e-4.  Codes and counters identical to the restatement's."""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    t = mechtab.load(mech)
    o = Oracle(mech)
    g = load_golden(mech)
    losses, seen = [], set()
    for r, s in _first_order_losses(t):
        if s not in seen:
            seen.add(s)
            losses.append((r, s))
    V, F = np.ascontiguousarray(g["var_in"][:1]), np.ascontiguousarray(g["fix"][:1])
    tstart, tend = 0.0, 1.5e-3
    opts = R.base_options(mech)
    for nzero in (1, 3):
        K = np.zeros((1, t.nreact))
        for i in range(nzero):
            K[0, losses[i][0]] = -1.0 / ((1.0e-3 / 2 ** i) * GAMMA1)
        want = [RT.rosenbrock_trace(o, t.diag, V[0], F[0], K[0], *opts, tstart=tstart, tend=tend)]
        assert want[0][2][7] == nzero and want[0][5].code[0] >> 1 == nzero and want[0][5].h[0] == 1.0e-3 / 2 ** nzero
        for dev in (False, True):
            call = Call(chem, mech, V, F, K, opts, 64, dev, tstart, tend)
            assert call.result_bytes() == Call(chem, mech, V, F, K, opts, None, dev, tstart, tend).result_bytes()
            call.check_log()
            assert call.stats[0, 7] == nzero and call.ti[0, 0, 1] >> 1 == nzero and call.td[0, 0, 1] == 1.0e-3 / 2 ** nzero, (nzero, dev)
            assert call.nt[0] <= 64 and np.array_equal(call.ti[0, :call.nt[0], 1], want[0][5].code) and np.array_equal(call.stats[0], want[0][2])
            assert (call.ti[0, 1:call.nt[0], 1] >> 1 == 0).all()


def test_t6_a_nan_cell_terminates_and_follows_the_rules(chem):
    """gas, a NaN in one species: Err is NaN in every attempt, each is rejected and H shrinks until it underflows to 0, where H <= Hmin accepts the
    attempt and the next step ends the call with IERR -7 — 323 attempts, more than the capacity of 300.  Counters, codes, T and H are the
    restatement's (none of them depends on a rounding).  Per record: a species whose restated term is NaN is never named, a named species has a
    NaN share (Err is NaN), species 0 goes with share 0; where the restated top term is far above underflow a species is named; the last attempts, whose error vector is exactly zero where it is not NaN, say species 0, share 0."""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    mech, cap = "gas", 300
    V, F, K = (x[:1].copy() for x in _cells(mech))
    V[0, 10] = np.nan
    opts = R.base_options(mech)
    want = RT.rosenbrock_trace(Oracle(mech), mechtab.load(mech).diag, V[0], F[0], K[0], *opts)
    tr = want[5]
    assert want[1] == -7 and len(tr.t) > cap and np.isnan(tr.err).all() and tr.code[-1] == 1 and not tr.code[:-1].any()
    assert tr.species[-1] == 0 and tr.share[-1] == 0.0 and np.isnan(tr.terms).any(axis=1).all()
    for dev in (False, True):
        call = Call(chem, mech, V, F, K, opts, cap, dev)
        assert call.result_bytes()[1:] == Call(chem, mech, V, F, K, opts, None, dev).result_bytes()[1:]
        assert call.ierr[0] == -7 and np.array_equal(call.stats[0], want[2]) and call.nt[0] == len(tr.t)
        call.check_log()
        assert np.array_equal(call.ti[0, :, 1], tr.code[:cap]) and np.isnan(call.td[0, :, 2]).all()
        assert np.array_equal(call.td[0, :, 0], tr.t[:cap]) and np.array_equal(call.td[0, :, 1], tr.h[:cap])
        for i in range(cap):
            s, share, terms = int(call.ti[0, i, 0]), call.td[0, i, 3], tr.terms[i]
            if s > 0:
                assert not np.isnan(terms[s - 1]) and np.isnan(share), (i, s, share)
            else:
                assert share == 0.0, (i, share)
            if tr.species[i] and terms[tr.species[i] - 1] > 1e-250:      # a top term far above underflow: some species is named
                assert s > 0, (i, tr.species[i])
        # the run's last attempts: H in the denormals, the error vector exactly zero (or NaN) on both sides
        tail = Call(chem, mech, V, F, K, opts, 400, dev)
        k = int(tail.nt[0])
        assert np.array_equal(tail.ti[0, :k, 1], tr.code) and np.array_equal(tail.td[0, :k, 1], tr.h)
        assert not tail.ti[0, k - 3:k, 0].any() and not tail.td[0, k - 3:k, 3].any() and not tr.species[-3:].any()
        assert tail.ct[0].sum() == np.count_nonzero(tail.ti[0, :k, 0])


def test_t7_two_calls_queued_on_one_stream_keep_their_own_traces(chem):
    """tot, INTEGRATE_x's AbsTol and 1e-15 queued back to back on one stream before any synchronisation: each equals its own synchronous call, the
    two differ"""
    mech = "tot"
    V, F, K = _cells(mech)
    sets = ("base", "atol_1e-15")
    want = {name: Call(chem, mech, V, F, K, RT.trace_set(mech, name), 256, True) for name in sets}
    assert not np.array_equal(want["base"].nt, want["atol_1e-15"].nt)
    queued = [Call(chem, mech, V, F, K, RT.trace_set(mech, name), 256, True, sync=False) for name in sets]
    for name, q in zip(sets, queued):
        q.fetch()
        assert q.result_bytes() == want[name].result_bytes(), name
        for k in ("td", "ti", "nt", "ct"):
            assert getattr(q, k).tobytes() == getattr(want[name], k).tobytes(), (name, k)


def test_t8_two_device_slots_ragged_split(chem):
    """init_devices([0, 0]), five gas cells over two slots (3 + 2), the host entries with the shared pair and with rows per cell: every slot stages its
    own rows of the caller's logs and of ctrl and hands them back.  cap is smaller than the longest cell's attempt count, the logs come in
    filled with a sentinel: results, n, ctrl and the logs — the sentinel rows past min(n, cap) too — equal one slot's bit for bit.  Cell 2 of the
    cells form is refused with -5, in the first slot's block: n = 0, its log rows and its ctrl row are the caller's."""
    g = load_golden("gas")
    V, F, K = (np.ascontiguousarray(g[k][:5]) for k in ("var_in", "fix", "rconst"))
    n = 5
    attempts = chem.rosenbrock_trace("gas", V, F, K, R.TIN, R.TOUT, cap=0)[2].n      # (n counts every attempt whatever the capacity)
    lo, hi = int(attempts.min()), int(attempts.max())
    cap = (lo + hi + 1) // 2 if lo < hi else hi - 1      # smaller than the longest cell's count; where the counts differ, larger than the shortest's
    assert 0 < cap < hi, attempts.tolist()
    at = np.array([[1.0e-25], [1.0e-20], [1.0e-22], [1.0e-18], [1.0e-24]])
    rt = np.array([[1.0e-3], [1.0e-4], [1.0], [1.0e-2], [2.0e-3]])

    def both():
        got = []
        for cells in (False, True):
            td, ti = _poison((n, cap, 4), np.float64, 1000.25), _poison((n, cap, 2), np.int32, 5)
            if cells:
                res, th, tr = chem.rosenbrock_trace_cells("gas", V, F, K, R.TIN, R.TOUT, None, None, at, rt, cap=cap, trace_d=td, trace_i=ti)
            else:
                res, th, tr = chem.rosenbrock_trace("gas", V, F, K, R.TIN, R.TOUT, cap=cap, trace_d=td, trace_i=ti)
            got.append({"var": res.var, "ierr": res.ierr, "stats": res.stats, "th": th, "td": td, "ti": ti, "n": tr.n, "ctrl": tr.ctrl})
        return got

    one = both()
    sentinel_d, sentinel_i = _poison((n, cap, 4), np.float64, 1000.25), _poison((n, cap, 2), np.int32, 5)
    plain, cells = one
    assert (plain["ierr"] == 1).all() and np.array_equal(plain["n"], attempts) and (plain["n"] > cap).any()
    assert cells["ierr"][2] == -5 and cells["n"][2] == 0 and (np.delete(cells["ierr"], 2) == 1).all() and (np.delete(cells["n"], 2) > 0).all()
    assert np.array_equal(cells["td"][2], sentinel_d[2]) and np.array_equal(cells["ti"][2], sentinel_i[2]) and not cells["ctrl"][2].any()
    for c in range(n):      # every kept row is written, every row past min(n, cap) is the sentinel's
        k = min(int(plain["n"][c]), cap)
        assert not np.isin(plain["ti"][c, :k], sentinel_i).any() and np.array_equal(plain["td"][c, k:], sentinel_d[c, k:]), c
    try:
        chem.finalize()
        chem.init_devices([0, 0])
        assert chem.device_count() == 2
        two = both()
    finally:
        chem.finalize()
        chem.init(0)
    for a, b, form in zip(two, one, ("shared pair", "cells form")):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (form, k)
