"""A series of Rosenbrock_x calls with the reaction flux of every leg on the GPU (-m gpu): mistra_chem_rosenbrock_series_flux_ex / _device and their cells
forms (kernel VARIANT 11).  The definition is an entry that exists: leg k's flux rows are EXACTLY what
mistra_chem_rosenbrock_flux_device returns for the call that leg k is, and everything else is the series with rates'.  So every comparison here is
bit for bit — against the queued sequence of flux calls on the legs' rows with var_out fed on, and against rosenbrock_series_rates — and there is no
tolerance to choose.  Cells of tests/golden/integrate_<mech>.npz with the ramp of tests/ros_series_rates_py.py; at most 65 cells and 16 legs a launch."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import ros_series_py as RS
import ros_series_rates_py as SR
from conftest import MECHS, REPO

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}
Res = namedtuple("Res", "var ierr stats t_h flux")


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    yield c
    if c.device_count() != 1:      # whatever a test initialised: the other modules' fixtures start from init(0)
        c.finalize()
        c.init(0)
    for mech in MECHS:
        c.clear_options(mech)


_ramps = {}


def _ramp(mech, n=3):
    """(VAR [n, NVAR], leg FIX [4, n, NFIX], leg RCONST [4, n, NREACT]): the ramp's three cells, or n cells made of them (cell c is cell c % 3 with
    its state, FIX and rate constants scaled by factors of its own, so that every cell's rows differ); made once, shared, never written"""
    if (mech, n) not in _ramps:
        V, LF, LK = SR.ramp(mech)
        if n < 3:
            V, LF, LK = V[:n].copy(), LF[:, :n].copy(), LK[:, :n].copy()
        elif n > 3:
            idx, rng = np.arange(n) % 3, np.random.default_rng(23)
            V = V[idx] * rng.uniform(0.9, 1.1, (n, 1))
            LF = LF[:, idx] * rng.uniform(0.99, 1.01, (1, n, 1))
            LK = LK[:, idx] * rng.uniform(0.9, 1.1, (4, n, 1))
        _ramps[(mech, n)] = (V, LF, LK)
        for x in _ramps[(mech, n)]:
            x.setflags(write=False)
    return _ramps[(mech, n)]


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _np(res):
    return Res(*(x.cpu().numpy() for x in res))


def _sflux(chem, mech, V, F, K, s, hstart=None, atol=None, rtol=None, host=False):
    """the entry under test: device (-> t_h [nleg, ncell, 2]) or host (-> [nleg, ncell, 3]); F, K: [ncell, .] shared or [nleg, ncell, .]"""
    import torch
    at, rt = (s.atol, s.rtol) if atol is None else (atol, rtol)
    if host:
        return Res(*chem.rosenbrock_series_flux(mech, V, F, K, s.times, s.ipar, s.rpar, at, rt, hstart=hstart, carry_h=s.carry))
    if atol is not None:
        at, rt = _T(at), _T(rt)
    res = chem.rosenbrock_series_flux(mech, _T(V), _T(F), _T(K), s.times, s.ipar, s.rpar, at, rt, hstart=None if hstart is None else _T(hstart),
                                      carry_h=s.carry)
    torch.cuda.synchronize()
    return _np(res)


def _rates(chem, mech, V, F, K, s, hstart=None, atol=None, rtol=None):
    """the series with rates, device entry, same arguments -> Res with flux None"""
    import torch
    at, rt = (s.atol, s.rtol) if atol is None else (_T(atol), _T(rtol))
    res = chem.rosenbrock_series_rates(mech, _T(V), _T(F), _T(K), s.times, s.ipar, s.rpar, at, rt, hstart=None if hstart is None else _T(hstart),
                                       carry_h=s.carry)
    torch.cuda.synchronize()
    return Res(*(x.cpu().numpy() for x in res), None)


def _sequence(chem, mech, V, F, K, s, hstart=None, atol=None, rtol=None):
    """the definition: nleg calls of the flux device entry queued on one stream, call k with leg k's rows on the state call k-1 left.  carry: the
    previous call's Hexit column as d_hstart; else d_hstart = None behind leg 0."""
    import torch
    dV, dF, dK = _T(V), _T(F), _T(K)
    hs = None if hstart is None else _T(hstart)
    if atol is not None:
        d_at, d_rt = _T(atol), _T(rtol)
    legs = []
    for k in range(len(s.times) - 1):
        t0, t1 = float(s.times[k]), float(s.times[k + 1])
        f, kk = dF[k] if dF.ndim == 3 else dF, dK[k] if dK.ndim == 3 else dK
        if atol is None:
            res, th, fl = chem.rosenbrock_flux(mech, dV, f, kk, t0, t1, s.ipar, s.rpar, s.atol, s.rtol, hstart=hs)
        else:
            res, th, fl = chem.rosenbrock_flux_cells(mech, dV, f, kk, t0, t1, s.ipar, s.rpar, d_at, d_rt, hstart=hs)
        legs.append((res, th, fl))
        dV = res.var
        hs = th[:, 1].contiguous() if s.carry else None
    torch.cuda.synchronize()
    return Res(np.stack([r.var.cpu().numpy() for r, _, _ in legs]), np.stack([r.ierr.cpu().numpy() for r, _, _ in legs]),
               np.stack([r.stats.cpu().numpy() for r, _, _ in legs]), np.stack([th.cpu().numpy() for _, th, _ in legs]),
               np.stack([fl.cpu().numpy() for _, _, fl in legs]))


def _same(a, b, what="", flux=True, nan=False):
    assert np.array_equal(a.ierr, b.ierr), (what, a.ierr.tolist(), b.ierr.tolist())
    assert np.array_equal(a.stats, b.stats), (what, a.stats.tolist(), b.stats.tolist())
    assert a.t_h.shape == b.t_h.shape and a.t_h.tobytes() == b.t_h.tobytes(), (what, a.t_h.tolist(), b.t_h.tolist())
    if nan:      # (a NaN's payload is not part of the contract: NaN where NaN, bytes elsewhere)
        assert np.array_equal(np.isnan(a.var), np.isnan(b.var)) and np.nan_to_num(a.var).tobytes() == np.nan_to_num(b.var).tobytes(), what
        if flux:
            assert np.array_equal(np.isnan(a.flux), np.isnan(b.flux)) and np.nan_to_num(a.flux).tobytes() == np.nan_to_num(b.flux).tobytes(), what
        return
    assert a.var.shape == b.var.shape and a.var.tobytes() == b.var.tobytes(), what
    if flux:
        assert a.flux.shape == b.flux.shape and a.flux.tobytes() == b.flux.tobytes(), what


def _host_as_device(r):
    return r._replace(t_h=r.t_h[..., :2].copy())


def _series(mech, method=2, nleg=4, carry=False):
    return RS.method_series(mech, method)._replace(times=np.array(SR.TIMES[:nleg + 1]), carry=carry)


# ---- 1. one leg is the flux entry
@pytest.mark.parametrize("method", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_f1_one_leg_is_the_flux_entry(chem, mech, method):
    """one leg with both counts 1 (2-D rows, and 3-D ones with one block): every output of rosenbrock_flux_device, bit for bit"""
    import torch
    V, LF, LK = _ramp(mech)
    s = _series(mech, method, 1)
    res, th, fl = chem.rosenbrock_flux(mech, _T(V), _T(LF[1]), _T(LK[1]), 0.0, 2.5, s.ipar, s.rpar, s.atol, s.rtol)
    torch.cuda.synchronize()
    want = Res(res.var.cpu().numpy()[None], res.ierr.cpu().numpy()[None], res.stats.cpu().numpy()[None], th.cpu().numpy()[None], fl.cpu().numpy()[None])
    assert (want.ierr == 1).all() and np.abs(want.flux).max() > 0.0
    for F, K in ((LF[1], LK[1]), (LF[1:2], LK[1:2])):
        _same(_sflux(chem, mech, V, F, K, s), want, (mech, method, F.ndim))


# ---- 2. the ramp is the queued sequence of flux calls
@pytest.mark.parametrize("method", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_f2_the_ramp_is_the_queued_sequence_of_flux_calls(chem, mech, method):
    """four legs: var, ierr, stats, t_h and flux of every leg bit-identical to the four queued calls of the flux device entry with leg k's rows and
    var_out fed on; all five methods.  Ros3 also with the carried first step, with a per-cell first step on leg 0 and with the four combinations of
    the two counts at 1, 2 and 4 legs.  The legs' sums are their own: no leg's row equals the one in front of it."""
    V, LF, LK = _ramp(mech)
    s = _series(mech, method)
    got = _sflux(chem, mech, V, LF, LK, s)
    _same(got, _sequence(chem, mech, V, LF, LK, s), "both of the leg's own")
    assert (got.ierr == 1).all() and all(got.flux[k].tobytes() != got.flux[k + 1].tobytes() for k in range(3))
    if method != 2:
        return
    for nleg in (1, 2, 4):
        for per_f in (False, True):
            for per_k in (False, True):
                F, K = LF[:nleg] if per_f else LF[0], LK[:nleg] if per_k else LK[0]
                _same(_sflux(chem, mech, V, F, K, _series(mech, 2, nleg)), _sequence(chem, mech, V, F, K, _series(mech, 2, nleg)), (nleg, per_f, per_k))
    c = s._replace(carry=True)
    carried = _sflux(chem, mech, V, LF, LK, c)
    _same(carried, _sequence(chem, mech, V, LF, LK, c), "carry_h = 1")
    assert carried.flux[0].tobytes() == got.flux[0].tobytes() and carried.flux[1:].tobytes() != got.flux[1:].tobytes()
    hs = np.array([0.0, 0.5, -1.0])
    for ser in (s, c):
        r = _sflux(chem, mech, V, LF, LK, ser, hstart=hs)
        _same(r, _sequence(chem, mech, V, LF, LK, ser, hstart=hs), "d_hstart, carry %s" % ser.carry)
        assert r.flux[0, 1].tobytes() != got.flux[0, 1].tobytes()


# ---- 3. everything but the flux is the series with rates
@pytest.mark.parametrize("n", (1, 3, 65))
@pytest.mark.parametrize("mech", MECHS)
def test_f3_everything_but_the_flux_is_the_series_with_rates(chem, mech, n):
    """var_series, ierr, stats, t_h bit for bit those of rosenbrock_series_rates_device with the same arguments: 1, 3 and 65 cells; the shared pair with
    the carried first step and a per-cell first step, and the cells form"""
    V, LF, LK = _ramp(mech, n)
    rng = np.random.default_rng(5)
    hs = rng.choice([0.0, 1.0e-4, 0.2], n)
    at, rt = 1.0e-25 * 10.0 ** rng.uniform(0.0, 6.0, (n, 1)), 10.0 ** rng.uniform(-4.0, -2.0, (n, 1))
    s = _series(mech, 2, 4, carry=True)
    _same(_sflux(chem, mech, V, LF, LK, s, hstart=hs), _rates(chem, mech, V, LF, LK, s, hstart=hs), "shared pair", flux=False)
    _same(_sflux(chem, mech, V, LF[0], LK, s, atol=at, rtol=rt), _rates(chem, mech, V, LF[0], LK, s, atol=at, rtol=rt), "cells form", flux=False)


# ---- 4. the barrier between a leg's closing evaluation and the next leg's first Fun_x
@pytest.mark.parametrize("mech", ("aer", "tot"))
def test_f4_many_short_legs_without_carry_and_with_shared_fix(chem, mech):
    """aer and tot (several waves per cell), carry_h = 0 and fix_legs = 1: the one case in which nothing but the barrier VARIANT 11 adds at the head of a
    leg lies between the previous leg's closing evaluation (every wave reads other threads' species out of X) and this leg's first Fun_x (which
    stores Y into X).  16 legs of 0.625 s, 65 cells, rate constants of the leg's own: equal to the 16 queued flux calls, bit for bit.  A race need not
    show in one run: a missing barrier lets a fast wave overwrite X while a slow one still reads it, which depends on timing.  This is the narrowest
    shape in which it can show — 16 leg boundaries x 65 workgroups of 4 / 8 waves — not a proof of absence; the barrier's place is argued in
    ros3_kernel.hip."""
    V, LF, LK = _ramp(mech, 65)
    w = np.linspace(0.0, 1.0, 16)
    K = np.stack([(1 - x) * LK[0] + x * LK[3] for x in w])
    s = _series(mech, 2)._replace(times=0.625 * np.arange(17))
    got = _sflux(chem, mech, V, LF[0], K, s)
    _same(got, _sequence(chem, mech, V, LF[0], K, s))
    assert (got.ierr == 1).all() and np.isfinite(got.flux).all()


# ---- 5. failures and refusals
@pytest.mark.parametrize("mech", MECHS)
def test_f5_failing_legs_and_refusals(chem, mech):
    """Max_no_steps = 3: -6 in every leg with a non-zero flux (the sum closed at Texit with the leg's own rate constants), each leg and the one behind
    it equal to its queued call.  A NaN rate constant in leg 1 of one cell: as the queued calls, the neighbours untouched.  A cells-form row refused
    with -5: +0.0 rows in every leg, the neighbours untouched.  A whole-call refusal (RelTol = 1 on the shared pair: -5): zeros in exactly the call's
    rows of a poisoned array, var = var_in, in stream order."""
    import torch
    V, LF, LK = _ramp(mech)
    n, nreact = V.shape[0], LK.shape[-1]
    s = SR.series_set(mech, "ros3_max_steps_3")[0]
    got = _sflux(chem, mech, V, LF, LK, s)
    _same(got, _sequence(chem, mech, V, LF, LK, s), "Max_no_steps = 3")
    assert (got.ierr == -6).all() and all(np.abs(got.flux[k, c]).max() > 0.0 for k in range(4) for c in range(n))
    s = _series(mech)
    good = _sflux(chem, mech, V, LF, LK, s)
    Kn = LK.copy()
    Kn[1, 1, 7] = np.nan
    got = _sflux(chem, mech, V, LF, Kn, s)
    _same(got, _sequence(chem, mech, V, LF, Kn, s), "NaN rate constant", nan=True)
    assert got.ierr[0, 1] == 1 and (got.ierr[1:, 1] < 0).all(), got.ierr.tolist()
    assert got.flux[:, [0, 2]].tobytes() == good.flux[:, [0, 2]].tobytes() and got.flux[0, 1].tobytes() == good.flux[0, 1].tobytes()
    at, rt = np.full((n, 1), 1.0e-25), np.full((n, 1), 1.0e-3)
    _same(_sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt), good, "rows of the shared pair")
    rt[1, 0] = 1.0      # RelTol >= 1: refused
    for host in (False, True):
        got = _sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt, host=host)
        assert (got.ierr[:, 1] == -5).all() and not got.stats[:, 1].any() and not got.t_h[:, 1].any()
        assert got.flux[:, 1].tobytes() == np.zeros((4, nreact)).tobytes()      # +0.0, every leg
        assert all(got.var[k, 1].tobytes() == V[1].tobytes() for k in range(4))
        assert got.flux[:, [0, 2]].tobytes() == good.flux[:, [0, 2]].tobytes() and got.var[:, [0, 2]].tobytes() == good.var[:, [0, 2]].tobytes()
    _same(_sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt), _sequence(chem, mech, V, LF, LK, s, atol=at, rtol=rt), "refused row")
    # the whole call refused: decided on the host, nothing launched; the device form zeroes the rows in stream order
    bad_rtol = np.ones_like(s.rtol)
    L, nleg, nvar = chem.lib(), 4, V.shape[1]
    d_in = [_T(x) for x in (V, LF, LK)]
    d_out, d_fl = _T(np.full(nleg * n * nvar + 3, np.nan)), _T(np.full((nleg + 1) * n * nreact, np.nan))
    d_ierr, d_stats, d_th = _T(np.full(nleg * n, 77, np.int32)), _T(np.full(nleg * n * 8, 77, np.int32)), _T(np.full(nleg * n * 2, np.nan))
    rc = L.mistra_chem_rosenbrock_series_flux_device(MID[mech], n, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), nleg, nleg, nleg,
                                                     s.times.ctypes.data_as(_dp), s.atol.ctypes.data_as(_dp), bad_rtol.ctypes.data_as(_dp),
                                                     s.rpar.ctypes.data_as(_dp), s.ipar.ctypes.data_as(_ip), d_out.data_ptr(), d_ierr.data_ptr(),
                                                     d_stats.data_ptr(), d_th.data_ptr(), 0, None, C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                                     d_fl.data_ptr())
    assert rc == 0, L.mistra_chem_last_error()
    torch.cuda.synchronize()
    out, fl = d_out.cpu().numpy(), d_fl.cpu().numpy()
    assert (d_ierr.cpu().numpy() == -5).all() and not d_stats.cpu().numpy().any() and not d_th.cpu().numpy().any()
    assert out[:nleg * n * nvar].tobytes() == np.stack([V] * nleg).tobytes() and np.isnan(out[nleg * n * nvar:]).all()
    assert fl[:nleg * n * nreact].tobytes() == np.zeros(nleg * n * nreact).tobytes() and np.isnan(fl[nleg * n * nreact:]).all()
    host = chem.rosenbrock_series_flux(mech, V, LF, LK, s.times, s.ipar, s.rpar, s.atol, bad_rtol)
    assert (host.ierr == -5).all() and host.flux.tobytes() == np.zeros((nleg, n, nreact)).tobytes() and host.var.tobytes() == np.stack([V] * nleg).tobytes()


# ---- 6. memory discipline
@pytest.mark.parametrize("mech", MECHS)
def test_f6_poisoned_caller_arrays(chem, mech):
    """the outputs one leg and one cell larger and poisoned with NaN: nothing outside [nleg][ncell][NREACT] of flux_series (threads with r >= NREACT,
    the last leg's stride) or outside the other outputs' rows is written, through the device and the host entry, shared pair and cells form; and var_in
    may be one leg's block of var_series"""
    import torch
    V, LF, LK = _ramp(mech)
    n, nvar = V.shape
    nreact = LK.shape[-1]
    s = _series(mech, 2, 4, carry=True)
    nleg = 4
    L, mid = chem.lib(), MID[mech]
    want = _sflux(chem, mech, V, LF, LK, s)
    at2, rt2 = np.repeat(s.atol[None], n, 0).copy(), np.repeat(s.rtol[None], n, 0).copy()
    tp, popts = s.times.ctypes.data_as(_dp), (s.rpar.ctypes.data_as(_dp), s.ipar.ctypes.data_as(_ip))

    def outs():
        return (np.full((nleg + 1) * n * nvar + nvar, np.nan), np.full((nleg + 1) * n + 1, 77, np.int32), np.full((nleg + 1) * n * 8 + 8, 77, np.int32),
                np.full((nleg + 1) * n * 3 + 3, np.nan), np.full((nleg + 1) * n * nreact + nreact, np.nan))

    def check(out, ierr, stats, th, fl, thw):
        assert out[:nleg * n * nvar].tobytes() == want.var.tobytes() and np.isnan(out[nleg * n * nvar:]).all()
        assert np.array_equal(ierr[:nleg * n], want.ierr.ravel()) and (ierr[nleg * n:] == 77).all()
        assert np.array_equal(stats[:nleg * n * 8], want.stats.ravel()) and (stats[nleg * n * 8:] == 77).all()
        assert th[:nleg * n * thw].reshape(nleg, n, thw)[..., :2].tobytes() == want.t_h.tobytes() and np.isnan(th[nleg * n * thw:]).all()
        assert fl[:nleg * n * nreact].tobytes() == want.flux.tobytes() and np.isnan(fl[nleg * n * nreact:]).all()

    for cells in (False, True):
        out, ierr, stats, th, fl = outs()
        head = (mid, n, V.ctypes.data_as(_dp), LF.ctypes.data_as(_dp), LK.ctypes.data_as(_dp), nleg, nleg, nleg, tp)
        tail = (1, None, out.ctypes.data_as(_dp), ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp), fl.ctypes.data_as(_dp))
        if cells:
            rc = L.mistra_chem_rosenbrock_series_flux_cells_ex(*head, at2.ctypes.data_as(_dp), rt2.ctypes.data_as(_dp), nvar, *popts, *tail)
        else:
            rc = L.mistra_chem_rosenbrock_series_flux_ex(*head, s.atol.ctypes.data_as(_dp), s.rtol.ctypes.data_as(_dp), *popts, *tail)
        assert rc == 0, L.mistra_chem_last_error()
        check(out, ierr, stats, th, fl, 3)
        out, ierr, stats, th, fl = outs()
        d_in = [_T(x) for x in (V, LF, LK)]
        d_out, d_ierr, d_stats, d_th, d_fl = _T(out), _T(ierr), _T(stats), _T(th[:(nleg + 1) * n * 2 + 2]), _T(fl)
        head = (mid, n, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), nleg, nleg, nleg, tp)
        tail = (d_out.data_ptr(), d_ierr.data_ptr(), d_stats.data_ptr(), d_th.data_ptr(), 1, None, C.c_void_p(torch.cuda.current_stream().cuda_stream),
                d_fl.data_ptr())
        if cells:
            d_at, d_rt = _T(at2), _T(rt2)
            rc = L.mistra_chem_rosenbrock_series_flux_cells_device(*head, d_at.data_ptr(), d_rt.data_ptr(), nvar, *popts, *tail)
        else:
            rc = L.mistra_chem_rosenbrock_series_flux_device(*head, s.atol.ctypes.data_as(_dp), s.rtol.ctypes.data_as(_dp), *popts, *tail)
        assert rc == 0, L.mistra_chem_last_error()
        torch.cuda.synchronize()
        check(d_out.cpu().numpy(), d_ierr.cpu().numpy(), d_stats.cpu().numpy(), d_th.cpu().numpy(), d_fl.cpu().numpy(), 2)
        for x, p in zip(d_in, (V, LF, LK)):      # the inputs are inputs
            assert x.cpu().numpy().tobytes() == p.tobytes()
    # var_in aliases leg 2's block of var_series
    out = torch.full((nleg, n, nvar), float("nan"), dtype=torch.float64, device="cuda")
    out[2] = _T(V)
    res = chem.rosenbrock_series_flux(mech, out[2], _T(LF), _T(LK), s.times, s.ipar, s.rpar, s.atol, s.rtol, carry_h=True, out=out)
    torch.cuda.synchronize()
    _same(_np(res), want, "var_in inside var_series")


# ---- 7. host, device and slots
@pytest.mark.parametrize("mech", MECHS)
def test_f7_host_is_device_and_cells_forms_with_shared_rows(chem, mech):
    """host entry = device entry at 1, 3 and 65 cells; the cells forms with every cell's row the shared pair = the shared-pair forms"""
    s = _series(mech, 2, 4, carry=True)
    for n in (1, 3, 65):
        V, LF, LK = _ramp(mech, n)
        dev = _sflux(chem, mech, V, LF, LK, s)
        _same(_host_as_device(_sflux(chem, mech, V, LF, LK, s, host=True)), dev, ("host", n))
        if n == 3:
            at, rt = np.repeat(s.atol[None, :1], n, 0), np.repeat(s.rtol[None, :1], n, 0)      # (INTEGRATE_x's pair is scalar: one entry per row)
            assert (s.atol == s.atol[0]).all() and (s.rtol == s.rtol[0]).all()
            _same(_sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt), dev, "cells device")
            _same(_host_as_device(_sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt, host=True)), dev, "cells host")


def test_f7_host_form_over_two_slots_ragged_split(chem):
    """gas, 65 cells whose rows all differ, 4 legs: the host entry over two device slots (33 + 32 cells; each slot stages and downloads its own
    [nleg][cells][NREACT] rows) equals the device entry on one slot; shared pair and cells form with a refused row in the second slot's block"""
    mech, n = "gas", 65
    V, LF, LK = _ramp(mech, n)
    s = _series(mech, 2, 4, carry=True)
    rng = np.random.default_rng(17)
    at, rt = 1.0e-25 * 10.0 ** rng.uniform(0.0, 6.0, (n, 1)), 10.0 ** rng.uniform(-4.0, -2.0, (n, 1))
    rt[40, 0] = 1.0
    full, full_cells, full_k = _sflux(chem, mech, V, LF, LK, s), _sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt), _sflux(chem, mech, V, LF, LK[0], s)
    assert (full_cells.ierr[:, 40] == -5).all() and not full_cells.flux[:, 40].any() and (np.delete(full_cells.ierr, 40, axis=1) == 1).all()
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    _same(_host_as_device(_sflux(chem, mech, V, LF, LK, s, host=True)), full, "two slots")
    _same(_host_as_device(_sflux(chem, mech, V, LF, LK, s, atol=at, rtol=rt, host=True)), full_cells, "two slots, cells form")
    _same(_host_as_device(_sflux(chem, mech, V, LF, LK[0], s, host=True)), full_k, "two slots, rconst shared")


def test_f7_two_calls_queued_on_one_stream(chem):
    """two calls with their own arrays, times, counts and nleg queued back to back on one stream: each equals its own synchronous result"""
    import torch
    mech = "tot"
    V, LF, LK = _ramp(mech)
    a = _series(mech, 2, 4, carry=True)
    b = _series(mech, 5, 2)._replace(times=np.array([0.0, 1.0, 3.0]))
    Fa, Ka, Fb, Kb = LF, LK, LF[2], LK[2:4] * 1.01
    want = {"a": _sflux(chem, mech, V, Fa, Ka, a), "b": _sflux(chem, mech, V[::-1], Fb, Kb, b)}
    da, db = [_T(x) for x in (V, Fa, Ka)], [_T(x) for x in (V[::-1], Fb, Kb)]
    torch.cuda.synchronize()
    queued = [chem.rosenbrock_series_flux(mech, *d, x.times, x.ipar, x.rpar, x.atol, x.rtol, carry_h=x.carry) for d, x in ((da, a), (db, b))]
    torch.cuda.synchronize()
    _same(_np(queued[0]), want["a"], "first of two")
    _same(_np(queued[1]), want["b"], "second of two")
    assert queued[0].flux.shape[0] == 4 and queued[1].flux.shape[0] == 2


# ---- 8. from Fortran
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
@pytest.mark.parametrize("mech", ("gas", "tot"))
def test_f8_from_fortran(tmp_path, mech):
    """shim/shim_driver BG / BT: ROSENBROCK_BATCH_SERIES_FLUX_x and ROSENBROCK_BATCH_SERIES_FLUX_CELLS_x on the Max_no_steps set, FLUX(NREACT, NCELL, NLEG)
    — the C host entry's bytes, FLUX included, and ros_ErrorMsg_x's lines on unit 6 for every failed leg and cell"""
    from mistra_amd import chem
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, LF, LK = _ramp(mech)
    s = SR.series_set(mech, "ros3_max_steps_3")[0]
    n, nvar = V.shape
    nreact, nleg = LK.shape[-1], len(s.times) - 1
    chem.init(0)
    for nlr, nlf in ((nleg, 1), (nleg, nleg)):
        F, K = LF if nlf > 1 else LF[1], LK
        want = _sflux(chem, mech, V, F, K, s, host=True)
        assert (want.ierr == -6).all() and np.abs(want.flux).max() > 0.0
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        for ntol in (0, 1):      # 0: the shared pair; 1: one scalar row per cell (the same values)
            with open(fin, "wb") as f:
                np.concatenate([s.ipar.astype(np.float64), s.rpar, s.atol, s.rtol, [float(n), float(nleg), float(s.carry), float(ntol), float(nlr), float(nlf)],
                                s.times]).tofile(f)
                V.tofile(f)
                np.ascontiguousarray(F).tofile(f)
                np.ascontiguousarray(K).tofile(f)
            r = subprocess.run([DRIVER, "B" + mech[0].upper(), str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
            rows = np.fromfile(fout, np.float64).reshape(nleg, n, nvar + 2 + 9 + nreact)      # per leg and cell: VAR, Texit, Hexit, IERR, ISTAT(8), FLUX
            assert rows[..., :nvar].tobytes() == want.var.tobytes(), (nlr, nlf, ntol)
            assert rows[..., nvar:nvar + 2].tobytes() == want.t_h[..., :2].tobytes(), (nlr, nlf, ntol)
            assert np.array_equal(rows[..., nvar + 2].astype(np.int32), want.ierr) and np.array_equal(rows[..., nvar + 3:nvar + 11].astype(np.int32), want.stats)
            assert rows[..., nvar + 11:].tobytes() == want.flux.tobytes(), (nlr, nlf, ntol)
            assert r.stdout.count("Forced exit from Rosenbrock_%s" % mech[0]) == nleg * n and r.stdout.count("No of steps exceeds maximum bound") == nleg * n, r.stdout


# ---- 9. nothing else moved
@pytest.mark.parametrize("mech", MECHS)
def test_f9_the_neighbours_give_the_same_bytes_around_a_series_flux_call(chem, mech):
    """chem.rosenbrock_flux, rosenbrock_series_rates and rosenbrock_series_linrates before and after a series-flux call in the same process: the same
    bytes (the new kernels share their units' launch tables, argument block and staging arenas with them)"""
    import torch
    V, LF, LK = _ramp(mech)
    s = _series(mech)
    nodes = np.concatenate([LK, LK[3:]])

    def neighbours():
        a = chem.rosenbrock_flux(mech, _T(V), _T(LF[1]), _T(LK[1]), 0.0, 2.5, s.ipar, s.rpar, s.atol, s.rtol)
        b = chem.rosenbrock_series_rates(mech, _T(V), _T(LF), _T(LK), s.times, s.ipar, s.rpar, s.atol, s.rtol)
        c = chem.rosenbrock_series_linrates(mech, _T(V), _T(LF), _T(nodes), s.times, s.ipar, s.rpar, s.atol, s.rtol)
        h = chem.rosenbrock_series_rates(mech, V, LF, LK, s.times, s.ipar, s.rpar, s.atol, s.rtol)
        torch.cuda.synchronize()
        parts = list(a[0]) + [a[1], a[2]] + list(b) + list(c)
        return b"".join(x.cpu().numpy().tobytes() for x in parts) + b"".join(np.ascontiguousarray(x).tobytes() for x in h)
    before = neighbours()
    _sflux(chem, mech, V, LF, LK, s)
    _sflux(chem, mech, V, LF, LK, s, host=True)
    assert neighbours() == before
