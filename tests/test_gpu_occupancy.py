"""Every integrator kernel on a FULL device (-m gpu): tests/occupancy_cases.py's cases.  Per slot of the launch table (capi.cpp: MechDesc::unit, and the
product unit's options kernel of Ros3) first the three cells alone, one launch of 3 workgroups on the idle device, then FILL[mech] copies — twice the
device's resident capacity, copy i = cell i % 3 — in one launch; every output row of copy i must be the row of cell i % 3 of the small launch, byte for
byte.  The small launch of the plain call is tied to the compiled reference's record (IERR, IPAR(11:18)), so the filled one is, through it.

What this is aimed at: the unit kernels' own copies of the LU rounds, look-ahead rings, tail chain and dense block (ros_unit_kernel.hip: compiled once
per unit) under the conditions of production — an LDS base above 0, neighbours on the CU's LDS, SIMDs and scalar cache, loaded memory, workgroups
starting beside others in mid-step.  Every other GPU test of these entries launches 1 .. 65 workgroups.  The supposition this rests on is NOT measured:
that a small launch lands one workgroup per CU, so that the alone-launch is the quiet case.  Where it is wrong the test loses nothing but contrast (the
alone-launch then shares CUs too, and is still tied to the reference's record).

What it has NOT been seen to catch.  Tried once on a scratch build, not in the tree: the series kernels without the workgroup barrier in front of a
leg's reload of FIX into LDS (ros3_kernel.hip: `if (!a.carry_h) lds_barrier()`; aer's per-leg rate constants are reloaded without a barrier, each thread
rewrites the cells it reads back itself, so there was none to take out there).  Every series, series-with-rates, series-with-flux and side-by-side
test stayed green on 1024 aer and 512 tot copies.  The likely reason: the last read of FIX of the leg before lies several barriers back (the step's LU,
solves and error norm follow the last Fun_x), so no wave is that far behind when thread 0 .. NFIX-1 store, loaded device or not; only the flux kernels'
closing pass reads X directly in front of it.  So a green run says that no copy's answer depends on its neighbours or on the load at the timings this
device produces, not that every barrier the code needs is there: a race whose window never opens on the hardware shows neither alone nor filled.

The comparisons run on the device (64-bit patterns, not values: a NaN equals itself, -0.0 is not +0.0); one mask per output comes back."""
import numpy as np
import pytest

import mech_ops_py as MO
import occupancy_cases as OC
import ros_dense_py as RD
import ros_linrates_py as RL
import ros_methods_py as RM
import ros_series_py as RS
import ros_series_rates_py as SR

pytestmark = pytest.mark.gpu
TIN, TOUT = RM.TIN, RM.TOUT
TRACE_CAP = 256
TIMES = np.array(SR.TIMES, np.float64)                     # four legs
OPS_SHIFT = 1.0 / (1.0e-3 * MO.GAMMA1)                     # 1/(H*gamma) of Ros3's first step at INTEGRATE_x's Hstart
MAX_LEGS = 4096                                            # MISTRA_SERIES_MAX_LEGS = MISTRA_REPLAY_MAX_SHARED


@pytest.fixture(scope="module")
def chem():
    """a library initialised anew, on a device that FILL fills twice over"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.finalize()
    c.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for mech in OC.MECHS:
        assert OC.FILL[mech] >= 2 * OC.PER_CU[mech] * cus, ("%s: %d copies do not fill this device's %d CUs twice (%d cells per CU): raise occupancy_cases.FILL"
                                                             % (mech, OC.FILL[mech], cus, OC.PER_CU[mech]))
    return c


# ---- inputs on the device, made once per (mechanism, batch size)
_inputs, _alone = {}, {}


def _T(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype), device=torch.device("cuda", 0))


def _in(mech, n):
    """the device arrays of n interleaved copies (n = 3: the cells themselves): V F K the cells; LF LK ros_series_rates_py.ramp()'s rows per leg; NK
    ros_linrates_py.nodes()' node blocks; AT RT the shared tolerance pair as rows per cell"""
    if (mech, n) not in _inputs:
        V, F, K = OC.cells(mech)
        rV, LF, LK = SR.ramp(mech)
        nV, nLF, NK = RL.nodes(mech)
        assert rV.tobytes() == V.tobytes() and nV.tobytes() == V.tobytes() and nLF.tobytes() == LF.tobytes()
        _, _, atol, rtol = RM.method_set(mech, "m2")[:4]
        _inputs[(mech, n)] = dict(V=_T(OC.fill(V, n)), F=_T(OC.fill(F, n)), K=_T(OC.fill(K, n)), LF=_T(OC.fill_legs(LF, n)), LK=_T(OC.fill_legs(LK, n)),
                                  NK=_T(OC.fill_legs(NK, n)), AT=_T(np.tile(atol, (n, 1))), RT=_T(np.tile(rtol, (n, 1))))
    return _inputs[(mech, n)]


def _opts(mech, method):
    return RM.method_set(mech, "m%d" % method)[:4]


def _sopts(mech, method):
    s = RS.method_series(mech, method)
    return s.ipar, s.rpar, s.atol, s.rtol


# ---- the entries: (chem, mech, method, inputs) -> {output: (tensor, the axis the cells run along)}
def _call(res, th, ax=0, **more):
    out = {"var": (res.var, ax), "ierr": (res.ierr, ax), "stats": (res.stats, ax), "t_h": (th, ax)}
    out.update(more)
    return out


def _series(res, **more):
    return _call(res, res.t_h, 1, **more)


def run_plain(chem, mech, method, d):
    return _call(*chem.rosenbrock(mech, d["V"], d["F"], d["K"], TIN, TOUT, *_opts(mech, method)))


def run_cells(chem, mech, method, d):
    ipar, rpar, _, _ = _opts(mech, method)
    return _call(*chem.rosenbrock_cells(mech, d["V"], d["F"], d["K"], TIN, TOUT, ipar, rpar, d["AT"], d["RT"]))


def run_trace(chem, mech, method, d):
    res, th, tr = chem.rosenbrock_trace(mech, d["V"], d["F"], d["K"], TIN, TOUT, *_opts(mech, method), cap=TRACE_CAP)
    return _call(res, th, ntrace=(tr.n, 0), ctrl=(tr.ctrl, 0), **{"log " + k: (getattr(tr, k), 0) for k in ("t", "h", "err", "share", "species", "code")})


def run_flux(chem, mech, method, d):
    res, th, flux = chem.rosenbrock_flux(mech, d["V"], d["F"], d["K"], TIN, TOUT, *_opts(mech, method))
    return _call(res, th, flux=(flux, 0))


def run_dense(chem, mech, method, d):
    res, th, ys, nout = chem.rosenbrock_dense(mech, d["V"], d["F"], d["K"], TIN, TOUT, RD.LINEAR8, *_opts(mech, method))
    return _call(res, th, ysample=(ys, 1), nout=(nout, 0))


def run_series(chem, mech, method, d, carry=False):
    return _series(chem.rosenbrock_series(mech, d["V"], d["F"], d["K"], TIMES, *_sopts(mech, method), carry_h=carry))


def run_series_carry(chem, mech, method, d):
    return run_series(chem, mech, method, d, True)


def run_series_rates(chem, mech, method, d):
    """rconst_legs = fix_legs = nleg: every leg reloads its own rows"""
    return _series(chem.rosenbrock_series_rates(mech, d["V"], d["LF"], d["LK"], TIMES, *_sopts(mech, method)))


def run_linrates(chem, mech, method, d):
    s, _, _, _ = RL.series_set(mech, "m%d" % method)
    assert s.times.tobytes() == TIMES.tobytes()
    return _series(chem.rosenbrock_series_linrates(mech, d["V"], d["F"], d["NK"], s.times, s.ipar, s.rpar, s.atol, s.rtol))


def run_series_flux(chem, mech, method, d):
    res = chem.rosenbrock_series_flux(mech, d["V"], d["LF"], d["LK"], TIMES, *_sopts(mech, method))
    return _series(res, flux_series=(res.flux, 1))


def run_ops(chem, mech, method, d):
    r = chem.ops(mech, d["V"], d["F"], d["K"], want_vdot=True, want_jvs=True, shift=OPS_SHIFT, fun_rhs=True)
    return {"vdot": (r.vdot, 0), "jvs": (r.jvs, 0), "x": (r.x, 1), "ising": (r.ising, 0)}


def _sequence(chem, mech):
    """the accepted steps of cell 0's trace alone -> hsteps [nsteps]"""
    if (mech, "sequence") not in _alone:
        d = _in(mech, OC.NCELL)
        _, _, tr = chem.rosenbrock_trace(mech, d["V"], d["F"], d["K"], TIN, TOUT, *_opts(mech, OC.ROS3), cap=TRACE_CAP)
        host = lambda x: x.cpu().numpy()
        td = np.stack([host(tr.t), host(tr.h), host(tr.err), host(tr.share)], axis=-1)
        ti = np.stack([host(tr.species), host(tr.code)], axis=-1)
        hs, ns = chem.accepted_steps(td, ti, host(tr.n))
        assert 1 <= ns[0] <= TRACE_CAP
        _alone[(mech, "sequence")] = np.ascontiguousarray(hs[0, :ns[0]])
    return _alone[(mech, "sequence")]


def _replay(chem, mech, d, hs, rows):
    """rows False: the sequence shared (it rides in the call's block); True: as device rows per cell, every row the same sequence"""
    import torch
    ncell = d["V"].shape[0]
    if rows:
        h, n = _T(np.tile(hs, (ncell, 1))), torch.full((ncell,), hs.size, dtype=torch.int32, device=d["V"].device)
    else:
        h, n = hs, np.array([hs.size], np.int32)
    res, th, err_log = chem.rosenbrock_replay(mech, d["V"], d["F"], d["K"], TIN, TOUT, h, n, *_opts(mech, OC.ROS3))
    return _call(res, th, err_log=(err_log, 0))


def run_replay(chem, mech, method, d):
    return _replay(chem, mech, d, _sequence(chem, mech), False)


def run_replay_rows(chem, mech, method, d):
    return _replay(chem, mech, d, _sequence(chem, mech), True)


RUN = {"plain": run_plain, "cells": run_cells, "trace": run_trace, "series": run_series, "series_carry": run_series_carry, "series_rates": run_series_rates,
       "flux": run_flux, "dense": run_dense, "ops": run_ops, "replay": run_replay, "replay_rows": run_replay_rows, "linrates": run_linrates,
       "series_flux": run_series_flux}
assert set(OC.ENTRIES) <= set(RUN)


def alone(chem, mech, entry, method):
    """the entry on the three cells alone, launched once per module and left unchanged"""
    key = (mech, entry, method)
    if key not in _alone:
        import torch
        torch.cuda.synchronize()      # the idle device: nothing of an earlier launch is running
        _alone[key] = RUN[entry](chem, mech, method, _in(mech, OC.NCELL))
        torch.cuda.synchronize()
    return _alone[key]


# ---- the comparison
def _bits(t):
    import torch
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _differ(full, small, axis, idx):
    """full against small's rows idx along `axis` -> numpy bool [ncopy] (axis 0) or [nlead, ncopy] (axis 1): the copy differs (in that leg / sample)"""
    f, s = _bits(full), _bits(small).index_select(axis, idx)
    assert f.shape == s.shape, (tuple(f.shape), tuple(s.shape))
    ne = f != s
    while ne.dim() > axis + 1:
        ne = ne.any(dim=-1)
    return ne.cpu().numpy()


def failures(mech, what, got, want, against="their cell launched alone"):
    """got: an entry's outputs on n copies; want: on the three cells (or, with as many rows as got, row for row) -> the texts of what differs"""
    import torch
    texts = []
    assert got.keys() == want.keys()
    for name, (t, axis) in got.items():
        n = t.shape[axis]
        rows = want[name][0].shape[axis]
        idx = torch.arange(n, device=t.device) % OC.NCELL if rows == OC.NCELL else torch.arange(n, device=t.device)
        ne = _differ(t, want[name][0], axis, idx)
        odd = np.nonzero(ne.any(axis=0) if axis else ne)[0]
        if len(odd):
            text = OC.differing(odd, "%s, output %s" % (what, name), mech, n).replace("their cell launched alone", against)
            if axis:
                text += "; in legs / samples %s, copy %d first in %d" % (np.nonzero(ne.any(axis=1))[0].tolist()[:16], odd[0], int(np.nonzero(ne[:, odd[0]])[0][0]))
            texts.append(text)
    return texts


def hold(mech, what, got, want, against="their cell launched alone"):
    texts = failures(mech, what, got, want, against)
    assert not texts, "\n".join(texts)


def filled(chem, mech, entry, method):
    import torch
    small = alone(chem, mech, entry, method)
    got = RUN[entry](chem, mech, method, _in(mech, OC.FILL[mech]))
    torch.cuda.synchronize()
    hold(mech, "%s %s on %d copies" % (entry, RM.METHOD_NAMES[method], OC.FILL[mech]), got, small)
    return small, got


def _ierr_1(mech, what, outs):
    ierr = outs["ierr"][0].cpu().numpy()
    assert (ierr == 1).all(), "%s %s alone: IERR %s" % (mech, what, ierr.tolist())


# ---- 3. the walk: one test per slot of the table
@pytest.mark.parametrize("mech,entry,variant,method", [pytest.param(mech, *w, id=OC.walk_id(mech, *w)) for mech in OC.MECHS for w in OC.WALK])
def test_filled_launch(chem, mech, entry, variant, method):
    """the slot's entry on the three cells alone, then on FILL[mech] copies: every output of every copy is its cell's, bit for bit"""
    small, _ = filled(chem, mech, entry, method)
    name = RM.METHOD_NAMES[method]
    if entry not in ("ops", "replay"):      # (a replay takes every step whatever its error; cells 1 and 2 run on cell 0's sequence)
        _ierr_1(mech, entry + " " + name, small)
    if entry == "plain":      # the tie to the compiled reference: its record of these three calls
        ierr, stats = OC.reference_record(mech, method)
        got_ierr, got_stats = small["ierr"][0].cpu().numpy(), small["stats"][0].cpu().numpy()
        print("%s %s alone: IERR %s, Nstp %s / the reference's %s" % (mech, name, got_ierr.tolist(), got_stats[:, 2].tolist(), stats[:, 2].tolist()))
        assert ierr is None or np.array_equal(got_ierr, ierr), (got_ierr, ierr)
        assert np.array_equal(got_stats, stats), (got_stats.tolist(), stats.tolist())
        if method == OC.ROS3:      # tolerances per cell, every row the shared pair: the shared-pair call, alone and filled
            hold(mech, "rosenbrock_cells alone", alone(chem, mech, "cells", method), small, "the shared-pair call")
            filled(chem, mech, "cells", method)
    elif entry == "trace":
        ntrace = small["ntrace"][0].cpu().numpy()
        assert (ntrace >= 1).all() and (ntrace <= TRACE_CAP).all(), ntrace      # the whole log is on file: rows behind ntrace are the zeros they were
        hold(mech, "trace alone", {k: small[k] for k in ("var", "ierr", "stats", "t_h")}, alone(chem, mech, "plain", method), "the plain call")
    elif entry == "series":
        if method == OC.ROS3:
            filled(chem, mech, "series_carry", method)
        if method in (OC.ROS3, OC.RODAS4):
            _ierr_1(mech, "series_rates " + name, filled(chem, mech, "series_rates", method)[0])
    elif entry == "dense":
        nout = small["nout"][0].cpu().numpy()
        assert (nout == RD.LINEAR8.size).all(), nout
    elif entry == "replay":
        assert int(small["ierr"][0][0]) == 1      # cell 0 along its own steps
        hold(mech, "replay with rows per cell alone", alone(chem, mech, "replay_rows", method), small, "the replay of the shared sequence")
        filled(chem, mech, "replay_rows", method)


@pytest.mark.parametrize("mech", OC.MECHS)
def test_filled_plain_ros3_twice(chem, mech):
    """the filled plain Ros3 launch twice: the two runs agree (else: run-to-run nondeterminism) and agree with the alone-launch (else, in the same
    rows of both: a dependence on load)"""
    import torch
    small = alone(chem, mech, "plain", OC.ROS3)
    d = _in(mech, OC.FILL[mech])
    a = run_plain(chem, mech, OC.ROS3, d)
    b = run_plain(chem, mech, OC.ROS3, d)
    torch.cuda.synchronize()
    what = "plain ros3 on %d copies" % OC.FILL[mech]
    ab = failures(mech, what, b, a, "the same copy of the first run")
    fa, fb = failures(mech, what + ", first run", a, small), failures(mech, what + ", second run", b, small)
    assert not ab, "RUN-TO-RUN NONDETERMINISM: two runs of one launch differ\n" + "\n".join(ab + fa + fb)
    assert not fa and not fb, "LOAD DEPENDENCE: the two runs agree with each other, in the same rows not with the alone-launch\n" + "\n".join(fa + fb)


# ---- 4. mechanisms side by side: the column driver's three streams
def _side_by_side(chem, jobs):
    """jobs: (mech, entry, method) each on a non-blocking stream of its own, queued without a synchronisation between them"""
    import torch
    small = [alone(chem, *j) for j in jobs]
    inputs = [_in(mech, OC.FILL[mech]) for mech, _, _ in jobs]
    streams = [torch.cuda.Stream() for _ in jobs]
    torch.cuda.synchronize()
    got = []
    for (mech, entry, method), d, s in zip(jobs, inputs, streams):
        with torch.cuda.stream(s):
            got.append(RUN[entry](chem, mech, method, d))
    torch.cuda.synchronize()
    texts = []
    for (mech, entry, method), g, w in zip(jobs, got, small):
        texts += failures(mech, "%s %s on %d copies beside the other two mechanisms" % (entry, RM.METHOD_NAMES[method], OC.FILL[mech]), g, w)
    assert not texts, "\n".join(texts)


def test_three_mechanisms_side_by_side_ros3_series(chem):
    _side_by_side(chem, [(mech, "series", OC.ROS3) for mech in OC.MECHS])


def test_three_mechanisms_side_by_side_method_mix(chem):
    """co-resident kernels of different units: gas Rodas4 flux, aer Ros2 linear rates, tot Ros4 dense"""
    _side_by_side(chem, [("gas", "flux", OC.RODAS4), ("aer", "linrates", 1), ("tot", "dense", 3)])


# ---- 5. the two users of the far end of the call's block (capi.cpp: RosCallRing), at capacity; gas, 3 cells
def _long_series(chem, d, carry):
    times = np.linspace(TIN, TOUT, MAX_LEGS + 1)
    return _series(chem.rosenbrock_series("gas", d["V"], d["F"], d["K"], times, *_sopts("gas", OC.ROS3), carry_h=carry)), times


@pytest.mark.parametrize("carry", (False, True), ids=("carry_h0", "carry_h1"))
def test_series_of_4096_legs(chem, carry):
    """nleg = MISTRA_SERIES_MAX_LEGS: the last time fills the block to its last word.  Equal, in every leg, to two series of 2048 legs, the second
    started from the first's last state (carry_h: and with the first's last Hexit as hstart); and the same again behind a call with a short table"""
    import torch
    d = _in("gas", OC.NCELL)
    opts = _sopts("gas", OC.ROS3)
    whole, times = _long_series(chem, d, carry)
    half = MAX_LEGS // 2
    first = chem.rosenbrock_series("gas", d["V"], d["F"], d["K"], times[:half + 1], *opts, carry_h=carry)
    hstart = first.t_h[half - 1, :, 1].contiguous() if carry else None
    second = chem.rosenbrock_series("gas", first.var[half - 1].contiguous(), d["F"], d["K"], times[half:], *opts, carry_h=carry, hstart=hstart)
    torch.cuda.synchronize()
    assert whole["var"][0].shape[0] == MAX_LEGS and (whole["ierr"][0] == 1).all()
    parts = {k: (torch.cat([getattr(first, k), getattr(second, k)]), 1) for k in ("var", "ierr", "stats", "t_h")}
    hold("gas", "series of %d legs, carry_h %d" % (MAX_LEGS, carry), whole, parts, "two series of 2048 legs")
    short = run_series(chem, "gas", OC.ROS3, d, carry)      # queued directly in front: the ring's next block holds ... what an earlier long call left
    again, _ = _long_series(chem, d, carry)
    torch.cuda.synchronize()
    hold("gas", "series of %d legs behind a series of 4" % MAX_LEGS, again, whole, "the first run")
    hold("gas", "series of 4 legs in front of one of %d" % MAX_LEGS, short, alone(chem, "gas", "series_carry" if carry else "series", OC.ROS3))


def test_replay_of_4096_shared_steps(chem):
    """nsteps = MISTRA_REPLAY_MAX_SHARED on one shared row: 4096 steps and the count cell fill the block.  Equal to the same sequence as device rows per
    cell, which do not ride in the block; and the same again behind a replay with a short table"""
    import torch
    d = _in("gas", OC.NCELL)
    hs = np.full(MAX_LEGS, (TOUT - TIN) / MAX_LEGS)
    assert float(hs.sum()) == TOUT - TIN      # (10 / 4096 is exact: the sequence ends on tend)
    shared, rows = _replay(chem, "gas", d, hs, False), _replay(chem, "gas", d, hs, True)
    torch.cuda.synchronize()
    assert (shared["ierr"][0] == 1).all() and (shared["stats"][0][:, 2] == MAX_LEGS).all() and (shared["t_h"][0][:, 0] == TOUT).all()
    hold("gas", "replay of %d shared steps" % MAX_LEGS, shared, rows, "the replay of the same steps as rows per cell")
    short = run_replay(chem, "gas", OC.ROS3, d)
    again = _replay(chem, "gas", d, hs, False)
    torch.cuda.synchronize()
    hold("gas", "replay of %d shared steps behind a short one" % MAX_LEGS, again, shared, "the first run")
    hold("gas", "short replay in front of one of %d steps" % MAX_LEGS, short, alone(chem, "gas", "replay", OC.ROS3))
