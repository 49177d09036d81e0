"""Dense output of Rosenbrock_x, CPU side: the restatement with the sampling (tests/ros_dense_py.py) against the one without, what
the sample-time sets are there for, the interpolant against an independent evaluation, the bounds of the GPU tests (tests/ros_dense_bounds.py), the
refusals the four dense-output entries make before a device is touched, the tool's CPU path and the series unit that holds the kernel."""
import ctypes as C

import numpy as np
import pytest

import ros_dense_bounds as db
import ros_dense_py as RD
import ros_methods_py as RM
from conftest import MECHS, load_golden

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
FORWARD_DONE = ("m1", "m2", "m3", "m4", "m5", "m4_vector_tol")


# ---- (a), (b), (c)
@pytest.mark.parametrize("mech", MECHS)
def test_restatement_with_the_sampling_equals_the_one_without(mech):
    """(a) VAR, IERR, IPAR(11:18), Texit, Hexit bit for bit on every set used: the closing evaluation is not counted.  (b) On the forward completed
    sets every sample is reached and the one at Tend is VAR bit for bit (th == 1).  (c) The Max_no_steps set ends with -6 and 0 < nout < ns on every
    test cell, the rows behind nout are +0.0, the reached ones are not; the backward set completes on gas with every sample reached, the last one (on
    its Tend = 0) VAR bit for bit."""
    g = load_golden(mech)
    got, want = RD.restated(mech, g), RM.restated(mech, g, 0, RD.DENSE_SETS)
    for name in RD.DENSE_SETS:
        ns = len(RD.times_of(name))
        for i in range(5):
            assert np.asarray(got[name][i]).tobytes() == np.asarray(want[name][i]).tobytes(), (name, i)
        var, ierr, samples, nout = got[name][0], got[name][1], got[name][5], got[name][6]
        assert samples.shape == (3, ns, var.shape[1]) and np.isfinite(samples).all(), name
        for c in range(3):      # always a prefix; behind it +0.0, bytes
            assert 0 <= nout[c] <= ns and samples[c][nout[c]:].tobytes() == np.zeros((ns - nout[c], var.shape[1])).tobytes(), (name, c)
            assert (np.abs(samples[c][:nout[c]]).max(axis=1) > 0).all(), (name, c)
        if name in FORWARD_DONE:
            assert (ierr == 1).all() and (nout == ns).all(), name
            assert samples[:, -1].tobytes() == var.tobytes(), name
    m = got["m5_max_steps_5"]
    assert (m[1] == -6).all() and (m[2][:, 3] >= 1).all() and ((0 < m[6]) & (m[6] < len(RD.MAX_STEPS))).all(), m[6]
    assert set(RD.EARLY_LINEAR8) <= set(RD.MAX_STEPS)
    b = got["m4_backward"]
    if mech == "gas":
        assert (b[1] == 1).all() and (b[6] == len(RD.BACKWARD)).all() and b[5][:, -1].tobytes() == b[0].tobytes()
    else:      # aer and tot are unstable backward: -7 before the first sample time
        assert (b[1] == -7).all() and (b[6] < len(RD.BACKWARD)).all()


def test_sample_time_sets_are_what_they_are_named_for():
    """every set is strictly monotone inside its call's interval, Tstart excluded; `early` has three samples in the first step of a call whose first
    attempt (Hstart = 1e-3) is accepted, the third exactly on its end, and one just behind; `cluster` lies inside one late step of gas Ros3"""
    for name, ts in RD.TIME_SETS.items():
        d = np.diff(ts)
        assert ts.size >= 1 and ((d < 0).all() if name == "backward" else (d > 0).all()), name
        assert (ts >= 0.0).all() and (ts <= 10.0).all() and (ts[0] != (10.0 if name == "backward" else 0.0)), name
        assert ts.size <= RD.MAX_TIMES
    assert RD.LINEAR8.tolist() == [1.25, 2.5, 3.75, 5.0, 6.25, 7.5, 8.75, 10.0] and RD.END.tolist() == [10.0] and RD.CLUSTER.size == 64
    assert (RD.EARLY[:3] <= 1.0e-3).all() and RD.EARLY[2] == 1.0e-3 and RD.EARLY[3] > 1.0e-3
    assert RD.FORWARD[-1] == 10.0 and set(RD.EARLY) | set(RD.CLUSTER) | set(RD.LINEAR8) == set(RD.FORWARD)


# ---- (d)
# The forward rounding bound of hermite(), written out.  u = 2**-53; every operation returns its exact result times (1 + e), |e| <= u; 0 <= th <= 1, so
# |om|, |th|, |1 - 2 th| <= 1 and th*om <= 1/4; S = |Y0| + |Y1| + |dh F0| + |dh F1|, the latter two as computed (their own roundings are in the count).
#   d = Y1 - Y0: one rounding, |d| <= |Y0| + |Y1|.    hf0, hf1: one each.    om, 1 - 2 th: one each (2 th is exact).    th*om: two on top of om's.
#   c: (1 - 2 th)*d carries 3 roundings (e, d, the product), om*hf0 3, their difference 1 more on both, th*hf1 2, the sum 1 more on all three:
#      |c^ - c| <= 5 u (|d| + |hf0| + |hf1|) <= 5 u S, to first order, and |c| <= S.
#   (th*om)*c: the factor's 2 + the product's 1 on |th om c| <= S/4, plus c's own error times 1/4: <= (3/4 + 5/4) u S = 2 u S.
#   om*Y0 + th*Y1: 2 roundings on om*Y0, 1 on th*Y1, the sum 1 on both: <= 3 u (|Y0| + |Y1|) <= 3 u S.
#   the last subtraction: u times the result, <= u (|Y0| + |Y1| + S/4) <= 1.25 u S.
# Sum 6.25 u S; second-order terms are below 40 u^2 S.  The bound held is 8 u S = 4 eps S: the next power of two, nothing measured.  The reference is the
# Hermite BASIS form h00 Y0 + h10 dh F0 + h01 Y1 + h11 dh F1 in np.longdouble (u_l = 2**-64 on x86: its own error, a few u_l S, is 2000 times smaller).
HERMITE_BOUND_U = 8.0


@pytest.mark.parametrize("mech", MECHS)
def test_formula_against_the_hermite_basis_in_long_double(mech):
    from oracle.oracle import Oracle
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than double here: no independent reference"
    g, o = load_golden(mech), Oracle(mech)
    L = np.longdouble
    ths = np.concatenate([[0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 2.0 ** -30, 1.0 - 2.0 ** -30], np.random.default_rng(11).uniform(0.0, 1.0, 25)])
    worst = 0.0
    for c in RD.cells_of(g["var_in"].shape[0]):
        y0, y1, fix, rc = g["var_in"][c], g["var_out"][c], g["fix"][c], g["rconst"][c]
        f0, f1 = o.fun(y0, fix, rc), o.fun(y1, fix, rc)
        for dh in (1.0e-3, 10.0, -0.37):
            hf0, hf1 = dh * f0, dh * f1
            S = np.abs(y0) + np.abs(y1) + np.abs(hf0) + np.abs(hf1)
            for th in ths:
                u = RD.hermite(y0, f0, y1, f1, dh, float(th))
                t = L(float(th))
                h00, h10, h01, h11 = (1 + 2 * t) * (1 - t) ** 2, t * (1 - t) ** 2, t * t * (3 - 2 * t), t * t * (t - 1)
                ref = h00 * y0.astype(L) + h10 * (L(dh) * f0.astype(L)) + h01 * y1.astype(L) + h11 * (L(dh) * f1.astype(L))
                err = np.abs(u.astype(L) - ref).astype(np.float64)
                ok = S > 0
                worst = max(worst, float((err[ok] / S[ok]).max()) / 2.0 ** -53)
                assert (err <= HERMITE_BOUND_U * 2.0 ** -53 * S).all(), (c, dh, th, float((err[ok] / S[ok]).max()) / 2.0 ** -53)
                if th == 1.0:
                    assert u.tobytes() == y1.tobytes()
                if th == 0.0:
                    assert np.array_equal(u, y0)
    print("%s: worst error %.2f u S (bound %.0f u S)" % (mech, worst, HERMITE_BOUND_U))


@pytest.mark.parametrize("method", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_single_step_condition(mech, method):
    """AbsTol = 1e30, RelTol = 0.5, 0 -> 1e-3 s: the restatement makes one attempt, accepted, and its three samples are hermite() of Y_0, Y_1 and the
    oracle's Fun_x at both, bit for bit — what the GPU's exact test (d2) rests on"""
    from oracle.oracle import Oracle
    g, o = load_golden(mech), Oracle(mech)
    var, ierr, st, texit, hexit, samples, nout = RD.restated_single(mech, g, method)
    assert (ierr == 1).all() and (st[:, 2] == 1).all() and (st[:, 3] == 1).all() and (nout == 3).all() and (texit == 1.0e-3).all()
    for i, c in enumerate(RD.cells_of(g["var_in"].shape[0])):
        y0, fix, rc = g["var_in"][c], g["fix"][c], g["rconst"][c]
        f0, f1 = o.fun(y0, fix, rc), o.fun(var[i], fix, rc)
        for k, tk in enumerate(RD.SINGLE_TS):
            assert samples[i][k].tobytes() == RD.hermite(y0, f0, var[i], f1, 1.0e-3, (tk - 0.0) / 1.0e-3).tobytes(), (c, k)
        assert samples[i][2].tobytes() == var[i].tobytes()


# ---- (e)
@pytest.mark.parametrize("mech", MECHS)
def test_bounds_follow_the_restatements_own_movement(mech):
    """tests/ros_dense_bounds.py: no re-association changes IERR, a counter or nout on a test cell; each constant is within [10x, 100x] of the spread
    measured now, or is the floor."""
    spread, scaled, moved = db.measure_spread(mech, load_golden(mech))
    print("%s: sample spread %.3e by rel_diff, %.3e over the row maximum" % (mech, spread, scaled))
    assert not moved, "re-association changes IERR, the counters or nout: %s" % moved
    db.check(mech, spread, scaled)


# ---- (f)
def _P(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


def test_arguments_are_refused_before_a_device_is_touched():
    """Null ts / ysample / nout, ns out of range, a NaN time, a repeated time, a time at Tstart, a time beyond Tend, a change of direction, a bad ntol,
    an unknown mechanism and both user slots: each fails with its own text through the dense-output entries it applies to, with every data pointer NULL
    and no device initialised — never the 'no HIP device' or an unknown-symbol path."""
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    nvar = chem.DIMS["gas"][0]
    rpar, tol = np.zeros(20), np.full((1, nvar), 1.0e-3)
    ipar = np.array([0, 1, 0, 2] + [0] * 16, np.int32)
    vector = np.array([0, 0, 0, 2] + [0] * 16, np.int32)
    ys, nout = np.zeros(4), np.zeros(1, np.int32)      # never written: every call below is refused
    good = np.array([1.0, 2.0, 10.0])
    vp = lambda a: None if a is None else C.cast(_P(a), C.c_void_p)      # noqa: E731
    hp = lambda a: None if a is None else _P(a)      # noqa: E731

    def entries(mid, ts=good, ns=None, y=ys, n=nout, ntol=nvar, ip=ipar, t0=0.0, t1=10.0):
        ns = (0 if ts is None else len(ts)) if ns is None else ns
        head = (mid, 1, None, None, None, t0, t1)
        return {
            "dense_ex": lambda: L.mistra_chem_rosenbrock_dense_ex(*head, _P(tol), _P(tol), _P(rpar), _P(ip), None, None, None, None, ns, hp(ts), hp(y), hp(n)),
            "dense_device": lambda: L.mistra_chem_rosenbrock_dense_device(*head, _P(tol), _P(tol), _P(rpar), _P(ip), None, None, None, None, None, None, ns,
                                                                          hp(ts), vp(y), vp(n)),
            "dense_cells_ex": lambda: L.mistra_chem_rosenbrock_dense_cells_ex(*head, _P(tol), _P(tol), ntol, _P(rpar), _P(ip), None, None, None, None, ns,
                                                                              hp(ts), hp(y), hp(n)),
            "dense_cells_device": lambda: L.mistra_chem_rosenbrock_dense_cells_device(*head, vp(tol), vp(tol), ntol, _P(rpar), _P(ip), None, None, None,
                                                                                      None, None, None, ns, hp(ts), vp(y), vp(n)),
        }

    def refused(calls, text):
        assert len(calls) in (2, 4)
        for what, call in calls.items():
            assert call() != 0, (what, text)
            msg = L.mistra_chem_last_error().decode()
            assert text in msg and "no HIP device" not in msg, (what, text, msg)

    refused(entries(0, ts=None, ns=3), "dense output: null ts pointer (ts: [ns], a host array)")
    refused(entries(0, y=None), "dense output: null ysample pointer (ysample: [ns][ncell][NVAR])")
    refused(entries(0, n=None), "dense output: null nout pointer (nout: [ncell])")
    refused(entries(0, ns=0), "dense output: ns = 0: a call takes 1 .. MISTRA_DENSE_MAX_TIMES = 4096 sample times")
    refused(entries(0, ns=RD.MAX_TIMES + 1), "dense output: ns = 4097: a call takes 1 .. MISTRA_DENSE_MAX_TIMES = 4096 sample times")
    refused(entries(0, ts=np.array([1.0, np.nan, 3.0])), "dense output: ts[1] is not finite")
    refused(entries(0, ts=np.array([1.0, np.inf])), "dense output: ts[1] is not finite")
    refused(entries(0, ts=np.array([1.0, 2.0, 2.0])), "dense output: ts[2] repeats ts[1]: the sample times are strictly monotone")
    refused(entries(0, ts=np.array([0.0, 1.0])), "dense output: ts[0] does not lie behind Tstart in the call's direction")
    refused(entries(0, ts=np.array([1.0, 10.5])), "dense output: ts[1] lies beyond Tend")
    refused(entries(0, ts=np.array([1.0, 3.0, 2.0])), "dense output: the sample times change direction at ts[2]")
    # a backward call: its direction is the kernel's, Tend >= Tstart ? 1 : -1
    refused(entries(0, ts=np.array([1.0, 2.0]), t0=10.0, t1=0.0), "dense output: the sample times change direction at ts[1]")
    refused(entries(0, ts=np.array([10.0, 5.0]), t0=10.0, t1=0.0), "dense output: ts[0] does not lie behind Tstart")
    refused(entries(0, ts=np.array([5.0, -1.0]), t0=10.0, t1=0.0), "dense output: ts[1] lies beyond Tend")
    refused(entries(9), "unknown mechanism id")
    refused(entries(-1), "unknown mechanism id")
    cells = lambda **kw: {k: v for k, v in entries(0, **kw).items() if "cells" in k}      # noqa: E731
    refused(cells(ntol=2), "ntol = 2: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    refused(cells(ntol=0), "ntol = 0: a tolerance row holds 1 or NVAR = %d entries" % nvar)
    refused(cells(ntol=1, ip=vector), "vector tolerances (ipar[1] = 0) need rows of NVAR = %d entries, ntol = 1" % nvar)
    # both user slots: the slot's existing text, whatever else the call carries (ids 3 and 4 of a library without slots are no mechanisms)
    names = chem.user_mechs()
    for i in range(2):
        if i < len(names):
            refused(entries(3 + i), "user mechanism slot %d (%s) has no dense-output entries: a user slot integrates" % (i, names[i]))
            refused(entries(3 + i, ts=None), "and nothing else")
        else:
            refused(entries(3 + i), "unknown mechanism id")
    assert len(names) == 2      # the library this repository builds has both
    # the Python surface passes the refusals on, without init()
    g = load_golden("gas")
    V, F, K = g["var_in"][:2], g["fix"][:2], g["rconst"][:2]
    with pytest.raises(chem.MistraChemError, match="repeats"):
        chem.rosenbrock_dense("gas", V, F, K, 0.0, 10.0, [1.0, 1.0])
    with pytest.raises(chem.MistraChemError, match="ntol = 5"):
        chem.rosenbrock_dense_cells("gas", V, F, K, 0.0, 10.0, [1.0], None, None, np.ones((2, 5)), np.ones((2, 5)))
    with pytest.raises(chem.MistraChemError, match="has no dense-output entries"):
        chem.rosenbrock_dense(3, np.zeros((1, chem.DIMS[names[0]][0])), np.zeros((1, chem.DIMS[names[0]][1])), np.zeros((1, chem.DIMS[names[0]][2])), 0.0, 10.0,
                              [1.0])


# ---- (g)
def test_dense_needs_a_device():
    """Without a GPU a well-formed call raises 'no HIP device' (there is no CPU path), through both wrappers."""
    import torch
    from mistra_amd import chem
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = load_golden("gas")
    V, F, K = g["var_in"][:1], g["fix"][:1], g["rconst"][:1]
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_dense("gas", V, F, K, 0.0, 10.0, RD.LINEAR8)
    with pytest.raises(chem.MistraChemError, match="no HIP device"):
        chem.rosenbrock_dense_cells("gas", V, F, K, 0.0, 10.0, RD.END, None, None, np.full((1, 1), 1.0e-25), np.full((1, 1), 1.0e-3))


# ---- (h)
def test_tool_on_the_cpu():
    """tools/step_control.py gas --dense 4 --cpu on two golden cells: runs without a GPU and prints the table of --series with the run's side from one
    call.  Nothing is asserted on the figures but that they are numbers."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    path = os.path.join(REPO, "tests", "golden", "integrate_gas.npz")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "step_control.py"), "gas", "--golden", path, "--cells", "0:2", "--dense", "4", "--cpu"],
                       check=True, capture_output=True, text=True, timeout=300)
    assert "CPU restatement" in r.stdout and "dense output: the run's side sampled inside ONE call" in r.stdout, r.stdout
    table = r.stdout.split("dense output:")[1].split("\n")[2:6]      # behind the title and the header: one row per sub-time
    rows = [[float(x) for x in l.split()] for l in table]
    assert [row[0] for row in rows] == [2.5, 5.0, 7.5, 10.0] and all(len(row) == 4 and np.isfinite(row).all() and row[3] == 2 for row in rows), r.stdout


# ---- (i)
def test_dense_kernel_lives_in_the_series_unit_and_is_checked_like_every_unit():
    """no unit of its own: the unit list is what it was; the gas Ros3 series unit compiled here passes the register-ring and hazard reports the build
    runs on every unit, and holds exactly two kernels, the VARIANT 5 and the VARIANT 7 instantiation"""
    from mistra_amd import build as B
    assert sorted(B.VARIANT_METHODS) == [3, 4, 5, 6] and len(B.VARIANT_UNITS) == 45
    with pytest.raises(ValueError, match="no kernel unit"):
        B.unit_build(B.Unit(7, 0, 2))
    rep = B.ring_register_report(unit=B.Unit(5, 0, 2))
    assert B.isa_hazard_report(rep["__isa_text__"]) == []
    kernels = sorted(k for k in rep if "ros3_integrate_kernel" in k)
    assert kernels == ["_ZN6mistra21ros3_integrate_kernelINS_9GasTraitsELi64ELi5ELi2EEEvNS_10KernelArgsE",
                       "_ZN6mistra21ros3_integrate_kernelINS_9GasTraitsELi64ELi7ELi2EEEvNS_10KernelArgsE"], kernels
