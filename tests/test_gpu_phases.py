"""Phase-level parity on the GPU (-m gpu): the kernel's first-step dump variant (mistra_chem_debug_first_step) hands out
Fcn0, Ghimj as prepared, Ghimj as factorised, the pivots' reciprocals, K(1..3) and the error norm of the first attempt of
the first step, and each is compared with what it should be — so that a difference at the end can be pinned on a phase:

  Fun_x, ros_PrepareMatrix_x      bit for bit against the oracle (same operation order, no contraction)
  KppDecomp_x                     against the TEST-ONLY emulator of the kernel's own programs (tests/emu), which repeats the
                                  kernel's arithmetic operation by operation (LDS VM rounds, scaling pass, the dense tail
                                  block's MFMA steps as fused multiply-add chains), and against the oracle's factors to the
                                  bound tests/test_schedule.py holds the emulator to
  KppSolve_x (K1, K2, K3)         against the oracle's solve with the oracle's factors, stage by stage on the GPU's own
                                  previous-stage vectors
  ros_ErrorNorm_x                 against the oracle's formula on the GPU's K vectors

Plus the error paths no captured call reaches: a crafted zero pivot (Nsng = 1, H halved, integration goes on), six in a
row (IERR = -8), and backward integration (TOUT < TIN, Direction = -1).

test_phases_of_the_first_step sees H = 1e-3 only, where Ghimj = 2294*I - J is the friendliest matrix the integrator ever factorises;
test_phases_at_running_step_sizes repeats the phases at the step sizes the integrator runs at, against the re-association of the oracle
that the kernel's factorisation IS (oracle.set_variant(4)), and ties the dump instantiation of the kernel to the one that ships;
test_rejected_steps_long_and_backward_horizons runs the product kernel through rejected steps after accepted ones, hour-long and
backward horizons and an IERR = -7 from a finite state.  Their bounds come from the oracle alone: tests/parity_bounds.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import MECHS, REPO, rel_diff
from parity_bounds import REJECT_CASES

pytestmark = pytest.mark.gpu
GAMMA = (0.43586652150845899941601945119356, 0.24291996454816804366592249683314, 0.21851380027664058511513169485832e+01)
C21, C31, C32 = -0.10156171083877702091975600115545e+01, 0.40759956452537699824805835358067e+01, 0.92076794298330791242156818474003e+01
E = (0.5, -0.29079558716805469821718236208017e+01, 0.22354069897811569627360909276199e+00)
dp = C.POINTER(C.c_double)


def P(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    c.lib().mistra_chem_debug_first_step.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.c_double, C.c_double, dp]
    return c


@pytest.fixture(scope="module")
def emu():
    d = os.path.join(REPO, "tests", "emu")
    subprocess.run(["make", "-s", "-C", d], check=True)
    lib = C.CDLL(os.path.join(d, "libschedule_emu.so"))
    lib.emu_create.restype = C.c_void_p
    lib.emu_create.argtypes = [C.c_char_p, C.c_int]
    lib.emu_lu.argtypes = [C.c_void_p, dp, dp, dp]
    lib.emu_tail_h.argtypes = [C.c_void_p]
    lib.emu_solve_backward.argtypes = [C.c_void_p, dp, dp]
    lib.emu_solve_kernel_form.argtypes = [C.c_void_p, dp, dp]
    return lib


def first_step(chem, mech, var, fix, rconst, tin=0.0, tout=10.0):
    from mistra_amd.chem import DIMS, MECH_IDS
    nvar, _, _, nnz = DIMS[mech]
    n = var.shape[0]
    dump = np.zeros((n, 5 * nvar + 2 * nnz + 2))
    v, f, r = (np.ascontiguousarray(x, np.float64) for x in (var, fix, rconst))
    assert chem.lib().mistra_chem_debug_first_step(MECH_IDS[mech], n, P(v), P(f), P(r), tin, tout, P(dump)) == 0, chem.lib().mistra_chem_last_error()
    o = 0
    out = {}
    for name, ln in (("fcn0", nvar), ("ghimj", nnz), ("lu", nnz), ("r", nvar), ("k1", nvar), ("k2", nvar), ("k3", nvar), ("err", 1), ("h", 1)):
        out[name] = dump[:, o:o + ln]
        o += ln
    return out


@pytest.mark.parametrize("mech", MECHS)
def test_phases_of_the_first_step(chem, emu, mech, golden, oracles):
    """The first attempt of the first step, H = 1e-3.  The two bounds against the PINNED oracle below (factors <= 1e-7 of the row maximum, K vectors
    <= 1e-9) hold because of that H and are deliberately not extended to larger ones: on the CPU (emulator against oracle) the factors differ by 3e-9
    at H = 1e-3 and by 2.6e-5 at H = 10 on aer (tot: 3e-12 and 4e-9), K1 by 4e-10 and 2.6e-6 — and the reference itself moves by up to 1.7e-5 there
    when its multipliers are formed with the reciprocal (variant 4).  test_phases_at_running_step_sizes measures against that variant instead."""
    from mistra_amd.mechtab import load
    o, g, t = oracles[mech], golden[mech], load(mech)
    nt = {"gas": 64, "aer": 256, "tot": 512}[mech]      # the workgroup sizes ros3_kernel.hpp instantiates (gas: one wavefront per cell)
    h_emu = emu.emu_create(os.path.join(REPO, "mistra_amd", "mech", mech + ".mech").encode(), nt)
    cells = [0, 7, len(g["var_in"]) - 1]
    V, F, K = g["var_in"][cells], g["fix"][cells], g["rconst"][cells]
    d = first_step(chem, mech, V, F, K)
    worst = dict(lu_vs_emu=0.0, lu_vs_oracle=0.0, k=0.0, err=0.0)
    for i in range(len(cells)):
        v, f, k = (np.ascontiguousarray(x[i]) for x in (V, F, K))
        H = d["h"][i, 0]
        assert H == 1.0e-3                                                    # Hstart (gas.f:743), first attempt
        # ---- Fun_x
        fcn0 = o.fun(v, f, k)
        assert np.array_equal(d["fcn0"][i], fcn0), "Fun_x differs from the oracle"
        # ---- ros_PrepareMatrix_x
        ghinv = 1.0 / (H * GAMMA[0])
        G = -o.jac_sp(v, f, k)
        G[t.diag] += ghinv
        assert np.array_equal(d["ghimj"][i], G), "Ghimj = 1/(H*gamma) - Jac0 differs from the oracle"
        # ---- KppDecomp_x: the kernel's programs, repeated on the host operation by operation
        lu_emu, r_emu, x = G.copy(), np.empty(o.nvar), fcn0.copy()
        assert emu.emu_lu(h_emu, P(lu_emu), P(r_emu), P(x)) == 0
        rowmax = np.array([np.abs(lu_emu[t.crow[r]:t.crow[r + 1]]).max() for r in range(o.nvar)])
        scale = np.repeat(rowmax, np.diff(t.crow))
        worst["lu_vs_emu"] = max(worst["lu_vs_emu"], (np.abs(d["lu"][i] - lu_emu) / scale).max())
        assert np.array_equal(d["lu"][i], lu_emu), "factors differ from the emulated kernel programs (max %.1e of the row maximum)" % (np.abs(d["lu"][i] - lu_emu) / scale).max()
        assert np.array_equal(d["r"][i], r_emu), "pivot reciprocals differ from the emulated kernel programs"
        # ... and KppDecomp_x itself: the reference's factors, un-scaling the rows the kernel keeps row-scaled
        lu_ref, ier = o.decomp(G)
        assert ier == 0
        lu_un = d["lu"][i].copy()
        for r in range(emu.emu_tail_h(h_emu), o.nvar):
            lu_un[t.diag[r] + 1:t.crow[r + 1]] *= lu_un[t.diag[r]]
        rowmax_ref = np.repeat(np.array([np.abs(lu_ref[t.crow[r]:t.crow[r + 1]]).max() for r in range(o.nvar)]), np.diff(t.crow))
        worst["lu_vs_oracle"] = max(worst["lu_vs_oracle"], (np.abs(lu_un - lu_ref) / rowmax_ref).max())
        # (multipliers formed as W*R instead of W/U(j,j), carried through the elimination: 1e-16 per operation times the
        #  growth of the factorisation of this particular matrix — 3e-9 on the worst of the captured aer cells)
        assert (np.abs(lu_un - lu_ref) / rowmax_ref).max() <= 1e-7
        # ---- KppSolve_x, stage by stage on the GPU's own vectors (gas.f:1236-1262)
        k1, k2, k3 = d["k1"][i], d["k2"][i], d["k3"][i]
        want1 = o.solve(lu_ref, fcn0)
        fcn = o.fun(v + k1, f, k)
        want2 = o.solve(lu_ref, fcn + (C21 / H) * k1)
        want3 = o.solve(lu_ref, (fcn + (C31 / H) * k1) + (C32 / H) * k2)
        for got, want in ((k1, want1), (k2, want2), (k3, want3)):
            e = np.abs(got - want).max() / np.abs(want).max()
            worst["k"] = max(worst["k"], e)
            assert e <= 1e-9
        # ... and bit for bit against the emulated solve programs (head sweeps, tail chain — for tot with the cross-lane chain over
        # the dense block) run on the GPU's own factors and right-hand sides: same operations, same order, same fused multiply-adds
        lu_gpu = np.ascontiguousarray(d["lu"][i])
        e1 = x.copy()                                   # (emu_lu above carried the stage-1 right-hand side through the elimination)
        assert emu.emu_solve_backward(h_emu, P(lu_gpu), P(e1)) == 0
        e2 = np.ascontiguousarray((fcn + (C21 / H) * k1) + (H * GAMMA[1]) * 0.0)
        assert emu.emu_solve_kernel_form(h_emu, P(lu_gpu), P(e2)) == 0
        e3 = np.ascontiguousarray(((fcn + (C31 / H) * k1) + (C32 / H) * k2) + (H * GAMMA[2]) * 0.0)
        assert emu.emu_solve_kernel_form(h_emu, P(lu_gpu), P(e3)) == 0
        assert np.array_equal(k1, e1), "K1 differs from the emulated solve programs"      # (the forward-swept stage-1 vector is the emulator's: its factors are the GPU's, bit for bit — asserted above)
        assert np.array_equal(k2, e2), "K2 differs from the emulated solve programs"
        assert np.array_equal(k3, e3), "K3 differs from the emulated solve programs"
        worst["k_bitwise"] = worst.get("k_bitwise", 0) + 1
        # ---- ros_ErrorNorm_x (gas.f:1341) on the GPU's K vectors
        ynew = ((v + k1) + 0.61697947043828245592553615689730e+01 * k2) + -0.42772256543218573326238373806514e+00 * k3
        yerr = ((0.0 + E[0] * k1) + E[1] * k2) + E[2] * k3
        sc = 1.0e-25 + 1.0e-3 * np.maximum(np.abs(v), np.abs(ynew))
        err = np.sqrt(((yerr / sc) ** 2).sum() / o.nvar)
        worst["err"] = max(worst["err"], abs(d["err"][i, 0] - err) / err)
        assert abs(d["err"][i, 0] - err) <= 1e-12 * err
    print("%s phases: Fun and Ghimj bit-exact; LU vs emulated kernel %.1e, vs reference factors %.1e (of row max); "
          "K vectors %.1e vs the oracle's solve, bit-identical to the emulated solve programs in %d cells; error norm %.1e"
          % (mech, worst["lu_vs_emu"], worst["lu_vs_oracle"], worst["k"], worst.get("k_bitwise", 0), worst["err"]))


@pytest.mark.parametrize("state", ["var_in", "var_out"])
@pytest.mark.parametrize("mech", MECHS)
def test_phases_at_running_step_sizes(chem, emu, mech, state, golden, oracles):
    """One launch of 12 cells per mechanism and state: cells {0, 7, last} of the main captured set, as captured (var_in) or after the 10 s call (the
    golden var_out, bit-exact to the oracle), each at the first step sizes {1e-3, 0.1, Hexit, 10} through the dump entry's hstart (Hexit: the last
    step size of the cell's captured call, what the Hstart-reuse path would feed back; 2.7-9.5 s aer, 3-3.7 s tot, 10 s gas), TOUT = 10.

    Per cell: the dumped H is the one asked for; Fun_x and Ghimj bit for bit against the oracle; factors, pivot reciprocals and K1..K3 bit for bit
    against the emulated kernel programs; the error norm to 1e-12 of the formula; and, facing the oracle,
      factors   against KppDecomp_x with its multipliers formed as W*(1/U(j,j)) (oracle.set_variant(4), the one way the kernel's factorisation
                departs from the reference's): head rows bit for bit, tail rows of gas and aer within 4 units of round-off of each entry (one
                rounding each for R = 1/U, W*R, U*R and the un-scaling product), tail rows of tot within parity_bounds.TOT_TAIL_BOUND = 7.4e-13 of
                the row maximum = 10x what the emulator shows on these very matrices on the CPU (7.4e-14; gas and aer 2.2e-16 = 2.2 and 2.3 units of
                round-off); yardstick: the oracle's variant 4 against its variant 6 moves those entries by 9.5e-10
      K1..K3    stage by stage on the GPU's own previous-stage vectors against the oracle's solve that multiplies by the pivot's reciprocal, on the
                variant-4 factors: <= 10x the spread of the oracle's eight solve variants on the same factors and right-hand sides, per step size
                (parity_bounds.check_k_vectors says why per step size).  CPU, emulator, error / spread at H = 1e-3, 0.1, Hexit, 10:
                  gas var_in  2.1e-17/2.0e-16 3.6e-17/2.1e-16 4.1e-17/1.4e-16 4.1e-17/1.4e-16   var_out 5.0e-17/1.7e-16 2.4e-17/1.9e-16 3.1e-17/1.7e-16 3.1e-17/1.7e-16
                  aer var_in  4.2e-11/1.7e-10 3.4e-10/1.5e-8  2.3e-9/1.1e-6   1.7e-9/3.3e-7     var_out 3.1e-16/2.0e-13 1.7e-15/4.7e-13 2.8e-12/6.9e-13 3.3e-12/6.5e-12
                  tot var_in  3.9e-12/4.1e-12 1.8e-11/5.8e-11 1.1e-9/4.0e-10  2.8e-9/2.0e-9     var_out 3.7e-16/2.3e-13 7.0e-16/2.8e-13 6.7e-13/3.4e-13 1.2e-11/5.7e-12
                (the GPU's K vectors are the emulator's bit for bit, so the test prints the same figures on an MI355X, and 7.4e-14 for tot's tail rows).

    Then the dump instantiation ros3_integrate_kernel<.., 2> against the product instantiation <.., 0>: VAR, IERR and /Statistics/ of the integration the
    dump kernel carried to its end are bit-identical to the product kernel's on the same inputs — with the same hstart through the device entry, and
    with none through the host entry."""
    import torch
    import parity_bounds as pb
    from mistra_amd.mechtab import load
    o, g, t = oracles[mech], golden[mech], load(mech)
    nt = {"gas": 64, "aer": 256, "tot": 512}[mech]
    h_emu = emu.emu_create(os.path.join(REPO, "mistra_amd", "mech", mech + ".mech").encode(), nt)
    tail_h = emu.emu_tail_h(h_emu)
    V, F, K, Hask = pb.phase_cases(g, o, state)
    assert len(Hask) >= 12
    d = chem.debug_first_step(mech, V, F, K, 0.0, 10.0, hstart=Hask)
    found, worst_ulps, worst_row, worst_err = [], 0.0, 0.0, 0.0
    for i in range(len(Hask)):
        v, f, k = V[i], F[i], K[i]
        H = d.h[i, 0]
        assert H == Hask[i], "cell %d: the dumped attempt ran at H = %r, asked for %r" % (i, H, Hask[i])
        fcn0 = o.fun(v, f, k)
        assert np.array_equal(d.fcn0[i], fcn0), "Fun_x differs from the oracle"
        G = -o.jac_sp(v, f, k)
        G[t.diag] += 1.0 / (H * GAMMA[0])
        assert np.array_equal(d.ghimj[i], G), "Ghimj = 1/(H*gamma) - Jac0 differs from the oracle at H = %g" % H
        lu_emu, r_emu, x = G.copy(), np.empty(o.nvar), fcn0.copy()
        assert emu.emu_lu(h_emu, P(lu_emu), P(r_emu), P(x)) == 0
        assert np.array_equal(d.lu[i], lu_emu), "factors differ from the emulated kernel programs at H = %g" % H
        assert np.array_equal(d.r[i], r_emu), "pivot reciprocals differ from the emulated kernel programs at H = %g" % H
        lu_v4 = pb.variant4_factors(o, G)
        ulps, of_row = pb.check_lu_against_variant4(mech, t, tail_h, d.lu[i], lu_v4)
        worst_ulps, worst_row = max(worst_ulps, ulps), max(worst_row, of_row)
        k1, k2, k3 = d.k1[i], d.k2[i], d.k3[i]
        fcn = o.fun(v + k1, f, k)
        r2 = np.ascontiguousarray(fcn + (C21 / H) * k1)
        r3 = np.ascontiguousarray((fcn + (C31 / H) * k1) + (C32 / H) * k2)
        for got, rhs in ((k1, fcn0), (k2, r2), (k3, r3)):
            want, spread = pb.solve_reference_and_spread(o, lu_v4, rhs)
            found.append((i % len(pb.PHASE_H), np.abs(got - want).max() / np.abs(want).max(), spread))
        lu_gpu = np.ascontiguousarray(d.lu[i])
        e1 = x.copy()
        assert emu.emu_solve_backward(h_emu, P(lu_gpu), P(e1)) == 0
        e2 = np.ascontiguousarray(r2 + (H * GAMMA[1]) * 0.0)
        assert emu.emu_solve_kernel_form(h_emu, P(lu_gpu), P(e2)) == 0
        e3 = np.ascontiguousarray(r3 + (H * GAMMA[2]) * 0.0)
        assert emu.emu_solve_kernel_form(h_emu, P(lu_gpu), P(e3)) == 0
        assert np.array_equal(k1, e1) and np.array_equal(k2, e2) and np.array_equal(k3, e3), "K vectors differ from the emulated solve programs at H = %g" % H
        ynew = ((v + k1) + 0.61697947043828245592553615689730e+01 * k2) + -0.42772256543218573326238373806514e+00 * k3
        yerr = ((0.0 + E[0] * k1) + E[1] * k2) + E[2] * k3
        sc = 1.0e-25 + 1.0e-3 * np.maximum(np.abs(v), np.abs(ynew))
        err = np.sqrt(((yerr / sc) ** 2).sum() / o.nvar)
        worst_err = max(worst_err, abs(d.err[i, 0] - err) / err)
        assert abs(d.err[i, 0] - err) <= 1e-12 * err
    print("%s %s: LU tail rows vs variant 4 %.2f units of round-off of the entry, %.2e of the row maximum; error norm %.1e" % (mech, state, worst_ulps, worst_row, worst_err))
    per_h = pb.check_k_vectors(mech, found)
    print("%s %s: K vectors, error / spread of the oracle's solve variants per H: %s" % (mech, state, "  ".join("%.1e / %.1e" % per_h[i] for i in sorted(per_h))))
    # ---- the dump instantiation against the product instantiation
    dev = torch.device("cuda", 0)
    n = len(Hask)
    tv, tf, tk, th = (torch.tensor(a, device=dev) for a in (V, F, K, Hask))
    out = torch.empty_like(tv)
    ierr = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty((n, 8), dtype=torch.int32, device=dev)
    chem.integrate_into(mech, tv, tf, tk, out, ierr, stats, 0.0, 10.0, hstart=th)
    torch.cuda.synchronize()
    assert np.all(d.ierr == 1)
    assert np.array_equal(d.ierr, ierr.cpu().numpy()) and np.array_equal(d.stats, stats.cpu().numpy()), "dump kernel and product kernel count differently"
    assert np.array_equal(d.var, out.cpu().numpy()), "dump kernel and product kernel integrate to different states (max rel diff %.1e)" % rel_diff(d.var, out.cpu().numpy()).max()
    want, want_ierr, want_st = o.integrate_batch(V, F, K, 0.0, 10.0, hstart=Hask)      # ... and both count as the oracle started at the same H
    assert np.array_equal(d.stats, want_st) and np.array_equal(d.ierr, want_ierr)
    d0 = chem.debug_first_step(mech, V, F, K, 0.0, 10.0)
    res = chem.integrate(mech, V, F, K, 0.0, 10.0)
    assert np.all(d0.h == 1.0e-3)
    assert np.array_equal(d0.ierr, res.ierr) and np.array_equal(d0.stats, res.stats) and np.array_equal(d0.var, res.var), "dump kernel and product kernel differ without hstart"


@pytest.mark.parametrize("name", list(REJECT_CASES))
def test_rejected_steps_long_and_backward_horizons(chem, name, oracles):
    """No captured call and no synthetic batch rejects a step after it has accepted one (Nrej = 0 everywhere), so `if (nacc >= 1) nrej += 1`, a reject
    with Y advanced and T > Tstart, and RejectLastH capping the next accepted step never ran under a test.  These inputs do (tests/parity_bounds.py:
    REJECT_CASES; oracle on the CPU):
      gas_day cells 0..7, 0.5 -> 0     IERR 1, Nrej 2 6 1 8 2 5 0 3, Nstp <= 28      backward
      gas cell 2, 5 -> 0               IERR 1, Nrej 6, Nstp 22                       backward
      aer cells 3 6 7, 0 -> 3600       IERR 1, Nrej 1 2 2, Nstp <= 246               an hour
      tot_day cells 1 4 7, 0 -> 3600   IERR 1, Nrej 1 1 1, Nstp <= 249               an hour
      tot cells 0 1, 0.02 -> 0         IERR -7 from a FINITE state, Nrej 18 31, Nstp <= 441
    The product kernel against the oracle: IERR and /Statistics/ identical; exit time, last accepted step size and VAR within 10x
    the oracle's own spread under re-association ON THAT INPUT (measured on the CPU by tests/test_oracle.py::test_reject_cases_are_stable_under_reassociation,
    which also holds that no re-association changes the bookkeeping of these inputs): spread 3.2e-16, 2.2e-16, 8.3e-5, 1.7e-5, 8.8e-14 in the order
    above, bounds parity_bounds.REJECT_RTOL (exit time and step size: 1.3e-14, 2.3e-15, 1.1e-4, 1.2e-5, 7.4e-14, bounds REJECT_TH_RTOL).  The test prints what the kernel shows; on an MI355X: VAR 4.8e-16, 2.4e-16, 9.5e-5, 1.1e-5, 1.1e-13, last step size 2.5e-14, 2.1e-15,
    6.8e-5, 2.6e-6, 7.1e-14, exit times identical."""
    import parity_bounds as pb
    _, _, cells, _, _, want_ierr, want_nrej, max_nstp = pb.REJECT_CASES[name]
    mech, V, F, K, tin, tout = pb.reject_case_inputs(name)
    o = oracles[mech]
    want = [o.integrate(V[i], F[i], K[i], tin, tout) for i in range(len(V))]
    w_var, w_ierr = np.array([w[0] for w in want]), np.array([w[1] for w in want], np.int32)
    w_st, w_te, w_he = np.array([w[2] for w in want]), np.array([w[3] for w in want]), np.array([w[4] for w in want])
    # the premise, so that the test cannot quietly stop covering the path
    assert np.all(w_ierr == want_ierr) and np.isfinite(V).all() and np.isfinite(w_var).all()
    assert w_st[:, 4].tolist() == list(want_nrej) and np.all(w_st[:, 3] >= 1) and w_st[:, 2].max() <= max_nstp
    assert sum(x > 0 for x in w_st[:, 4]) >= len(cells) - 1
    res, th = chem.integrate_ex(mech, V, F, K, tin, tout)
    d = rel_diff(res.var, w_var)
    print("%s: kernel vs oracle max rel diff %.3e (bound %.1e), Nrej %s, Nstp %s, IERR %s" % (name, d.max(), pb.REJECT_RTOL[name], res.stats[:, 4].tolist(), res.stats[:, 2].tolist(), res.ierr.tolist()))
    assert np.array_equal(res.ierr, w_ierr), (res.ierr, w_ierr)
    assert np.array_equal(res.stats, w_st), (res.stats, w_st)
    # exit time (on the scale of the interval's ends) and last step size: 10x what the oracle's own variants move them by (REJECT_TH_RTOL)
    d_te = np.abs(th[:, 0] - w_te).max() / max(abs(tin), abs(tout))
    d_he = (np.abs(th[:, 1] - w_he) / np.abs(w_he)).max()
    print("%s: exit time %.3e of the interval, last step size %.3e from the oracle's" % (name, d_te, d_he))
    assert d_te <= pb.REJECT_TH_RTOL[name] and d_he <= pb.REJECT_TH_RTOL[name]
    assert np.isfinite(res.var).all()
    assert d.max() <= pb.REJECT_RTOL[name]


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
def test_zero_pivot_paths(chem, mech, golden, oracles):
    """ros_PrepareMatrix_x's singular branch (gas.f:1439-1467): a first-order loss with the NEGATIVE rate constant
    k = -1/(H*gamma) puts an exact zero on the diagonal of Ghimj at step size H.  One such reaction: one failed
    decomposition, H halved, the step goes on (Nsng = 1, Ndec = Nstp + 1).  Six of them, tuned to H, H/2 .. H/32: six
    failures in a row, IERR = -8.  Kernel against oracle: IERR, /Statistics/, state."""
    from mistra_amd.mechtab import load
    o, g, t = oracles[mech], golden[mech], load(mech)
    losses, seen = [], set()
    for r, s in _first_order_losses(t):
        if s not in seen:
            seen.add(s)
            losses.append((r, s))
    assert len(losses) >= 6
    V, F = g["var_in"][:1].copy(), g["fix"][:1].copy()
    tin, tout = 0.0, 1.5e-3
    for nzero, want_ierr in ((1, 1), (6, -8)):
        K = np.zeros((1, t.nreact))
        for i in range(nzero):
            K[0, losses[i][0]] = -1.0 / ((1.0e-3 / 2 ** i) * GAMMA[0])
        # the premise: the oracle's own Jacobian has the exact zero on the diagonal at the first attempt
        G = -o.jac_sp(V[0], F[0], K[0])
        G[t.diag] += 1.0 / (1.0e-3 * GAMMA[0])
        assert G[t.diag[losses[0][1]]] == 0.0
        want, ierr, st = o.integrate_batch(V, F, K, tin, tout)
        res = chem.integrate(mech, V, F, K, tin, tout)
        assert int(ierr[0]) == want_ierr and int(res.ierr[0]) == want_ierr
        assert np.array_equal(res.stats, st), (res.stats, st)
        assert int(st[0, 7]) == (1 if nzero == 1 else 6)                       # Nsng
        assert np.allclose(res.var, want, rtol=1e-9, atol=1e-300)
        # the row KppDecomp_x reports (IER = first row with an exactly zero diagonal, gas.f:6157) and ros_PrepareMatrix_x prints
        # (gas.f:1456): at H/2**i the loss of species losses[i] cancels 1/(H*gamma)
        rows = chem.singular_rows(mech, 0)
        assert list(rows[:nzero]) == [losses[i][1] + 1 for i in range(nzero)], rows
        _, ier = o.decomp(G)
        assert ier == rows[0]
    print(mech, "zero-pivot paths: Nsng = 1 continues, six in a row end with IERR = -8; statistics identical to the oracle's")


def test_backward_integration(chem, golden, oracles):
    """TOUT < TIN: Direction = -1 (gas.f:1188-1192), every H-dependent factor changes sign."""
    g, o = golden["gas"], oracles["gas"]
    V, F, K = g["var_in"][:3], g["fix"][:3], g["rconst"][:3]
    want, ierr, st = o.integrate_batch(V, F, K, 2.0e-3, 0.0)
    res = chem.integrate("gas", V, F, K, 2.0e-3, 0.0)
    assert np.array_equal(res.ierr, ierr) and np.array_equal(res.stats, st)
    assert np.allclose(res.var, want, rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("mech", MECHS)
def test_too_many_steps_exit(chem, mech, golden, oracles):
    """IERR = -6, "No of steps exceeds maximum bound" (gas.f:1199-1202): the bound Max_no_steps = 100000 that INTEGRATE_x leaves in place
    is out of a test's reach, so kernel and oracle both get 5 through their test hooks (mistra_chem_debug_set_max_steps /
    kpp_set_max_steps; the oracle's exit is pinned against the compiled reference's Rosenbrock_x called with IPAR(3) = 5,
    tests/test_oracle.py).  Code, /Statistics/, exit time, last step and the state reached, cells that finish below the bound among them."""
    from oracle import oracle as om
    g, o = golden[mech], oracles[mech]
    n = min(12, g["var_in"].shape[0])
    V, F, K = g["var_in"][:n], g["fix"][:n], g["rconst"][:n]
    touts = (10.0, 1.0e-6)      # (the second horizon is short enough for every cell to finish below the bound: the ordinary exit under the same hook)
    try:
        om.set_max_steps(5)
        chem.debug_set_max_steps(5)
        seen = set()
        for tout in touts:
            want, ierr, st = o.integrate_batch(V, F, K, 0.0, tout)
            res = chem.integrate(mech, V, F, K, 0.0, tout)
            assert np.array_equal(res.ierr, ierr), (res.ierr, ierr)
            assert np.array_equal(res.stats, st)
            assert rel_diff(res.var, want).max() <= 2e-5
            seen |= set(int(x) for x in ierr)
        assert -6 in seen and (mech == "tot" or 1 in seen), seen      # (the cloudy tot cells reject their way past the bound on any horizon)
    finally:
        om.set_max_steps(0)
        chem.debug_set_max_steps(0)
    res = chem.integrate(mech, V[:2], F[:2], K[:2], 0.0, 10.0)
    assert np.all(res.ierr == 1) and np.array_equal(res.stats[:, 2], g["stats"][:2, 2])
