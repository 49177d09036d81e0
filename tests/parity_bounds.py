"""Bounds of the parity tests that are MEASURED ON THE REFERENCE SIDE, the inputs they were measured on, and the comparisons both the CPU tests
(tests/test_oracle.py, tests/test_schedule.py) and the GPU tests (tests/test_gpu_parity.py, tests/test_gpu_phases.py) make with them.  Nothing
here looks at the kernel: every figure is the oracle's own movement under legal re-association (oracle.set_variant), 10x of which is the bound,
or follows from the rounding of the operations involved.  tests/test_oracle.py re-measures every figure and holds every constant to
[10x, 100x] of it (check_constant), so that a constant can neither go stale upwards nor downwards."""
import numpy as np

VARIANTS = (1, 2, 3, 4, 5, 7)      # the re-associations test_reference_sensitivity has always run (oracle.set_variant)
U = 2.0 ** -53                     # unit round-off


def check_constant(name, const, spread, floor=None, cap=None):
    """const is at least 10x and at most 100x the spread measured now — or is the stated floor, where 10x the spread lies below it, or the stated
    cap, where 10x the spread lies above it"""
    if floor is not None and 10.0 * spread <= floor:
        assert const == floor, "%s: 10x the measured spread %.3e is below the floor %.1e, the constant must be the floor (is %.3e)" % (name, spread, floor, const)
        return
    if cap is not None and 10.0 * spread >= cap:
        assert const == cap, "%s: 10x the measured spread %.3e is above the cap %.1e, the constant must be the cap (is %.3e)" % (name, spread, cap, const)
        return
    assert 10.0 * spread <= const <= 100.0 * spread, "%s = %.3e is not within [10x, 100x] of the measured spread %.3e" % (name, const, spread)


# ---- E. end-to-end parity over a 10 s call, per mechanism (tests/test_gpu_parity.py: check).  Spread: the worst rel_diff (conftest) between the pinned
# oracle and its variants over the captured sets of the mechanism (main + EXTRA_SETS), measured by
# tests/test_oracle.py::test_reference_sensitivity_bounds_the_parity_tolerance.  Bound = min(PARITY_CAP, max(10 x spread, PARITY_FLOOR)).
#   measured (CPU):  gas  main 1.6e-16  day 1.3e-16  base1 4.1e-16
#                    aer  main 1.86e-6  day 1.88e-6  base1 7.25e-6  buys13 1.2e-8
#                    tot  main 2.46e-7  day 3.41e-7
#   (measured once, too slow for the suite: the seeded synthetic batches of test_synthetic_batch_against_oracle move by gas 1.2e-15, aer 2.4e-6,
#    tot 4.2e-7 — each bound below is at least 8x that as well)
PARITY_FLOOR = 1e-13               # gas: 10x the spread would be 4e-15; 1e-13 is the project's own floor for that mechanism
PARITY_CAP = 2e-5                  # the bound every mechanism had before: this module only tightens.  aer's cloud-free base1 set moves by 7.3e-6,
#                                    10x of which is above it, so aer keeps 2e-5
PARITY_RTOL = {"gas": PARITY_FLOOR, "aer": PARITY_CAP, "tot": 3.5e-6}


# ---- B. the first-step dump at the step sizes the integrator runs at
PHASE_CELLS = (0, 7, -1)
PHASE_STATES = ("var_in", "var_out")
PHASE_H = (1.0e-3, 0.1, None, 10.0)       # None: the cell's Hexit, the last step size of the captured 10 s call (what the Hstart-reuse path feeds back)
LU_TAIL_ULPS = 4                          # gas, aer: R = 1/U, the multiplier W*R against variant 4's, U*R and the un-scaling product — one rounding each
# tot: the tail block is factorised by MFMA steps = fused multiply-add chains, no derivable bound.  Measured on the CPU on the 2 x 12 matrices of
# phase_cases("tot", ...): emulator against variant 4, worst tail entry as a fraction of its row's maximum
# maximum: 7.4e-14 (variant 4 against variant 6, the oracle's own fma-contracted factorisation, moves the same entries by 9.5e-10: the yardstick).
# gas and aer on the same scale: 2.2e-16, at most 2.3 units of round-off of the entry.
TOT_TAIL_BOUND = 7.4e-13                  # 10 x the measured figure (the inputs are a sample); tests/test_schedule.py holds it to [10x, 100x]


def phase_cases(g, o, state):
    """-> V, F, K, H [12]: cells PHASE_CELLS of a golden set in `state`, each at the four first step sizes of PHASE_H"""
    n = g["var_in"].shape[0]
    cells = [c % n for c in PHASE_CELLS]
    idx, H = [], []
    for c in cells:
        hexit = o.integrate(g["var_in"][c], g["fix"][c], g["rconst"][c], 0.0, 10.0)[4]
        for h in PHASE_H:
            idx.append(c)
            H.append(hexit if h is None else h)
    return (np.ascontiguousarray(g[state][idx]), np.ascontiguousarray(g["fix"][idx]), np.ascontiguousarray(g["rconst"][idx]), np.array(H))


def row_scale(t, lu):
    """per entry: the largest magnitude of the entry's row"""
    return np.repeat(np.maximum.reduceat(np.abs(lu), t.crow[:-1]), np.diff(t.crow))


def unscale_tail(t, lu, tail_h):
    """the kernel keeps the upper triangle of the rows from tail_h on row-scaled, U'(i,c) = U(i,c)*R(i): multiply U(i,i) back in"""
    out = lu.copy()
    for r in range(tail_h, len(t.diag)):
        out[t.diag[r] + 1:t.crow[r + 1]] *= out[t.diag[r]]
    return out


def variant4_factors(o, G):
    """KppDecomp_x with its multipliers formed as W*(1/U(j,j)) — the one way the kernel's factorisation departs from the reference's"""
    from oracle.oracle import set_variant
    try:
        set_variant(4)
        lu, ier = o.decomp(G)
    finally:
        set_variant(0)
    assert ier == 0
    return lu


def check_lu_against_variant4(mech, t, tail_h, lu_kernel_form, lu_v4):
    """Head rows bit for bit; tail rows to LU_TAIL_ULPS of each entry (gas, aer) or TOT_TAIL_BOUND of the row maximum (tot).
    -> (worst tail |diff| / |entry| in units of U, worst tail |diff| / row maximum)"""
    lu = unscale_tail(t, lu_kernel_form, tail_h)
    head = t.crow[tail_h]
    assert np.array_equal(lu[:head], lu_v4[:head]), "%s: head rows of the factors differ from variant 4 of the oracle" % mech
    d = np.abs(lu[head:] - lu_v4[head:])
    ref = np.abs(lu_v4[head:])
    of_row = (d / row_scale(t, lu_v4)[head:]).max()
    ulps = (d[ref > 0] / ref[ref > 0]).max() / U if (ref > 0).any() else 0.0
    if mech == "tot":
        assert of_row <= TOT_TAIL_BOUND, "tot: tail rows %.2e of the row maximum from variant 4, bound %.2e" % (of_row, TOT_TAIL_BOUND)
    else:
        assert np.array_equal(lu[head:][ref == 0], lu_v4[head:][ref == 0])
        assert ulps <= LU_TAIL_ULPS, "%s: tail rows %.2f units of round-off from variant 4, bound %d" % (mech, ulps, LU_TAIL_ULPS)
    return ulps, of_row


ALL_VARIANTS = (0, 1, 2, 3, 4, 5, 6, 7)


def solve_reference_and_spread(o, lu_v4, rhs):
    """-> (x, spread): KppSolve_x on variant-4 factors by the oracle's solve that multiplies by the pivot's reciprocal (variant 4), and how far the
    oracle's other solve variants move from it on the same factors and right-hand side, as a fraction of max|x|"""
    from oracle.oracle import set_variant
    try:
        set_variant(4)
        x = o.solve(lu_v4, rhs)
        spread = 0.0
        for v in ALL_VARIANTS:
            set_variant(v)
            spread = max(spread, np.abs(o.solve(lu_v4, rhs) - x).max() / np.abs(x).max())
    finally:
        set_variant(0)
    return x, spread


def check_k_vectors(mech, found):
    """found: (index of the first step size in PHASE_H, |K - reference| / max|reference|, spread of the oracle's solve variants) of every cell and
    stage of one launch.  Bound per step size: 10x the largest spread at that step size.  (Per step size and not per solve: the spread of ONE solve is
    the largest gap between eight roundings of one vector and drops to 1e-22 where they happen to coincide, while what it estimates — the conditioning
    of Ghimj at that H — belongs to the matrix; and the kernel's tail chain works on row-scaled rows, a re-association that is none of the eight.)
    -> {H index: (worst error, spread)}"""
    out = {}
    for hi in sorted({f[0] for f in found}):
        err = max(f[1] for f in found if f[0] == hi)
        spread = max(f[2] for f in found if f[0] == hi)
        out[hi] = (err, spread)
        assert err <= 10.0 * spread, "%s, first step size #%d: K vectors %.2e from the oracle's solve, its own variants spread by %.2e" % (mech, hi, err, spread)
    return out


# ---- D. rejected steps after an accepted one, long and backward horizons, IERR = -7 from a finite state.
# name: (golden set suffix, mechanism, cells, tin, tout, IERR, Nrej per cell, largest Nstp).  Chosen on the oracle: every variant leaves IERR and /Statistics/
# of these cells unchanged (tests/test_oracle.py holds that), which e.g. aer cell 1 at 0.02 -> 0 does not.
REJECT_CASES = {
    "gas_day_backward": ("_day", "gas", tuple(range(8)), 0.5, 0.0, 1, (2, 6, 1, 8, 2, 5, 0, 3), 28),
    "gas_backward": ("", "gas", (2,), 5.0, 0.0, 1, (6,), 22),
    "aer_hour": ("", "aer", (3, 6, 7), 0.0, 3600.0, 1, (1, 2, 2), 246),
    "tot_day_hour": ("_day", "tot", (1, 4, 7), 0.0, 3600.0, 1, (1, 1, 1), 249),
    "tot_backward_fails": ("", "tot", (0, 1), 0.02, 0.0, -7, (18, 31), 441),
}
# worst rel_diff (conftest) of the oracle's VARIANTS against the pinned oracle on that input, and the bound: 10x
#   measured (CPU):  gas_day_backward 3.23e-16  gas_backward 2.15e-16  aer_hour 8.30e-5  tot_day_hour 1.73e-5  tot_backward_fails 8.84e-14
# exit time (as a fraction of the larger end of the interval) and last accepted step size move further than the state does where the state hardly moves
# (gas): they follow Err**(1/3), to which every species contributes alike.  The same variants on the same inputs, and the bound, 10x:
#   measured (CPU):  gas_day_backward 1.32e-14  gas_backward 2.33e-15  aer_hour 1.09e-4  tot_day_hour 1.24e-5  tot_backward_fails 7.41e-14
REJECT_TH_RTOL = {"gas_day_backward": 1.4e-13, "gas_backward": 2.4e-14, "aer_hour": 1.1e-3, "tot_day_hour": 1.3e-4, "tot_backward_fails": 7.5e-13}
# VAR: worst rel_diff (conftest) of the same variants, and the bound, 10x
REJECT_RTOL = {"gas_day_backward": 3.3e-15, "gas_backward": 2.2e-15, "aer_hour": 8.4e-4, "tot_day_hour": 1.8e-4, "tot_backward_fails": 9.0e-13}


def reject_case_inputs(name):
    from conftest import load_golden
    suffix, mech, cells, tin, tout, ierr, nrej, nstp = REJECT_CASES[name]
    g = load_golden(mech, suffix)
    c = list(cells)
    return mech, g["var_in"][c], g["fix"][c], g["rconst"][c], tin, tout


# ---- F. the liq_parm kernels on the seeded cases of tests/liq_cases.py (tests/test_gpu_liq_synth.py), where a result passes through exp or log.
# Spread: the worst relative movement of the restatement itself (oracle/liq_py.py, oracle/kmt_py.py, oracle/rates_py.py) over those cases when exp, log,
# log10, pow and sqrt return the next double up, or down (liq_cases.MathShim), measured by
# tests/test_liq_cases.py::test_bounds_of_the_synthetic_comparisons_follow_the_restatements_own_movement.  Bound = max(LIQ_SYNTH_FLOOR, 10 x spread).
#   measured (CPU):  henry 5.94e-16  equil_co 5.89e-16  dry_rates (xeq, the gas routine's henry4) 4.30e-16  st_coeff 5.21e-16  vt 1.30e-15
# (200-320 K, against the 281-288 K of the captured layers: the temperature laws' exponents grow to ~16 and with them the last place of exp's argument,
# which this measure does not move — argument roundings are the same operations on both sides.)  vt: Beard's polynomial sits between a log and an exp.
LIQ_SYNTH_FLOOR = 1e-14            # what tests/test_gpu_liq.py, tests/test_gpu_kmt.py (vt) and tests/test_gpu_rates.py (st_coeff) hold on the captured layers
LIQ_SYNTH_RTOL = {"henry": LIQ_SYNTH_FLOOR, "equil_co": LIQ_SYNTH_FLOOR, "dry_rates": LIQ_SYNTH_FLOOR, "st_coeff": LIQ_SYNTH_FLOOR, "vt": 1.3e-14}


# ---- G. the rate evaluator on the edge cases of tests/rates_cases.py (tests/test_gpu_rates_edges.py), in the programs that hold a call of a rate law
# with exp, pow or log10 in it (rates_cases.LIBRARY_LAWS; every other program is compared bit for bit).  Spread: the worst relative movement of the
# restatement itself (oracle/rates_py.py) over those cases when exp, pow and log10 return the next double up, or down (liq_cases.MathShim), NaN,
# infinite and exactly-zero entries left out (the GPU test holds those patterns equal), measured by
# tests/test_rates_cases.py::test_bound_of_the_device_comparison_follows_the_restatements_own_movement.  Bound = max(RATES_EDGES_FLOOR, 10 x spread).
#   measured (CPU):  gas 5.93e-16 (1 987 entries)  aer 8.07e-16 (8 923)  tot 8.07e-16 (14 185)
# (180-330 K against the 220-310 K of the seeded fixture; the Troe laws chain two pow, a log10 and a pow.)  No entry cancels: the comparison leaves
# none to a looser bound.
RATES_EDGES_FLOOR = 1e-13          # what tests/test_gpu_rates.py holds on the seeded and the captured vectors
RATES_EDGES_RTOL = {"gas": RATES_EDGES_FLOOR, "aer": RATES_EDGES_FLOOR, "tot": RATES_EDGES_FLOOR}
