"""The bound on the solves of the operators (mistra_chem_ops_ex / _device) and the cases it is held on.  MEASURED ON THE REFERENCE
SIDE: nothing here looks at the kernel.

A forward comparison of x is meaningless here: the oracle's own re-association variants (oracle.set_variant 0, 1, 2, 4, 6, 7: fused multiply-adds,
reciprocal pivots, sweep order — the kernel's deliberate departures) move x by up to 1e-3 of max|x| at the small shift, where J is nearly singular along
conserved sums.  The yardstick is the row-wise backward error (tests/mech_ops_py.py: backward_error), in long double from the oracle's A:

    omega = max_i |b - A x|_i / (||A_i||_1 * ||x||_inf + |b_i|)

The cases, per mechanism: eight cells of the captured BTZ96 column (CELLS: evenly spread, first and last included), the four shifts
+-1/(1e-3*gamma1), 1/(10*gamma1), 1e-4, and three right-hand sides, the cell's vdot, its var and a seeded normal vector.

  ORACLE_OMEGA   the oracle's worst omega over those cases and the six variants (A and b are the pinned restatement's, variant 0: the matrix the kernel
                 forms bit for bit; the variant factorises and solves).  tests/test_mech_ops.py re-measures it and holds that the figure recorded here
                 is not below the measurement.
  OMEGA_BOUND    10 x ORACLE_OMEGA per mechanism: the project's margin over the reference's own spread.  The kernel is held to it
                 (tests/test_gpu_mech_ops.py), on every case, for the fun_rhs row and for every explicit row.
  GPU_OMEGA      what the kernel measured on the MI355X on the same cases (recorded, not asserted: the assertion is OMEGA_BOUND)."""
import numpy as np

import mech_ops_py as MO

VARIANTS = (0, 1, 2, 4, 6, 7)
NCELLS = 8
ORACLE_OMEGA = {"gas": 1.65e-16, "aer": 1.52e-16, "tot": 2.49e-16}      # measured 1.646e-16 (variants 0, 1, 2), 1.515e-16 (all six), 2.4805e-16 (variant 1), rounded up
OMEGA_BOUND = {m: 10.0 * v for m, v in ORACLE_OMEGA.items()}
GPU_OMEGA = {"gas": 1.798e-16, "aer": 1.604e-16, "tot": 2.016e-16}      # the same at all four shifts' running maximum: set at the first (largest) shift


def cells(mech):
    """the eight cells of the column the bound is held on -> (indices, V, F, RCT)"""
    V, F, K = MO.column_cells(mech)
    idx = np.unique(np.linspace(0, V.shape[0] - 1, NCELLS).round().astype(int))
    return idx, V[idx], F[idx], K[idx]


def shifts():
    g = MO.GAMMA1
    return (1.0 / (1.0e-3 * g), -1.0 / (1.0e-3 * g), 1.0 / (10.0 * g), 1.0e-4)


def rhs_rows(mech, vdot, V):
    """the explicit right-hand sides of a batch: [3, ncell, NVAR] = the cells' vdot, their var, a seeded normal vector per cell"""
    rng = np.random.default_rng(16 + len(mech))
    return np.ascontiguousarray(np.stack([vdot, V, rng.standard_normal(V.shape)]))


def measure_oracle(mech, variants=VARIANTS):
    """-> the oracle's worst omega over the cases and `variants`"""
    from oracle import oracle as O
    orc = O.Oracle(mech)
    crow, icol, diag = MO.pattern(mech)
    _, V, F, K = cells(mech)
    O.set_variant(0)
    vdot = np.array([orc.fun(V[c], F[c], K[c]) for c in range(len(V))])
    jvs = [orc.jac_sp(V[c], F[c], K[c]) for c in range(len(V))]
    rows = rhs_rows(mech, vdot, V)
    worst = 0.0
    try:
        for v in variants:
            O.set_variant(v)
            for sh in shifts():
                for c in range(len(V)):
                    a = MO.prepared(jvs[c], diag, sh)
                    lu, ising = orc.decomp(a)
                    assert ising == 0, (mech, sh, c, ising)
                    for j in range(rows.shape[0]):
                        worst = max(worst, MO.backward_error(a, crow, icol, orc.solve(lu, rows[j, c]), rows[j, c]))
    finally:
        O.set_variant(0)
    return worst
