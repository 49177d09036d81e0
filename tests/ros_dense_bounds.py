"""Bounds of the whole-call tests of mistra_chem_rosenbrock_dense_ex on the GPU (tests/test_gpu_ros_dense.py), MEASURED ON THE REFERENCE SIDE exactly as
tests/ros_flux_bounds.py measures its own: nothing here looks at the kernel.  The expected values are the restatement's (tests/ros_dense_py.py: the
restatement of Rosenbrock_x that equals the compiled one bit for bit, with the sampling added); the spread is its own movement under the oracle's
re-associations parity_bounds.VARIANTS (oracle.set_variant 1, 2, 3, 4, 5, 7) on ros_dense_py.DENSE_SETS with the sets' sample times (times_of), three
cells (cells_of) of each mechanism's captured set.  tests/test_ros_dense.py re-measures the figures and holds every constant to [10x, 100x] of them,
with floor parity_bounds.PARITY_FLOOR.

The measure: conftest.rel_diff of a sample row, |got - want| / (|want| + 1e-12 * the row's largest concentration), the worst species of the worst
reached sample (rows behind nout are +0.0 on both sides and are compared for that, not measured).

Premise, held by the same test: no variant changes IERR, IPAR(11:18) or nout on any (set, cell) — what entitles the GPU test to demand identical
counters and nout.  No (set, cell) is left out and no sample time had to be moved.

  measured (CPU):  samples by rel_diff, worst set    gas 6.57e-15 (floor)   aer 1.13e+3 (m5)   tot 8.15 (m5)
                   no counter and no nout moved; the Max_no_steps set reaches 15 of 16 (gas), 4 (aer), 2 (tot) samples on every cell

What the large figures are.  aer's and tot's are set by two or three stiff trace species (aer 106 and 59, tot 71 and 154) whose interpolated value, 1e-16
.. 1e-11, is what cancels out of the terms dh*F_n and dh*F_(n+1) inside a long late step, next to a row maximum of 1.6e-2: a re-association moves the
steps by 1e-8 and that residue by several times itself, and rel_diff's floor (1e-12 of the row maximum) lies below it.  It is a property of the cubic
Hermite interpolant on a stiff system, stated in INTEGRATION.md 4o, and as a relative bound DENSE_RTOL holds those two mechanisms to little.  So the GPU
test holds a SECOND measure as well, found and held in exactly the same way: |got - want| over the row's largest concentration, in which no species'
own smallness enters.

  measured (CPU):  samples over the row maximum      gas 1.31e-16 (floor)   aer 1.37e-7   tot 3.80e-10"""
import numpy as np

import parity_bounds as pb
from conftest import rel_diff

DENSE_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 1.2e4, "tot": 8.2e1}
DENSE_SCALED = {"gas": pb.PARITY_FLOOR, "aer": 1.4e-6, "tot": 3.9e-9}


def sample_diff(got, want, nout):
    """worst rel_diff over the reached samples of the cells of one set; got, want [ncell, ns, NVAR], nout [ncell]"""
    worst = 0.0
    for c, n in enumerate(np.asarray(nout)):
        if n > 0:
            worst = max(worst, float(rel_diff(got[c][:n], want[c][:n]).max()))
    return worst


def scaled_diff(got, want, nout):
    """the second measure: worst |got - want| / the row's largest concentration over the reached samples (no species' own smallness enters)"""
    worst = 0.0
    for c, n in enumerate(np.asarray(nout)):
        if n > 0:
            worst = max(worst, float((np.abs(got[c][:n] - want[c][:n]) / np.abs(want[c][:n]).max(axis=1, keepdims=True)).max()))
    return worst


def measure_spread(mech, golden_set, names=None):
    """-> (sample spread by rel_diff, by the scaled measure, [(variant, set) whose IERR, counters or nout moved]) of the restatement over
    parity_bounds.VARIANTS"""
    import ros_dense_py as RD
    names = RD.DENSE_SETS if names is None else names
    base = RD.restated(mech, golden_set, 0, names)
    spread, scaled, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = RD.restated(mech, golden_set, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2]) and np.array_equal(b[6], x[6])):
                moved.append((v, name))
                continue
            spread = max(spread, sample_diff(x[5], b[5], b[6]))
            scaled = max(scaled, scaled_diff(x[5], b[5], b[6]))
    return spread, scaled, moved


def check(mech, spread, scaled):
    pb.check_constant("DENSE_RTOL[%s]" % mech, DENSE_RTOL[mech], spread, floor=pb.PARITY_FLOOR)
    pb.check_constant("DENSE_SCALED[%s]" % mech, DENSE_SCALED[mech], scaled, floor=pb.PARITY_FLOOR)
