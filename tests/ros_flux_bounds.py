"""Bounds of the whole-call tests of mistra_chem_rosenbrock_flux_ex on the GPU (tests/test_gpu_ros_flux.py), MEASURED ON THE REFERENCE SIDE exactly as
tests/ros_methods_bounds.py measures its own: nothing here looks at the kernel.  The expected values are the restatement's (tests/ros_flux_py.py: the
restatement of Rosenbrock_x that equals the compiled one bit for bit, with the flux sum added); the spread is its own movement under the oracle's
re-associations ros_flux_py.FLUX_VARIANTS (oracle.set_variant 1, 2, 4) on ros_flux_py.FLUX_SETS, three cells (cells_of) of each mechanism's captured
set.  tests/test_ros_flux.py re-measures the figures and holds every constant to [10x, 100x] of them, with floor parity_bounds.PARITY_FLOOR.

The measure, per cell: |got - want| / (|want| + 1e-12 * max_r |want|), the worst reaction.

Premise, held by the same test: no variant changes IERR or IPAR(11:18) on any (set, cell) — what entitles the GPU test to demand identical counters.

  measured (CPU):  flux, worst set     gas 1.43e-14 (m4_backward; the forward sets 2e-16 .. 4e-16)   aer 5.85e-7 (m2)   tot 8.79e-9 (m2)
                   no counter moved; the restatement makes 7 .. 22 (gas), 9 .. 487 (aer), 11 .. 685 (tot) attempts per cell and set
                   S*flux - (Y(Texit) - Y(Tstart)), worst species as a fraction of the cell's largest concentration (the trapezoid's own error, not a
                   bound of any test):  gas 1.5e-15 .. 6.6e-15;  aer 4.8e-8 (Rodas4) .. 4.4e-5 (Ros4), 5.9e-3 with the vector tolerances (RelTol up to
                   1e-2);  tot 1.2e-8 (Rodas3) .. 2.8e-5 (Ros4)"""
import numpy as np

import parity_bounds as pb

FLUX_RTOL = {"gas": 1.5e-13, "aer": 5.9e-6, "tot": 8.8e-8}


def flux_diff(got, want):
    """worst |got - want| / (|want| + 1e-12 * max_r |want|) over the cells [ncell, NREACT] of one set"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    return float((np.abs(got - want) / (np.abs(want) + 1.0e-12 * np.abs(want).max(axis=1, keepdims=True))).max())


def measure_spread(mech, golden_set, names=None):
    """-> (flux spread, [(variant, set) whose IERR or counters moved]) of the restatement over ros_flux_py.FLUX_VARIANTS"""
    import ros_flux_py as RF
    names = RF.FLUX_SETS if names is None else names
    base = RF.restated(mech, golden_set, 0, names)
    spread, moved = 0.0, []
    for v in RF.FLUX_VARIANTS:
        r = RF.restated(mech, golden_set, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            spread = max(spread, flux_diff(x[5], b[5]))
    return spread, moved


def check(mech, spread):
    pb.check_constant("FLUX_RTOL[%s]" % mech, FLUX_RTOL[mech], spread, floor=pb.PARITY_FLOOR)
