"""Bounds of the tests of the per-cell tolerance entries on the GPU (tests/test_gpu_ros_celltol.py), MEASURED ON THE REFERENCE SIDE exactly as
tests/ros_methods_bounds.py measures its own: nothing here looks at the kernel.  The expected values are the compiled Rosenbrock_x's, called once per
cell with the cell's row (tests/golden/ros_celltol_<mech>.npz); the spread is the movement of its bit-identical restatement (tests/ros_celltol_py.py
over tests/ros_methods_py.py) under the oracle's legal re-associations (oracle.set_variant over parity_bounds.VARIANTS) on the fixture's own sets.
tests/test_ros_celltol.py re-measures every figure and holds every constant to [10x, 100x] of it, with floor parity_bounds.PARITY_FLOOR
(check_constant).

Premise, held by the same test: no variant changes IERR or IPAR(11:18) on any (set, cell) of the fixture, so every (set, cell) is compared in full.

  measured (CPU):  VAR, worst rel_diff (conftest)                        gas 2.75e-16   aer 1.45e-6   tot 3.73e-8
                   exit time / last accepted step size (th_diff)         gas 0          aer 9.69e-5   tot 3.59e-8

Trace records: tests/ros_trace_bounds.py is used as it is, and its constants were measured on ros_trace_py's sets.  On the sets here the restated
records move as follows under the same variants (T, H, Err, share; measure_trace_spread):
  gas rel_1e-13    0        0        7.94e-7  6.96e-7        gas vector_rows  0        0        1.16e-9  5.10e-9
  aer rel_1e-13    1.48e-8  5.29e-8  3.59e-4  1.98e-4        aer vector_rows  3.84e-6  1.03e-5  3.17e-4  3.88e-4
  tot rel_1e-13    1.44e-9  3.84e-8  5.60e-5  7.13e-5        tot vector_rows  5.20e-9  1.17e-7  1.74e-6  1.58e-6
Where 10x that movement lies inside ros_trace_bounds' constants (TRACE_RECORD_SETS) the GPU records are compared with the restatement within them.
Elsewhere (aer vector_rows: T, H; tot: Err, share on both sets — the restatement itself moves by more than the constant on tot rel_1e-13) the
constants say nothing about the set, and the records are held bit for bit to the shared trace entry run per cell with the cell's row as its pair,
whose records tests/test_gpu_ros_trace.py holds to those constants on the sets they were measured on."""
import numpy as np

import parity_bounds as pb
from ros_options_bounds import th_diff, var_diff  # noqa: F401

# VAR against the fixture, rel_diff of conftest.  gas: 10x the spread is 2.8e-15, below the floor
CELLTOL_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 1.5e-5, "tot": 3.8e-7}
# exit time (as a fraction of the larger end of the interval) and last accepted step size (relative), as ros_options_bounds.OPTIONS_TH_RTOL is taken.
# gas: no variant moves either on these sets, the floor
CELLTOL_TH_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 9.7e-4, "tot": 3.6e-7}
# (mechanism: sets) whose trace records are compared with the restatement within tests/ros_trace_bounds.py as it is; held by tests/test_ros_celltol.py
TRACE_RECORD_SETS = {"gas": ("rel_1e-13", "vector_rows"), "aer": ("rel_1e-13",), "tot": ()}


def measure_spread(mech, golden_set, names=None):
    """-> (VAR spread, Texit / Hexit spread, [(variant, set) whose IERR or counters moved]) of the restatement over parity_bounds.VARIANTS"""
    import ros_celltol_py as RC
    names = RC.SET_NAMES if names is None else names
    base = RC.restated(mech, golden_set, 0, names)
    s_var, s_th, moved = 0.0, 0.0, []
    for v in pb.VARIANTS:
        r = RC.restated(mech, golden_set, v, names)
        for name in names:
            b, x = base[name], r[name]
            if not (np.array_equal(b[1], x[1]) and np.array_equal(b[2], x[2])):
                moved.append((v, name))
                continue
            s_var = max(s_var, var_diff(x[0], b[0]))
            s_th = max(s_th, *th_diff(x[3], x[4], b[3], b[4]))
    return s_var, s_th, moved


def measure_trace_spread(mech, golden_set, name):
    """-> ((T, H, Err, share) spreads, [(variant, cell) whose record count, codes or species moved]) of ros_trace_py.rosenbrock_trace called per cell
    with the cell's row of set `name`, over parity_bounds.VARIANTS"""
    import ros_celltol_py as RC
    import ros_trace_bounds as tb
    import ros_trace_py as RT
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    g = golden_set
    cells = list(RC.cells_of(g["var_in"].shape[0]))
    nvar = g["var_in"].shape[1]
    o, diag = Oracle(mech), mechtab.load(mech).diag
    ipar, rpar, atol, rtol = RC.celltol_set(mech, name, g["var_in"][cells])

    def run(v):
        try:
            set_variant(v)
            return [RT.rosenbrock_trace(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, RC.full_row(atol[i], nvar),
                                        RC.full_row(rtol[i], nvar)) for i, c in enumerate(cells)]
        finally:
            set_variant(0)
    base = RC.traced(mech, g, (name,))[name]
    spread, moved = [0.0, 0.0, 0.0, 0.0], []
    for v in pb.VARIANTS:
        for c, (b, x) in enumerate(zip(base, run(v))):
            t0, t1 = b[5], x[5]
            if not (len(t0.t) == len(t1.t) and np.array_equal(t0.code, t1.code) and np.array_equal(t0.species, t1.species)):
                moved.append((v, c))
                continue
            d = tb.record_diff((t1.t, t1.h, t1.err, t1.share), (t0.t, t0.h, t0.err, t0.share))
            spread = [max(a, e) for a, e in zip(spread, d)]
    return tuple(spread), moved
