"""Bounds of the tests of the step-control trace on the GPU (tests/test_gpu_ros_trace.py), MEASURED ON THE REFERENCE SIDE exactly as
tests/ros_methods_bounds.py measures its own: nothing here looks at the kernel.  The expected records are those of the restatement
(tests/ros_trace_py.py, pinned through tests/ros_methods_py.py to the compiled Rosenbrock_x); the spread is the movement of those records under the
oracle's legal re-associations (oracle.set_variant over parity_bounds.VARIANTS) on the trace tests' own sets (ros_trace_py.SET_NAMES), cells 0, n/2,
n-1 of integrate_<mech>.npz, 0 -> 10 s.  tests/test_ros_trace.py re-measures every figure and holds every constant to [10x, 100x] of it, with floor
parity_bounds.PARITY_FLOOR (check_constant).

Premises, held by the same test: no variant changes the number of records, a record's code or its species on any (set, cell, attempt).

  measured (CPU):  T, of the interval's end   gas 0          aer 1.01e-6   tot 3.03e-8
                   H, relative                gas 0          aer 3.13e-6   tot 1.03e-7
                   Err, relative              gas 4.61e-5    aer 1.88e-2   tot 4.38e-7
                   share, absolute            gas 2.18e-5    aer 1.49e-2   tot 7.11e-7"""
import numpy as np

import parity_bounds as pb

# T at the start of the step, as a fraction of the larger end of the interval, and H as attempted, relative.  gas: no variant moves either (every
# step of its seven runs into FacMax), the constant is the floor
TRACE_T_TOL = {"gas": pb.PARITY_FLOOR, "aer": 1.1e-5, "tot": 3.1e-7}
TRACE_H_RTOL = {"gas": pb.PARITY_FLOOR, "aer": 3.2e-5, "tot": 1.1e-6}
# Err, relative, and the largest term's share of NVAR*Err**2, absolute.  Err moves further than H does: small error estimates are differences of
# nearly equal stage vectors, and the step size follows their cube root between FacMin and FacMax only
TRACE_ERR_RTOL = {"gas": 4.7e-4, "aer": 1.9e-1, "tot": 4.4e-6}
TRACE_SHARE_TOL = {"gas": 2.2e-4, "aer": 1.5e-1, "tot": 7.2e-6}


def record_diff(got, want, tin=0.0, tout=10.0):
    """got, want: (t, h, err, share) arrays of the same attempts -> (T difference on the scale of the interval's ends, relative difference of H, of
    Err, absolute difference of share); two NaNs, or two equal infinities, count 0"""
    def rel(a, b, scale):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        if a.size == 0:
            return 0.0
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(same, 0.0, np.abs(a - b) / scale(b))
        d = np.where(np.isnan(d), np.inf, d)      # a NaN on one side only, or infinities that differ
        return float(d.max())
    ends = max(abs(tin), abs(tout))
    own = lambda b: np.where(b != 0.0, np.abs(b), 1.0)  # noqa: E731
    return (rel(got[0], want[0], lambda b: ends), rel(got[1], want[1], own), rel(got[2], want[2], own), rel(got[3], want[3], lambda b: 1.0))


def measure_spread(mech, golden_set, names=None):
    """-> ((T, H, Err, share) spreads, [(variant, set, cell) whose record count, codes or species moved]) of the restated trace over
    parity_bounds.VARIANTS"""
    import ros_trace_py as RT
    names = RT.SET_NAMES if names is None else names
    base = RT.restated(mech, golden_set, 0, names)
    spread, moved = [0.0, 0.0, 0.0, 0.0], []
    for v in pb.VARIANTS:
        r = RT.restated(mech, golden_set, v, names)
        for name in names:
            for c, (b, x) in enumerate(zip(base[name], r[name])):
                tb, tx = b[5], x[5]
                if not (len(tb.t) == len(tx.t) and np.array_equal(tb.code, tx.code) and np.array_equal(tb.species, tx.species)
                        and b[1] == x[1] and np.array_equal(b[2], x[2])):
                    moved.append((v, name, c))
                    continue
                d = record_diff((tx.t, tx.h, tx.err, tx.share), (tb.t, tb.h, tb.err, tb.share))
                spread = [max(s, e) for s, e in zip(spread, d)]
    return tuple(spread), moved
