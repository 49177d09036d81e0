"""Bounds of the user-slot GPU tests (tests/test_gpu_user_mech.py), MEASURED ON THE ORACLE'S SIDE as tests/parity_bounds.py does it: nothing here looks
at a kernel.  Per demo table (tests/user_mech_cases.py) and per run — INTEGRATE_x's values, and the two option sets the GPU test puts in force — the
figure is how far the oracle itself moves on the test cells under its re-association variants 1, 2 and 4 (oracle.set_variant: descending backward
sweep, contracted multiply-adds, pivots' reciprocals); the bound is 10x that, or PARITY_FLOOR where 10x lies below it.
tests/test_user_mech.py re-measures every figure, holds every constant within [10x, 100x] of it (parity_bounds.check_constant) and FAILS if a variant
changes IERR or one of the eight counters on a test cell: that, and no allowance for cells that drift, is what entitles the GPU tests to demand
identical counters.  Cells 0, 16 and 31 of the captured sets pass it for both tables (none had to be replaced).

  measured (CPU), worst of the three cells:        VAR (conftest.rel_diff)    exit time / 10 s, last step size (relative)
    demo_g   base                                   2.7e-20                    0
             rtol_1e-5                              4.3e-16                    2.47e-14
             vector_tol                             2.7e-20                    0
    demo_a   base                                   9.28e-7                    2.18e-5
             rtol_1e-5                              8.42e-7                    1.18e-4
             vector_tol                             9.82e-7                    1.79e-7
             hstart                                 8.81e-7                    -
    (demo_g hstart: 2.1e-16)
(demo_g hardly moves: its cells run at the largest step from the second step on, and 10x its spreads lie below the floor but for one figure.)
"""
import numpy as np

from parity_bounds import PARITY_FLOOR

VARIANTS = (1, 2, 4)
RUNS = ("base", "rtol_1e-5", "vector_tol", "hstart")      # INTEGRATE_x's values | RelTol = 1e-5 | vector tolerances (as ros_options_py.option_set, sized to the
#                                                           table) | INTEGRATE_x's values from a per-cell first step (VAR and counters only)

# 10 x the measured spread, or the floor
VAR_RTOL = {("demo_g", "base"): PARITY_FLOOR, ("demo_g", "rtol_1e-5"): PARITY_FLOOR, ("demo_g", "vector_tol"): PARITY_FLOOR,
            ("demo_g", "hstart"): PARITY_FLOOR,
            ("demo_a", "base"): 9.3e-6, ("demo_a", "rtol_1e-5"): 8.5e-6, ("demo_a", "vector_tol"): 9.9e-6, ("demo_a", "hstart"): 8.9e-6}
# (no entry for "hstart": the oracle's entry with a per-cell first step reports neither)
TH_RTOL = {("demo_g", "base"): PARITY_FLOOR, ("demo_g", "rtol_1e-5"): 2.5e-13, ("demo_g", "vector_tol"): PARITY_FLOOR,
           ("demo_a", "base"): 2.2e-4, ("demo_a", "rtol_1e-5"): 1.2e-3, ("demo_a", "vector_tol"): 1.8e-6}


def options_for(name, run, nvar=None):
    """IPAR, RPAR, AbsTol, RelTol of a run for a demo table (None for "base": INTEGRATE_x's values, no options in force).  nvar: the size of a
    table that is not one of the demo tables (tests/user_edge_bounds.py)."""
    import user_mech_cases as uc
    if run in ("base", "hstart"):
        return None
    nvar = nvar or uc.SIZES[name][0]
    ipar, rpar = np.zeros(20, np.int32), np.zeros(20)      # over INTEGRATE_x's base, as ros_options_py.option_set builds its sets
    ipar[1], ipar[3] = 1, 2
    rpar[2] = 1.0e-3
    atol, rtol = np.full(nvar, 1.0e-25), np.full(nvar, 1.0e-3)
    if run == "rtol_1e-5":
        rtol[:] = 1.0e-5
    elif run == "vector_tol":
        rng = np.random.default_rng(7)
        ipar[1] = 0
        rtol[:] = 10.0 ** rng.uniform(-4.0, -2.0, nvar)
        atol[:] = 1.0e-25 * 10.0 ** rng.uniform(0.0, 10.0, nvar)
    else:
        raise KeyError(run)
    return ipar, rpar, atol, rtol


def th_diff(te, he, te_ref, he_ref, span=10.0):
    """worst |exit time difference| / span and worst relative difference of the last accepted step size"""
    te, he, te_ref, he_ref = (np.atleast_1d(np.asarray(x, np.float64)) for x in (te, he, te_ref, he_ref))
    d_te = np.abs(te - te_ref).max() / span
    d_he = (np.abs(he - he_ref) / np.maximum(np.abs(he_ref), 1e-300)).max()
    return max(d_te, d_he)


_runs = {}


def oracle_run(name, run, variant=0):
    """The oracle on the test cells of a demo table -> (VAR [3, NVAR], IERR [3], counters [3, 8], Texit [3], Hexit [3]); "base" by the oracle's own
    integrator, the option sets by the restatement of Rosenbrock_x over the oracle's routines.  Computed once per (table, run, variant)."""
    key = (name, run, variant)
    if key not in _runs:
        import ros_options_py as R
        import user_mech_cases as uc
        from conftest import load_golden
        from mistra_amd import mechtab
        from oracle.oracle import Oracle, set_variant
        uc.ensure_tables()
        o = Oracle(name)
        V, F, K = uc.cut_inputs(name, load_golden(uc.DEMOS[name][0]), uc.CELLS)
        opts = options_for(name, run)
        try:
            set_variant(variant)
            if run == "hstart":      # every cell starts at the last step size of its "base" run (pinned oracle): the per-cell first step of the kernel's opt-in mode
                var, ierr, st = o.integrate_batch(V, F, K, 0.0, 10.0, hstart=oracle_run(name, "base")[4])
                rows = [(var[i], ierr[i], st[i], 0.0, 0.0) for i in range(len(uc.CELLS))]      # (that entry of the oracle does not report exit time and step size)
            elif opts is None:
                rows = [o.integrate(V[i], F[i], K[i], 0.0, 10.0) for i in range(len(uc.CELLS))]
            else:
                diag = mechtab.load(name).diag
                rows = [R.rosenbrock(o, diag, V[i], F[i], K[i], *opts, 0.0, 10.0) for i in range(len(uc.CELLS))]
        finally:
            set_variant(0)
        _runs[key] = tuple(np.array([r[i] for r in rows]) for i in range(5))
    return _runs[key]


def measure(name, run):
    """-> (spread of VAR, spread of exit time / last step size) of the oracle's variants on the test cells; asserts that no variant changes IERR or a
    counter of a cell"""
    from conftest import rel_diff
    var, ierr, st, te, he = oracle_run(name, run)
    s_var = s_th = 0.0
    for v in VARIANTS:
        var2, ierr2, st2, te2, he2 = oracle_run(name, run, v)
        assert np.array_equal(ierr2, ierr) and np.array_equal(st2, st), \
            "%s, %s: variant %d of the oracle changes IERR or a counter on a test cell (%s -> %s): choose another cell" % (name, run, v, st.tolist(), st2.tolist())
        s_var = max(s_var, rel_diff(var2, var).max())
        s_th = max(s_th, th_diff(te2, he2, te, he))
    return s_var, s_th
