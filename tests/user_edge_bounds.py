"""Bounds of the edge-table GPU tests (tests/test_gpu_user_edges.py), MEASURED ON THE ORACLE'S SIDE by the scheme of tests/user_mech_bounds.py: nothing
here looks at a kernel.  Per edge table (tests/user_edge_cases.py) and run the figure is how far the oracle itself moves on the test cells under its
re-association variants 1, 2 and 4; the bound is 10x that, or PARITY_FLOOR where 10x lies below it.  tests/test_user_edges.py re-measures every figure,
holds every constant within [10x, 100x] of it (parity_bounds.check_constant) and FAILS if a variant changes IERR or one of the eight counters on a test
cell: that is what entitles the GPU tests to demand identical counters.

  measured (CPU), worst of cells 0, 16 and 31:     VAR (conftest.rel_diff)    exit time / 10 s, last step size (relative)
    edge_g64    base                                 5.6e-16                     1.39e-13
                rtol_1e-5                            1.1e-15                     2.11e-12
    edge_a128   base                                 2.30e-10                    4.54e-10
                rtol_1e-5                            1.39e-10                    5.57e-9
    edge_a129   base                                 3.60e-10                    3.54e-10
                rtol_1e-5                            1.63e-10                    2.24e-9
    edge_t417   base                                 1.26e-7                     7.89e-9
                rtol_1e-5                            2.44e-8                     1.10e-7
No cell had to be replaced for either run: cells 0, 16 and 31 keep IERR = 1 and all eight counters under every variant, on every table.
"""
import numpy as np

from parity_bounds import PARITY_FLOOR

VARIANTS = (1, 2, 4)
RUNS = ("base", "rtol_1e-5")      # INTEGRATE_x's values | RelTol = 1e-5 through Rosenbrock_x's options (user_mech_bounds.options_for)

# 10 x the measured spread, or the floor
VAR_RTOL = {("edge_g64", "base"): PARITY_FLOOR, ("edge_g64", "rtol_1e-5"): PARITY_FLOOR,
            ("edge_a128", "base"): 2.4e-9, ("edge_a128", "rtol_1e-5"): 1.4e-9,
            ("edge_a129", "base"): 3.7e-9, ("edge_a129", "rtol_1e-5"): 1.7e-9,
            ("edge_t417", "base"): 1.3e-6, ("edge_t417", "rtol_1e-5"): 2.5e-7}
TH_RTOL = {("edge_g64", "base"): 1.4e-12, ("edge_g64", "rtol_1e-5"): 2.2e-11,
           ("edge_a128", "base"): 4.6e-9, ("edge_a128", "rtol_1e-5"): 5.6e-8,
           ("edge_a129", "base"): 3.6e-9, ("edge_a129", "rtol_1e-5"): 2.3e-8,
           ("edge_t417", "base"): 7.9e-8, ("edge_t417", "rtol_1e-5"): 1.2e-6}


def options_for(name, run):
    import user_edge_cases as ec
    import user_mech_bounds as ub
    return ub.options_for(name, run, nvar=ec.SIZES[name][0])


_runs = {}


def oracle_run(name, run, variant=0):
    """The oracle on the test cells of an edge table -> (VAR [3, NVAR], IERR [3], counters [3, 8], Texit [3], Hexit [3]); "base" by the oracle's own
    integrator, "rtol_1e-5" by the restatement of Rosenbrock_x over the oracle's routines.  Computed once per (table, run, variant)."""
    key = (name, run, variant)
    if key not in _runs:
        import ros_options_py as R
        import user_edge_cases as ec
        from conftest import load_golden
        from oracle.oracle import set_variant
        ec.ensure_tables()
        o = ec.oracle(name)
        V, F, K = ec.cut_inputs(name, load_golden(ec.EDGES[name][0]))
        opts = options_for(name, run)
        try:
            set_variant(variant)
            if opts is None:
                rows = [o.integrate(V[i], F[i], K[i], 0.0, 10.0) for i in range(len(ec.CELLS))]
            else:
                diag = ec.tables(name).diag
                rows = [R.rosenbrock(o, diag, V[i], F[i], K[i], *opts, 0.0, 10.0) for i in range(len(ec.CELLS))]
        finally:
            set_variant(0)
        _runs[key] = tuple(np.array([r[i] for r in rows]) for i in range(5))
    return _runs[key]


def measure(name, run):
    """-> (spread of VAR, spread of exit time / last step size) of the oracle's variants on the test cells; asserts that no variant changes IERR or a
    counter of a cell"""
    import user_mech_bounds as ub
    from conftest import rel_diff
    var, ierr, st, te, he = oracle_run(name, run)
    s_var = s_th = 0.0
    for v in VARIANTS:
        var2, ierr2, st2, te2, he2 = oracle_run(name, run, v)
        assert np.array_equal(ierr2, ierr) and np.array_equal(st2, st), \
            "%s, %s: variant %d of the oracle changes IERR or a counter on a test cell (%s -> %s): choose another cell" % (name, run, v, st.tolist(), st2.tolist())
        s_var = max(s_var, rel_diff(var2, var).max())
        s_th = max(s_th, ub.th_diff(te2, he2, te, he))
    return s_var, s_th
