"""TEST INFRASTRUCTURE — the sets the tests of the per-cell tolerance entries run (include/mistra_chem.h: mistra_chem_rosenbrock_cells_ex / _device and
their trace forms).  Tolerances per cell need no restatement of their own: Rosenbrock_x is one call per cell, so tests/ros_methods_py.py's rosenbrock
(and tests/ros_trace_py.py's rosenbrock_trace) is called per cell with that cell's row.  Cells are cells_of(n) of integrate_<mech>.npz, 0 -> 10 s.

Pinned as ros_methods_py is: on every (set, cell) below the restatement equals the compiled Rosenbrock_x bit for bit — VAR, IERR, IPAR(11:18), Texit,
Hexit (tests/test_ros_celltol.py, against tests/golden/ros_celltol_<mech>.npz, recorded by tests/golden/make_ros_celltol_golden.py)."""
import numpy as np

import ros_methods_py as RM
import ros_options_py as R
from ros_options_py import MECHS, NVAR, TIN, TOUT, cells_of  # noqa: F401

# name -> what the rows are, mode, method
SET_NAMES = ("rel_1e-13",            # AbsTol_c = 1e-13 x the cell's largest concentration, RelTol 1e-3; scalar, ntol = 1, Ros3
             "rel_1e-10_ntolN",      # AbsTol_c = 1e-10 x cell max in entry 0 of a row of NVAR; entries 1 .. hold 0.0 and are neither read nor checked; scalar, Ros3
             "vector_rows",          # row c = option_set(mech, "vector_tol")'s vectors with AbsTol x 10^c; RelTol rows 1e-3, 1e-4, 1e-2; vector, Ros3
             "m4_rel_1e-13",         # as rel_1e-13, Rodas3
             "m5_vector_rows",       # as vector_rows, Rodas4
             "m1_rel_1e-13",         # as rel_1e-13, Ros2
             "bad_cell_vector",      # vector_rows with AbsTol(51) = 0 in cell 1's row: that cell -5, the other two run
             "bad_cell_scalar",      # the same rows in scalar mode: everything runs, entry 51 is not read
             "bad_rtol_cell")        # rel_1e-13's rows with RelTol = 1 in cell 2: that cell -5
BAD_CELLS = {"bad_cell_vector": (1,), "bad_cell_scalar": (), "bad_rtol_cell": (2,)}
TRACE_SETS = ("rel_1e-13", "vector_rows", "bad_cell_vector")      # the Ros3 sets the trace entries are run on


def cell_max(v):
    """the largest |concentration| of each cell [n, NVAR] -> [n], NaN entries ignored (the host formula of mistra_chem_cell_atol_device)"""
    return np.fmax.reduce(np.abs(np.asarray(v, np.float64)), axis=-1)


def method_of(name):
    return int(name[1]) if name[0] == "m" and name[1].isdigit() else 2


def celltol_set(mech, name, var):
    """-> (IPAR, RPAR, AbsTol rows [n, ntol], RelTol rows [n, ntol]) for the cells whose states are var [n, NVAR] (n = 3 in the fixture: the rows of
    vector_rows depend on the cell's position c = 0, 1, 2 in the batch, taken modulo 3)"""
    var = np.asarray(var, np.float64)
    n, nvar = var.shape
    ipar, rpar, _, _ = R.base_options(mech)
    ipar[3] = method_of(name)
    kind = name[3:] if name[0] == "m" and name[1].isdigit() else name
    if kind in ("rel_1e-13", "bad_rtol_cell"):
        atol = (1.0e-13 * cell_max(var)).reshape(n, 1)
        rtol = np.full((n, 1), 1.0e-3)
        if kind == "bad_rtol_cell":
            rtol[2::3] = 1.0
    elif kind == "rel_1e-10_ntolN":
        atol, rtol = np.zeros((n, nvar)), np.zeros((n, nvar))
        atol[:, 0] = 1.0e-10 * cell_max(var)
        rtol[:, 0] = 1.0e-3
    elif kind in ("vector_rows", "bad_cell_vector", "bad_cell_scalar"):
        _, _, a, r = R.option_set(mech, "vector_tol")
        c = np.arange(n) % 3
        atol = a[None, :] * (10.0 ** c)[:, None]
        rtol = np.repeat(np.array([1.0e-3, 1.0e-4, 1.0e-2])[c][:, None], nvar, axis=1)
        ipar[1] = 0
        if kind != "vector_rows":
            atol[1::3, 50] = 0.0
        if kind == "bad_cell_scalar":
            ipar[1] = 1
    else:
        raise KeyError(name)
    return ipar, rpar, np.ascontiguousarray(atol), np.ascontiguousarray(rtol)


def full_row(row, nvar):
    """a tolerance row as Rosenbrock_x takes it, NVAR entries: a row of one entry repeated (scalar mode reads entry 1 alone)"""
    row = np.asarray(row, np.float64)
    return np.full(nvar, row[0]) if row.size == 1 else row.copy()


_restated = {}
_traced = {}


def restated(mech, golden, variant=0, names=SET_NAMES):
    """{set name: (VAR [3, NVAR], IERR [3], IPAR(11:18) [3, 8], Texit [3], Hexit [3])} of ros_methods_py.rosenbrock called per cell with the cell's
    row, for one oracle variant; computed once per (mechanism, variant, set) and shared by the tests"""
    from mistra_amd import mechtab
    from oracle.oracle import Oracle, set_variant
    o, diag, g = None, None, golden
    cells = list(cells_of(g["var_in"].shape[0]))
    out = {}
    for name in names:
        key = (mech, variant, name)
        if key not in _restated:
            if o is None:
                o, diag = Oracle(mech), mechtab.load(mech).diag
            ipar, rpar, atol, rtol = celltol_set(mech, name, g["var_in"][cells])
            nvar = g["var_in"].shape[1]
            try:
                set_variant(variant)
                rows = [RM.rosenbrock(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, full_row(atol[i], nvar), full_row(rtol[i], nvar))
                        for i, c in enumerate(cells)]
            finally:
                set_variant(0)
            _restated[key] = tuple(np.array([r[i] for r in rows]) for i in range(5))
        out[name] = _restated[key]
    return out


def traced(mech, golden, names=TRACE_SETS):
    """{set name: [ros_trace_py.rosenbrock_trace's tuple per cell, called with the cell's row]} (Ros3 sets only)"""
    import ros_trace_py as RT
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    g = golden
    cells = list(cells_of(g["var_in"].shape[0]))
    nvar = g["var_in"].shape[1]
    out = {}
    for name in names:
        key = (mech, name)
        if key not in _traced:
            o, diag = Oracle(mech), mechtab.load(mech).diag
            ipar, rpar, atol, rtol = celltol_set(mech, name, g["var_in"][cells])
            _traced[key] = [RT.rosenbrock_trace(o, diag, g["var_in"][c], g["fix"][c], g["rconst"][c], ipar, rpar, full_row(atol[i], nvar),
                                                full_row(rtol[i], nvar)) for i, c in enumerate(cells)]
        out[name] = _traced[key]
    return out


# ---- mistra_chem_cell_atol_device: the rows its tests run
ATOL_EDGE_KINDS = ("ordinary", "all_zero", "nan_at_max", "negative", "minus_zero", "inf", "max_lane0", "max_lane63", "max_last")


def atol_edge_rows(nvar, ncell, seed=11):
    """[ncell, NVAR] states, row c of kind ATOL_EDGE_KINDS[c % 9]: ordinary values; all zero; a NaN where the maximum was; negative values (the
    largest magnitude negative); -0.0 throughout; an Inf; the maximum in species 0 (lane 0), 63 (lane 63) and NVAR - 1"""
    rng = np.random.default_rng(seed)
    v = 10.0 ** rng.uniform(-20.0, 12.0, (ncell, nvar))
    for c in range(ncell):
        kind = ATOL_EDGE_KINDS[c % len(ATOL_EDGE_KINDS)]
        if kind == "all_zero":
            v[c] = 0.0
        elif kind == "nan_at_max":
            v[c, np.argmax(v[c])] = np.nan
        elif kind == "negative":
            v[c] = -v[c]
            v[c, ::3] *= -1.0e-3
        elif kind == "minus_zero":
            v[c] = -0.0
        elif kind == "inf":
            v[c, (7 * c) % nvar] = np.inf
        elif kind == "max_lane0":
            v[c, 0] = 3.0e13
        elif kind == "max_lane63":
            v[c, 63] = 3.0e13
        elif kind == "max_last":
            v[c, nvar - 1] = -3.0e13
    return v


def cell_atol_plain(v, factor, floor):
    """max(floor, factor * max_i |v_i|) per row in plain Python floats, NaN entries skipped: what the header states, written without numpy"""
    out = []
    for row in np.asarray(v, np.float64):
        m = 0.0
        for x in row.tolist():
            a = abs(x)
            if a > m:
                m = a
        r = factor * m
        out.append(r if r > floor else floor)
    return np.array(out, np.float64).reshape(-1, 1)
