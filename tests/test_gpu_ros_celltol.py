"""Tolerances per cell on the GPU (-m gpu): mistra_chem_rosenbrock_cells_ex / _device, their trace forms and mistra_chem_cell_atol_device.  Expected
values: the compiled reference's Rosenbrock_x called once per cell with the cell's row (tests/golden/ros_celltol_<mech>.npz); bounds:
tests/ros_celltol_bounds.py, measured on the reference side (tests/test_ros_celltol.py).  Three cells per launch — cells 0, n/2, n-1 of
integrate_<mech>.npz — unless a test says otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ros_celltol_bounds as cb
import ros_celltol_py as RC
import ros_methods_py as RM
import ros_options_py as R
from conftest import MECHS, REPO, load_golden

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}
NT = {"gas": 64, "aer": 256}      # threads per cell of the two mechanisms that keep two species per lane


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    yield c
    if c.device_count() != 1:      # whatever a test initialised: the other modules' fixtures start from init(0)
        c.finalize()
        c.init(0)
    for mech in MECHS:
        c.clear_options(mech)


def _cells(mech):
    g = load_golden(mech)
    c = list(RC.cells_of(g["var_in"].shape[0]))
    return np.ascontiguousarray(g["var_in"][c]), np.ascontiguousarray(g["fix"][c]), np.ascontiguousarray(g["rconst"][c])


def _fixture(mech):
    return dict(np.load(os.path.join(REPO, "tests", "golden", "ros_celltol_%s.npz" % mech)))


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _host(res):
    """a result tuple of either entry as numpy arrays, t_h cut to Texit, Hexit; the Trace, if any, as a tuple of arrays"""
    import torch
    torch.cuda.synchronize()
    r, th = res[0], res[1]
    out = [type(r)(_np(r.var), _np(r.ierr), _np(r.stats)), np.ascontiguousarray(_np(th)[:, :2])]
    if len(res) == 3:
        out.append(tuple(None if x is None else np.ascontiguousarray(_np(x)) for x in res[2]))
    return tuple(out)


def _same(a, b):
    """two _host tuples, bit for bit (a NaN equals itself)"""
    ok = a[0].var.tobytes() == b[0].var.tobytes() and np.array_equal(a[0].ierr, b[0].ierr) and np.array_equal(a[0].stats, b[0].stats) and a[1].tobytes() == b[1].tobytes()
    if ok and len(a) == 3:
        ok = len(b) == 3 and all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2]))
    return ok


def _take(h, idx):
    """rows idx of a _host tuple"""
    r = type(h[0])(h[0].var[idx], h[0].ierr[idx], h[0].stats[idx])
    out = (r, np.ascontiguousarray(h[1][idx]))
    if len(h) == 3:
        out += (tuple(None if x is None else np.ascontiguousarray(x[idx]) for x in h[2]),)
    return out


def _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device=False, cap=None, hstart=None, tstart=R.TIN, tend=R.TOUT, sync=True):
    """rosenbrock_cells (cap None) or rosenbrock_trace_cells through the Python surface, host or device entry"""
    conv = _T if device else (lambda x: x)
    args = (mech, conv(V), conv(F), conv(K), tstart, tend, ipar, rpar, conv(atol), conv(rtol))
    hs = None if hstart is None else _T(hstart)
    res = chem.rosenbrock_cells(*args, hstart=hs) if cap is None else chem.rosenbrock_trace_cells(*args, hstart=hs, cap=cap)
    return _host(res) if sync else res


def _shared_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device=False, cap=None, hstart=None, tstart=R.TIN, tend=R.TOUT):
    conv = _T if device else (lambda x: x)
    args = (mech, conv(V), conv(F), conv(K), tstart, tend, ipar, rpar, atol, rtol)
    hs = None if hstart is None else _T(hstart)
    return _host(chem.rosenbrock(*args, hstart=hs) if cap is None else chem.rosenbrock_trace(*args, hstart=hs, cap=cap))


def _rows(pair_vec, n, ntol):
    return np.ascontiguousarray(np.tile(np.asarray(pair_vec, np.float64)[:ntol], (n, 1)))


# ---- 1. shared rows are the shared entry
@pytest.mark.parametrize("mech", MECHS)
def test_c1_shared_rows_are_the_shared_entry(chem, mech):
    """Ros3 at INTEGRATE_x's options, Rodas3 with vector tolerances and Rodas4 at RelTol 1e-5: every row equal to the call's pair gives
    rosenbrock's var, ierr, stats, t_h bit for bit, host and device, at ntol = NVAR and (scalar sets) ntol = 1; the trace likewise, logs included,
    at cap 0 and 256."""
    V, F, K = _cells(mech)
    n, nvar = V.shape
    sets = {"base": R.base_options(mech), "m4_vector_tol": RM.method_set(mech, "m4_vector_tol")[:4], "m5_rtol_1e-5": RM.method_set(mech, "m5_rtol_1e-5")[:4]}
    stats = {}
    for name, (ipar, rpar, atol, rtol) in sets.items():
        for device in (False, True):
            want = _shared_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device)
            assert (want[0].ierr == 1).all(), name
            stats[name] = want[0].stats
            for ntol in ((nvar, 1) if ipar[1] != 0 else (nvar,)):
                got = _cells_call(chem, mech, V, F, K, ipar, rpar, _rows(atol, n, ntol), _rows(rtol, n, ntol), device)
                assert _same(got, want), (name, device, ntol)
    assert not np.array_equal(stats["base"], stats["m5_rtol_1e-5"])
    ipar, rpar, atol, rtol = sets["base"]
    for device in (False, True):
        for cap in (0, 256):
            want = _shared_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device, cap=cap)
            for ntol in (nvar, 1):
                got = _cells_call(chem, mech, V, F, K, ipar, rpar, _rows(atol, n, ntol), _rows(rtol, n, ntol), device, cap=cap)
                assert _same(got, want), ("trace", device, cap, ntol)
            assert np.array_equal(want[2][6], want[0].stats[:, 2])


# ---- 2. every set against the compiled reference
@pytest.mark.parametrize("name", RC.SET_NAMES)
@pytest.mark.parametrize("mech", MECHS)
def test_c2_sets_against_the_compiled_rosenbrock(chem, mech, name):
    """Per set, every cell: IERR and /Statistics/ identical to Rosenbrock_x's called with the cell's row, VAR within CELLTOL_RTOL, exit time and last
    accepted step size within CELLTOL_TH_RTOL; the device entry gives the host entry's bits."""
    V, F, K = _cells(mech)
    z = _fixture(mech)
    ipar, rpar, atol, rtol = RC.celltol_set(mech, name, V)
    res, th = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol)
    d_var = cb.var_diff(res.var, z[name + "_var"])
    d_te, d_he = cb.th_diff(th[:, 0], th[:, 1], z[name + "_rpar"][:, 0], z[name + "_rpar"][:, 1])
    print("%s %s: VAR %.3e (bound %.1e), exit time %.3e, last step size %.3e (bound %.1e), Nstp %s, IERR %s" %
          (mech, name, d_var, cb.CELLTOL_RTOL[mech], d_te, d_he, cb.CELLTOL_TH_RTOL[mech], res.stats[:, 2].tolist(), res.ierr.tolist()))
    assert np.array_equal(res.ierr, z[name + "_ierr"]), (res.ierr, z[name + "_ierr"])
    assert np.array_equal(res.stats, z[name + "_ipar"]), (res.stats, z[name + "_ipar"])
    assert d_var <= cb.CELLTOL_RTOL[mech]
    assert d_te <= cb.CELLTOL_TH_RTOL[mech] and d_he <= cb.CELLTOL_TH_RTOL[mech]
    assert _same(_cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device=True), (res, th))


@pytest.mark.parametrize("mech", MECHS)
def test_c2_trace_on_rows_that_differ(chem, mech):
    """The trace cells entry on the Ros3 sets whose rows differ from cell to cell: results bit-identical to the untraced cells entry; every cell's
    results AND records bit-identical to the shared trace entry run on that cell alone with the cell's row as its pair, host and device; and, on the
    sets tests/ros_trace_bounds.py covers as it is (ros_celltol_bounds.TRACE_RECORD_SETS), the records against ros_trace_py.rosenbrock_trace called
    with the cell's row, within those bounds."""
    import test_gpu_ros_trace as TT
    V, F, K = _cells(mech)
    nvar = V.shape[1]
    g = load_golden(mech)
    for name in ("rel_1e-13", "vector_rows"):
        ipar, rpar, atol, rtol = RC.celltol_set(mech, name, V)
        plain = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol)
        for device in (False, True):
            got = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device, cap=256)
            assert _same(got[:2], plain), (name, device)
            assert (got[2][6] <= 256).all() and (got[2][6] > 0).all()
            for c in range(3):
                one = _shared_call(chem, mech, V[c:c + 1], F[c:c + 1], K[c:c + 1], ipar, rpar, RC.full_row(atol[c], nvar), RC.full_row(rtol[c], nvar), device,
                                   cap=256)
                assert _same(_take(got, [c]), one), (name, device, c)
        if name in cb.TRACE_RECORD_SETS[mech]:
            t, h, err, share, species, code, nt, ctrl = got[2]

            class Rec:
                pass
            rec = Rec()
            rec.n, rec.cap, rec.nt, rec.ierr, rec.stats = 3, 256, nt, got[0].ierr, got[0].stats
            rec.td, rec.ti = np.stack([t, h, err, share], axis=-1), np.stack([species, code], axis=-1)
            TT._against_restatement(mech, rec, RC.traced(mech, g, (name,))[name], label="cells " + name)


# ---- 3. stride faults
@pytest.mark.parametrize("mech", MECHS)
def test_c3_cells_reversed_with_their_rows(chem, mech):
    V, F, K = _cells(mech)
    rev = [2, 1, 0]
    for name in ("rel_1e-13", "vector_rows"):
        ipar, rpar, atol, rtol = RC.celltol_set(mech, name, V)
        for device in (False, True):
            fwd = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device)
            back = _cells_call(chem, mech, V[rev], F[rev], K[rev], ipar, rpar, atol[rev], rtol[rev], device)
            assert _same(back, _take(fwd, rev)), (name, device)


@pytest.mark.parametrize("mech", ("aer", "tot"))
def test_c3_transposed_rows_are_told_apart(chem, mech):
    """vector_rows laid out [NVAR][ncell] is another batch: the results differ from the correct layout's (a test that could not tell would pass
    the permutation test with any constant stride)."""
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = RC.celltol_set(mech, "vector_rows", V)
    right = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol)
    at, rt = np.ascontiguousarray(atol.T).reshape(atol.shape), np.ascontiguousarray(rtol.T).reshape(rtol.shape)
    assert at.tobytes() != atol.tobytes()
    wrong = _cells_call(chem, mech, V, F, K, ipar, rpar, at, rt)
    assert (wrong[0].ierr == 1).all()
    assert not _same(wrong, right) and wrong[0].var.tobytes() != right[0].var.tobytes()
    # and the wrong layout is what the shared entry gives for those very rows, cell by cell: the entry read what it was handed
    for c in range(3):
        one = _shared_call(chem, mech, V[c:c + 1], F[c:c + 1], K[c:c + 1], ipar, rpar, at[c], rt[c])
        assert _same(_take(wrong, [c]), one), c


@pytest.mark.parametrize("mech", ("gas", "aer"))
def test_c3_species_index_of_the_second_species_of_a_lane(chem, mech):
    """gas and aer keep two species per lane.  A row that is 1e-25 but in species NT, NT + 1 and NVAR - 1 (1-based), different in every cell: the
    cells entry equals the shared entry run per cell with that row as its pair, bit for bit; and a zero in one of those entries of one cell's row
    refuses that cell and no other."""
    V, F, K = _cells(mech)
    n, nvar = V.shape
    ipar, rpar, _, _ = R.base_options(mech)
    ipar[1] = 0
    atol, rtol = np.full((n, nvar), 1.0e-25), np.full((n, nvar), 1.0e-3)
    for c in range(n):
        for k, s in enumerate((NT[mech], NT[mech] + 1, nvar - 1)):
            atol[c, s - 1] = 10.0 ** (-6 - k - c) * np.abs(V[c]).max()
            rtol[c, s - 1] = 10.0 ** (-5 + k)
    for device in (False, True):
        got = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device)
        for c in range(n):
            one = _shared_call(chem, mech, V[c:c + 1], F[c:c + 1], K[c:c + 1], ipar, rpar, atol[c], rtol[c], device)
            assert _same(_take(got, [c]), one), (device, c)
    # that each of the three entries IS read, and in its own cell's row (gas runs into FacMax at every step: its results do not show a tolerance):
    # a zero there refuses exactly that cell
    for k, s in enumerate((NT[mech], NT[mech] + 1, nvar - 1)):
        c = k % n
        zero = atol.copy()
        zero[c, s - 1] = 0.0
        assert _cells_call(chem, mech, V, F, K, ipar, rpar, zero, rtol)[0].ierr.tolist() == [-5 if i == c else 1 for i in range(n)], (s, c)


# ---- 4. -5 per cell
def _poison(shape, dtype, base):
    n = int(np.prod(shape))
    return (-(base + np.arange(n))).astype(dtype).reshape(shape)


def _raw_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device, cap):
    """the C entries on poisoned caller arrays of n + 1 rows -> dict of numpy arrays (and their poison)"""
    import torch
    n, nvar = V.shape
    rows = max(cap or 0, 0)
    buf = {"out": _poison((n + 1, nvar), np.float64, 1.5), "ierr": _poison(n + 1, np.int32, 70), "stats": _poison((n + 1, 8), np.int32, 90),
           "th": _poison((n + 1, 2 if device else 3), np.float64, 3.5), "td": _poison((n + 1, rows, 4), np.float64, 1000.25),
           "ti": _poison((n + 1, rows, 2), np.int32, 5), "nt": _poison(n + 1, np.int32, 40), "ct": _poison((n + 1, nvar), np.int32, 7)}
    poison = {k: v.copy() for k, v in buf.items()}
    L = chem.lib()
    ntol = atol.shape[1]
    if device:
        d = {k: _T(v) for k, v in buf.items()}
        ins = [_T(x) for x in (V, F, K, atol, rtol)]
        args = [MID[mech], n, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), R.TIN, R.TOUT, ins[3].data_ptr(), ins[4].data_ptr(), ntol,
                rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip), d["out"].data_ptr(), d["ierr"].data_ptr(), d["stats"].data_ptr(), d["th"].data_ptr(), None,
                C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        if cap is None:
            rc = L.mistra_chem_rosenbrock_cells_device(*args)
        else:
            rc = L.mistra_chem_rosenbrock_trace_cells_device(*args, cap, d["td"].data_ptr() if rows else None, d["ti"].data_ptr() if rows else None,
                                                             d["nt"].data_ptr(), d["ct"].data_ptr())
        assert rc == 0, L.mistra_chem_last_error()
        torch.cuda.synchronize()
        buf = {k: v.cpu().numpy() for k, v in d.items()}
    else:
        args = [MID[mech], n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), R.TIN, R.TOUT, atol.ctypes.data_as(_dp),
                rtol.ctypes.data_as(_dp), ntol, rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip), buf["out"].ctypes.data_as(_dp),
                buf["ierr"].ctypes.data_as(_ip), buf["stats"].ctypes.data_as(_ip), buf["th"].ctypes.data_as(_dp)]
        if cap is None:
            rc = L.mistra_chem_rosenbrock_cells_ex(*args)
        else:
            rc = L.mistra_chem_rosenbrock_trace_cells_ex(*args, cap, buf["td"].ctypes.data_as(_dp) if rows else None,
                                                         buf["ti"].ctypes.data_as(_ip) if rows else None, buf["nt"].ctypes.data_as(_ip),
                                                         buf["ct"].ctypes.data_as(_ip))
        assert rc == 0, L.mistra_chem_last_error()
    return buf, poison


@pytest.mark.parametrize("name", tuple(RC.BAD_CELLS))
@pytest.mark.parametrize("mech", MECHS)
def test_c4_minus_five_is_a_result_per_cell(chem, mech, name):
    """The refused cell: var_out = var_in bit for bit, ierr -5, zeros in stats / t_h, ntrace 0, its log rows and ctrl untouched.  The other cells:
    their bits in a batch without the bad cell.  The row behind the batch: untouched.  Host and device entries, untraced and traced (cap 64)."""
    V, F, K = _cells(mech)
    n = V.shape[0]
    ipar, rpar, atol, rtol = RC.celltol_set(mech, name, V)
    bad = list(RC.BAD_CELLS[name])
    good = [c for c in range(n) if c not in bad]
    alone = _cells_call(chem, mech, V[good], F[good], K[good], ipar, rpar, atol[good], rtol[good], cap=64)
    for device in (False, True):
        for cap in (None, 64):
            b, p = _raw_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device, cap)
            what = (name, device, cap)
            assert b["ierr"][:n].tolist() == [-5 if c in bad else 1 for c in range(n)], what
            for c in bad:
                assert b["out"][c].tobytes() == V[c].tobytes() and not b["stats"][c].any() and not b["th"][c].any(), what
                if cap is not None:
                    assert b["nt"][c] == 0 and np.array_equal(b["td"][c], p["td"][c]) and np.array_equal(b["ti"][c], p["ti"][c]), what
                    assert np.array_equal(b["ct"][c], p["ct"][c]), what
            assert b["out"][good].tobytes() == alone[0].var.tobytes() and np.array_equal(b["stats"][good], alone[0].stats), what
            assert b["th"][good][:, :2].tobytes() == alone[1].tobytes(), what
            if cap is not None:
                assert np.array_equal(b["nt"][good], alone[2][6]) and np.array_equal(b["ct"][good], alone[2][7]), what
                for i, c in enumerate(good):
                    k = min(int(b["nt"][c]), cap)
                    assert b["td"][c, :k, 2].tobytes() == alone[2][2][i, :k].tobytes() and np.array_equal(b["td"][c, k:], p["td"][c, k:]), what
            else:
                for k in ("td", "ti", "nt", "ct"):
                    assert np.array_equal(b[k], p[k]), what
            for k in ("out", "ierr", "stats", "th") + (("td", "ti", "nt", "ct") if cap is not None else ()):
                assert np.array_equal(b[k][n], p[k][n]), (what, k)


def test_c4_refusals_of_the_call_go_before_the_cells(chem):
    """ipar[2] = -1 with a bad row in the batch: every cell is -1, not -5 — Rosenbrock_x's order — and no kernel runs (var_out = var_in, zeros)."""
    mech = "gas"
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = RC.celltol_set(mech, "bad_cell_vector", V)
    ipar[2] = -1
    for device in (False, True):
        for cap in (None, 16):
            b, p = _raw_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device, cap)
            assert (b["ierr"][:3] == -1).all() and b["out"][:3].tobytes() == V.tobytes() and not b["stats"][:3].any() and not b["th"][:3].any()
            if cap is not None:
                assert not b["nt"][:3].any() and np.array_equal(b["td"], p["td"]) and np.array_equal(b["ct"], p["ct"])
            assert np.array_equal(b["out"][3], p["out"][3]) and b["ierr"][3] == p["ierr"][3]


def test_c4_host_tolerance_arrays_are_refused_by_the_device_entry(chem):
    """The device entries hand the tolerance pointers to the kernel: host arrays there fail with a text, nothing is launched, the outputs stay."""
    import torch
    mech = "gas"
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = RC.celltol_set(mech, "rel_1e-13", V)
    dV, dF, dK = _T(V), _T(F), _T(K)
    out, ierr, stats = _T(np.full(V.shape, -7.25)), _T(np.full(3, 77, np.int32)), _T(np.full((3, 8), 77, np.int32))
    L = chem.lib()
    rc = L.mistra_chem_rosenbrock_cells_device(MID[mech], 3, dV.data_ptr(), dF.data_ptr(), dK.data_ptr(), R.TIN, R.TOUT, atol.ctypes.data, rtol.ctypes.data, 1,
                                               rpar.ctypes.data_as(_dp), ipar.ctypes.data_as(_ip), out.data_ptr(), ierr.data_ptr(), stats.data_ptr(), None, None,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"not device arrays" in L.mistra_chem_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.25).all() and (ierr.cpu().numpy() == 77).all() and (stats.cpu().numpy() == 77).all()


# ---- 5. batch edges
def test_c5_batch_sizes_with_the_rows_tiled(chem):
    mech = "gas"
    V, F, K = _cells(mech)
    for name in ("vector_rows", "bad_rtol_cell"):
        ipar, rpar, atol, rtol = RC.celltol_set(mech, name, V)
        three = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol)
        for n in (1, 3, 65):
            idx = np.arange(n) % 3
            for device in (False, True):
                got = _cells_call(chem, mech, V[idx], F[idx], K[idx], ipar, rpar, atol[idx], rtol[idx], device)
                assert _same(got, _take(three, idx)), (name, n, device)


def test_c5_two_device_slots_with_a_ragged_split(chem):
    """init_devices([0, 0]), five tot cells whose rows all differ: the batch is split 3 + 2, each block with its own rows — the bits of one device."""
    mech = "tot"
    g = load_golden(mech)
    V, F, K = g["var_in"][:5], g["fix"][:5], g["rconst"][:5]
    ipar, rpar, _, _ = R.base_options(mech)
    atol = np.ascontiguousarray((10.0 ** -np.arange(10.0, 15.0) * RC.cell_max(V)).reshape(5, 1))
    rtol = np.ascontiguousarray(np.array([1e-3, 2e-3, 1e-4, 5e-3, 1e-2]).reshape(5, 1))
    one = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol)
    one_tr = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, cap=32)
    assert (one[0].ierr == 1).all()
    shifted = _cells_call(chem, mech, V[3:], F[3:], K[3:], ipar, rpar, atol[:2], rtol[:2])      # what a block that kept row 0's offset would compute
    assert not np.array_equal(shifted[0].stats, one[0].stats[3:]), "rows 3, 4 and rows 0, 1 give these cells the same counters: the test cannot see the offset"
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    assert _same(_cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol), one), "the split over two slots differs from one device"
    assert _same(_cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, cap=32), one_tr)


def test_c5_per_cell_first_step_with_per_cell_rows(chem):
    mech = "aer"
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = RC.celltol_set(mech, "rel_1e-13", V)
    plain = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device=True)
    assert _same(_cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device=True, hstart=np.array([0.0, -1.0, 0.0])), plain)
    got = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol, device=True, hstart=np.array([0.0, 0.5, -3.0]))
    rp05 = rpar.copy()
    rp05[2] = 0.5
    all05 = _cells_call(chem, mech, V, F, K, ipar, rp05, atol, rtol, device=True)
    assert not _same(_take(all05, [1]), _take(plain, [1]))
    assert _same(_take(got, [0, 2]), _take(plain, [0, 2])) and _same(_take(got, [1]), _take(all05, [1]))


def test_c5_two_calls_queued_with_different_device_rows(chem):
    import torch
    mech = "tot"
    V, F, K = _cells(mech)
    a = RC.celltol_set(mech, "rel_1e-13", V)
    b = RC.celltol_set(mech, "rel_1e-10_ntolN", V)
    want = [_cells_call(chem, mech, V, F, K, *s, device=True) for s in (a, b)]
    assert not _same(want[0], want[1])
    torch.cuda.synchronize()
    queued = [_cells_call(chem, mech, V, F, K, *s, device=True, sync=False) for s in (a, b, a)]
    for q, w in zip(queued, (want[0], want[1], want[0])):
        assert _same(_host(q), w)


# ---- 6. cell_atol on the device
@pytest.mark.parametrize("mech", MECHS)
def test_c6_cell_atol_device_equals_the_host_formula(chem, mech):
    import torch
    nvar = chem.DIMS[mech][0]
    L = chem.lib()
    for ncell in (1, 63, 64, 65, 257):
        v = RC.atol_edge_rows(nvar, ncell, seed=ncell)
        for factor, floor in ((1.0e-13, 1.0e-30), (0.3, 1.0e-3)):
            out = _T(np.full(ncell + 1, -7.25))
            dv = _T(v)
            rc = L.mistra_chem_cell_atol_device(MID[mech], ncell, dv.data_ptr(), factor, floor, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, L.mistra_chem_last_error()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            with np.errstate(invalid="ignore"):
                want = np.array([max(floor, factor * np.fmax.reduce(np.abs(row))) for row in v])
            assert got[:ncell].tobytes() == want.tobytes(), (ncell, factor, np.nonzero(got[:ncell] != want)[0][:5])
            assert got[ncell] == -7.25
            assert chem.cell_atol(mech, v, factor, floor).tobytes() == want.tobytes()
    assert _np(chem.cell_atol(mech, _T(v), 1.0e-13, 1.0e-30)).tobytes() == chem.cell_atol(mech, v, 1.0e-13, 1.0e-30).tobytes()


@pytest.mark.parametrize("mech", MECHS)
def test_c6_cell_atol_feeds_the_cells_entry_on_the_device(chem, mech):
    V, F, K = _cells(mech)
    ipar, rpar, _, _ = R.base_options(mech)
    rtol = np.full((3, 1), 1.0e-3)
    host = _cells_call(chem, mech, V, F, K, ipar, rpar, chem.cell_atol(mech, V, 1.0e-13, 1.0e-300), rtol)
    dV = _T(V)
    got = _host(chem.rosenbrock_cells(mech, dV, _T(F), _T(K), R.TIN, R.TOUT, ipar, rpar, chem.cell_atol(mech, dV, 1.0e-13, 1.0e-300), _T(rtol)))
    assert _same(got, host)
    assert _same(host, _cells_call(chem, mech, V, F, K, *RC.celltol_set(mech, "rel_1e-13", V)))


# ---- 7. a user slot
def test_c7_user_slot(chem):
    import user_mech_cases as uc
    uc.ensure_tables()
    name = "demo_g"
    V, F, K = uc.batch(name, load_golden(uc.DEMOS[name][0]), 3)
    n, nvar = V.shape
    ipar, rpar, _, _ = R.base_options("gas")
    atol, rtol = np.full(nvar, 1.0e-25), np.full(nvar, 1.0e-3)
    try:
        for device in (False, True):
            want = _shared_call(chem, name, V, F, K, ipar, rpar, atol, rtol, device)
            for ntol in (nvar, 1):
                assert _same(_cells_call(chem, name, V, F, K, ipar, rpar, _rows(atol, n, ntol), _rows(rtol, n, ntol), device), want), (device, ntol)
            a = (1.0e-13 * RC.cell_max(V)).reshape(n, 1)
            r = np.full((n, 1), 1.0e-3)
            got = _cells_call(chem, name, V, F, K, ipar, rpar, a, r, device)
            assert (got[0].ierr == 1).all()
            for c in range(n):
                one = _shared_call(chem, name, V[c:c + 1], F[c:c + 1], K[c:c + 1], ipar, rpar, np.full(nvar, a[c, 0]), rtol, device)
                assert _same(_take(got, [c]), one), (device, c)
            if device:
                assert _np(chem.cell_atol(name, _T(V), 1.0e-13, 1.0e-300)).tobytes() == a.tobytes()
    finally:
        chem.clear_options(name)


# ---- 8. from Fortran
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_c8_from_fortran(chem, tmp_path):
    """shim/shim_driver YG: ROSENBROCK_BATCH_CELLS_g on bad_cell_vector — ISTAT and IERR identical to the Python entry, VAR, Texit, Hexit its bits, the
    refused cell's message on unit 6."""
    mech, name = "gas", "bad_cell_vector"
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    V, F, K = _cells(mech)
    n, nvar = V.shape
    ipar, rpar, atol, rtol = RC.celltol_set(mech, name, V)
    want, th = _cells_call(chem, mech, V, F, K, ipar, rpar, atol, rtol)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.concatenate([ipar.astype(np.float64), rpar, [R.TIN, R.TOUT, float(n), float(atol.shape[1])]]).tofile(f)
        for i in range(n):
            np.concatenate([V[i], F[i], K[i], atol[i], rtol[i]]).tofile(f)
    r = subprocess.run([DRIVER, "YG", str(fin), str(fout)], check=True, timeout=300, capture_output=True, text=True)
    raw = np.fromfile(fout, np.float64)
    out = raw[:n * (nvar + 2)].reshape(n, nvar + 2)
    tail = raw[n * (nvar + 2):].reshape(n, 9)
    assert np.array_equal(tail[:, 0].astype(np.int32), want.ierr) and tail[:, 0].tolist() == [1.0, -5.0, 1.0]
    assert np.array_equal(tail[:, 1:].astype(np.int32), want.stats)
    assert out[:, :nvar].tobytes() == want.var.tobytes() and out[:, nvar:].tobytes() == th.tobytes()
    assert r.stdout.count("Forced exit from Rosenbrock_g") == 1 and "Improper tolerance values" in r.stdout
