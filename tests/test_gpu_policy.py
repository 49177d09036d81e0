"""The integrator policy on the GPU (-m gpu; include/mistra_chem.h: mistra_chem_set_policy, OPT-IN and not the reference's behaviour): a method of
Rosenbrock_x's five and / or a cell-relative AbsTol for the entries that carry no options of their own — the integrate family, the COMMON-block entry and
the column driver.

Everything is held bit for bit to a composition of entries that are pinned to the compiled reference elsewhere (tests/test_gpu_ros_methods.py,
tests/test_gpu_ros_celltol.py): the yardstick of a policy (method, factor, floor) is the same cells through mistra_chem_cell_atol_device and then
mistra_chem_rosenbrock_cells_device (mistra_chem_rosenbrock_device when factor = 0) with ipar[3] = method and the options in force spelt out —
INTEGRATE_x's where none are.  No tolerance is introduced here.

Cells: 0, n/2, n-1 of tests/golden/integrate_<mech>.npz, tiled where a count is named.  Columns: tests/golden/drivecol_base1.npz (gas, aer),
drivecol_BTZ96.npz (tot), through the helpers of tests/test_gpu_step_reuse.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ros_options_py as R
import test_gpu_step_reuse as SR
from conftest import MECHS, REPO, load_golden

pytestmark = pytest.mark.gpu
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MID = {"gas": 0, "aer": 1, "tot": 2}
NT = {"gas": 64, "aer": 256, "tot": 512}      # threads per cell: species s sits in thread s % NT, register s // NT
FACTOR, FLOOR = 1.0e-13, 1.0e-25
POLICY = (4, FACTOR, FLOOR)                   # Rodas3 with the cell-relative AbsTol of INTEGRATION.md §4k
DRIVER = os.path.join(REPO, "shim", "shim_driver")
N, DT, KEYS = SR.N, SR.DT, SR.KEYS


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)

    def reset():
        if c.device_count() != 1:      # whatever a test initialised: the other modules' fixtures start from init(0)
            c.finalize()
            c.init(0)
        for mech in list(MECHS) + c.user_mechs():
            c.clear_policy(mech)
            c.clear_options(mech)
        for mech in MECHS:
            c.set_step_reuse(mech, False)
    reset()
    yield c
    reset()


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


_GOLDEN = {}


def _cells(mech, n=3):
    if mech not in _GOLDEN:
        g = load_golden(mech)
        c = list(R.cells_of(g["var_in"].shape[0]))
        _GOLDEN[mech] = tuple(np.ascontiguousarray(g[k][c]) for k in ("var_in", "fix", "rconst"))
    idx = np.arange(n) % 3
    return tuple(np.ascontiguousarray(a[idx]) for a in _GOLDEN[mech])


def _yardstick(chem, mech, V, F, K, policy, opts=None, tin=R.TIN, tout=R.TOUT, hstart=None):
    """cell_atol -> rosenbrock_cells on the device (rosenbrock where factor = 0) with ipar[3] = method and the options spelt out -> dict of numpy arrays.
    V, F, K: numpy arrays or tensors on the GPU."""
    import torch
    method, factor, floor = policy
    ipar, rpar, atol, rtol = opts if opts is not None else R.base_options("gas" if mech not in MECHS else mech)
    ipar = np.array(ipar, np.int32)
    ipar[3] = method
    dV, dF, dK = [x if isinstance(x, torch.Tensor) else _T(x) for x in (V, F, K)]
    n, nvar = dV.shape
    hs = None if hstart is None else _T(hstart)
    if not factor:
        res, th = chem.rosenbrock(mech, dV, dF, dK, tin, tout, ipar, rpar, np.asarray(atol)[:nvar], np.asarray(rtol)[:nvar], hstart=hs)
    else:
        a = chem.cell_atol(mech, dV, factor, floor)
        if ipar[1] == 0:      # vector options: rows of NVAR
            a = a.expand(n, nvar).contiguous()
            r = _T(np.tile(np.asarray(rtol, np.float64)[:nvar], (n, 1)))
        else:                 # scalar options: ntol = 1
            r = _T(np.full((n, 1), float(np.asarray(rtol).ravel()[0])))
        res, th = chem.rosenbrock_cells(mech, dV, dF, dK, tin, tout, ipar, rpar, a, r, hstart=hs)
    torch.cuda.synchronize()
    return dict(var=_np(res.var), ierr=_np(res.ierr), stats=_np(res.stats), th=_np(th))


def _poison(shape, dtype, base):
    n = int(np.prod(shape))
    return (-(base + np.arange(n))).astype(dtype).reshape(shape)


def _integrate_device(chem, mech, V, F, K, tin=R.TIN, tout=R.TOUT, hstart=None):
    """mistra_chem_integrate_device(_hstart) on the caller's arrays, one row more than the call, every entry poisoned -> (dict of the call's rows, ok):
    ok = the row behind the call kept its poison"""
    import torch
    n, nvar = V.shape
    buf = {"var": _poison((n + 1, nvar), np.float64, 1.5), "ierr": _poison(n + 1, np.int32, 70), "stats": _poison((n + 1, 8), np.int32, 90),
           "th": _poison((n + 1, 2), np.float64, 3.5)}
    d = {k: _T(v) for k, v in buf.items()}
    ins = [_T(x) for x in (V, F, K)]
    hs = None if hstart is None else _T(hstart)
    L = chem.lib()
    rc = L.mistra_chem_integrate_device_hstart(chem._mech_id(mech)[0], n, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), tin, tout, d["var"].data_ptr(),
                                               d["ierr"].data_ptr(), d["stats"].data_ptr(), d["th"].data_ptr(), None if hs is None else hs.data_ptr(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.mistra_chem_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    ok = all(got[k][n].tobytes() == buf[k][n].tobytes() for k in buf)
    return {k: v[:n] for k, v in got.items()}, ok


def _integrate_ex(chem, mech, V, F, K, **kw):
    res, th = chem.integrate_ex(mech, V, F, K, R.TIN, R.TOUT, **kw)
    return dict(var=res.var, ierr=res.ierr, stats=res.stats, th=np.ascontiguousarray(th[:, :2]))


def _same(a, b):
    """two result dicts, every bit (a NaN equals itself): VAR, IERR, all eight counters, Texit, Hexit"""
    return a["var"].tobytes() == b["var"].tobytes() and np.array_equal(a["ierr"], b["ierr"]) and np.array_equal(a["stats"], b["stats"]) and \
        a["th"].tobytes() == b["th"].tobytes()


# ---- 1. off is off
@pytest.mark.parametrize("mech", MECHS)
def test_p1_off_is_off(chem, mech):
    """No policy, and set_policy followed by clear_policy: integrate_ex is what it was before any policy call; debug_first_step is the Ros3 diagnostic with
    a policy set or not."""
    V, F, K = _cells(mech)
    assert chem.get_policy(mech) is None
    before = _integrate_ex(chem, mech, V, F, K)
    dump0 = chem.debug_first_step(mech, V, F, K)
    chem.set_policy(mech, *POLICY)
    assert chem.get_policy(mech) == chem.Policy(*POLICY)
    under = _integrate_ex(chem, mech, V, F, K)
    dump1 = chem.debug_first_step(mech, V, F, K)      # (not refused: no options are set)
    for x, y in zip(dump0, dump1):
        assert x.tobytes() == y.tobytes(), "the first-step dump differs with a policy set"
    chem.clear_policy(mech)
    assert chem.get_policy(mech) is None
    assert _same(_integrate_ex(chem, mech, V, F, K), before)
    assert not _same(under, before), "the policy changed nothing: the test cannot tell set from cleared"


def test_p1_off_is_off_in_the_column_driver(chem):
    g = SR._load("base1")
    SR._maps(chem, g)
    ks = SR.Column(g).layers("gas")[:8]

    def step():
        col = SR.Column(g)
        return SR._host_step(chem, col, "gas", ks, 0), col
    host0, col0 = step()
    chem.set_policy("gas", *POLICY)
    chem.clear_policy("gas")
    host1, col1 = step()
    for key in KEYS:
        assert col0.a[key].tobytes() == col1.a[key].tobytes(), key
    for x, y in zip(host0, host1):
        assert x.tobytes() == y.tobytes()


# ---- 2. the base options block
@pytest.mark.parametrize("mech", MECHS)
def test_p2_ros3_without_a_factor_is_no_policy(chem, mech):
    V, F, K = _cells(mech)
    plain_h = _integrate_ex(chem, mech, V, F, K)
    plain_d, _ = _integrate_device(chem, mech, V, F, K)
    chem.set_policy(mech, 2)
    assert chem.get_policy(mech) == chem.Policy(2, 0.0, 0.0)
    assert _same(_integrate_ex(chem, mech, V, F, K), plain_h)
    got, ok = _integrate_device(chem, mech, V, F, K)
    assert ok and _same(got, plain_d) and _same(got, plain_h)


# ---- 3. every method, with and without the cell-relative AbsTol
@pytest.mark.parametrize("factor", (0.0, FACTOR))
@pytest.mark.parametrize("method", (1, 3, 4, 5))
@pytest.mark.parametrize("mech", MECHS)
def test_p3_methods_through_integrate_device(chem, mech, method, factor):
    policy = (method, factor, FLOOR)
    chem.set_policy(mech, *policy)
    want3 = None
    for n in (1, 3, 65):      # 65: the workgroup behind a full group of cell_atol_kernel's four waves
        V, F, K = _cells(mech, n)
        got, ok = _integrate_device(chem, mech, V, F, K)
        want = _yardstick(chem, mech, V, F, K, policy)
        assert ok, "the row behind the call was written"
        assert _same(got, want), (n, got["stats"][:3, 2].tolist(), want["stats"][:3, 2].tolist())
        if n == 3:
            want3 = want
            assert (got["ierr"] == 1).all()
            assert _same(_integrate_ex(chem, mech, V, F, K), want), "integrate_ex"
            hs = np.array([0.0, 0.5, -1.0])      # a first step size per cell goes before Hstart, with a policy as without
            want_h = _yardstick(chem, mech, V, F, K, policy, hstart=hs)
            assert not _same(want_h, want)
            assert _same(_integrate_ex(chem, mech, V, F, K, hstart=hs), want_h), "integrate_hstart_ex"
            assert _same(_integrate_device(chem, mech, V, F, K, hstart=hs)[0], want_h), "integrate_device_hstart"
    assert _same({k: v[64:65] for k, v in got.items()}, {k: v[1:2] for k, v in want3.items()}), "cell 64 of the tiled batch is cell 1"


# ---- 4. the maximum formed in the kernel
def _max_cells(mech):
    """one cell per case -> (V, F, K, names)"""
    V3, F3, K3 = _cells(mech)
    nvar = V3.shape[1]
    base = V3[1]
    big = 16.0 * np.abs(base).max()
    rows, names = [], []
    for s in sorted({0, 63, 64, NT[mech] - 1, NT[mech], nvar - 1}):
        if s < nvar:
            v = base.copy()
            v[s] = big
            rows.append(v)
            names.append("largest in species %d" % s)
    v = base.copy()
    v[nvar // 2] = -big
    rows.append(v)
    names.append("largest entry negative")
    v = base.copy()
    v[5] = np.nan
    rows.append(v)
    names.append("a NaN in one species")
    rows.append(np.zeros(nvar))
    names.append("all zeros")
    n = len(rows)
    return np.ascontiguousarray(rows), np.ascontiguousarray(np.tile(F3[1], (n, 1))), np.ascontiguousarray(np.tile(K3[1], (n, 1))), names


@pytest.mark.parametrize("mech", MECHS)
def test_p4_the_in_kernel_maximum(chem, mech):
    """The cell's largest |VAR| held in turn by the first and last species of a lane's first register, by the second register's first species (gas, aer:
    species NT) and by the last species; negative; beside a NaN; a cell of zeros (AbsTol = floor) — each against the yardstick, whatever that returns.
    AbsTol is read off the results: the same cells under factors a decade apart differ."""
    V, F, K, names = _max_cells(mech)
    atol = chem.cell_atol(mech, V, FACTOR, FLOOR).ravel()
    assert atol[-1] == FLOOR and np.all(atol[:len(names) - 3] == FACTOR * 16.0 * np.abs(_cells(mech)[0][1]).max())
    for method in (2, 4):
        policy = (method, FACTOR, FLOOR)
        chem.set_policy(mech, *policy)
        got, ok = _integrate_device(chem, mech, V, F, K)
        want = _yardstick(chem, mech, V, F, K, policy)
        for c, name in enumerate(names):
            assert _same({k: v[c:c + 1] for k, v in got.items()}, {k: v[c:c + 1] for k, v in want.items()}), (method, name)
        assert ok
        assert _same(_integrate_ex(chem, mech, V, F, K), want), (method, "integrate_ex")
        if method == 2:
            ros3 = got
    # the factor reaches the integrator: a far larger one gives other steps (gas runs into FacMax at every step, its counters do not show a tolerance)
    chem.set_policy(mech, 2, 1.0e-3, FLOOR)
    other, _ = _integrate_device(chem, mech, V, F, K)
    assert _same(other, _yardstick(chem, mech, V, F, K, (2, 1.0e-3, FLOOR)))
    assert mech == "gas" or not np.array_equal(other["stats"], ros3["stats"])
    # factor * max below the floor
    floor = 1.0e3 * FACTOR * 16.0 * np.abs(_cells(mech)[0][1]).max()
    policy = (2, FACTOR, floor)
    assert np.all(chem.cell_atol(mech, V, FACTOR, floor) == floor)
    chem.set_policy(mech, *policy)
    got, ok = _integrate_device(chem, mech, V, F, K)
    assert ok and _same(got, _yardstick(chem, mech, V, F, K, policy))


# ---- 5. with options in force
@pytest.mark.parametrize("mech", MECHS)
def test_p5_with_options_in_force(chem, mech):
    """Vector RelTol, FacMax 3 and Hstart 0.05 from mistra_chem_set_options, the method and AbsTol from the policy; neither setting touches the other."""
    V, F, K = _cells(mech)
    ipar, rpar, atol, rtol = R.option_set(mech, "vector_tol")
    rpar[2], rpar[4] = 0.05, 3.0
    chem.set_policy(mech, *POLICY)
    chem.set_options(mech, ipar, rpar, atol, rtol)
    assert chem.get_policy(mech) == chem.Policy(*POLICY), "set_options changed the policy"
    o = chem.get_options(mech)
    assert np.array_equal(o.ipar, ipar) and o.ipar[3] == 2 and np.array_equal(o.rpar, rpar) and np.array_equal(o.atol, atol) and np.array_equal(o.rtol, rtol)
    want = _yardstick(chem, mech, V, F, K, POLICY, (ipar, rpar, atol, rtol))
    got, ok = _integrate_device(chem, mech, V, F, K)
    assert ok and _same(got, want)
    assert _same(_integrate_ex(chem, mech, V, F, K), want)
    assert not _same(want, _yardstick(chem, mech, V, F, K, POLICY)), "the options changed nothing: the test cannot see them"
    # the options alone, then the policy again over them: get_options is the same throughout
    chem.clear_policy(mech)
    o2 = chem.get_options(mech)
    assert all(np.array_equal(x, y) for x, y in zip(o, o2))
    only_options = _integrate_ex(chem, mech, V, F, K)
    assert _same(only_options, _yardstick(chem, mech, V, F, K, (2, 0.0, 0.0), (ipar, rpar, atol, rtol)))
    chem.set_policy(mech, 5, 0.0)
    assert _same(_integrate_ex(chem, mech, V, F, K), _yardstick(chem, mech, V, F, K, (5, 0.0, 0.0), (ipar, rpar, atol, rtol)))
    chem.clear_options(mech)
    assert chem.get_options(mech) is None and chem.get_policy(mech) == chem.Policy(5, 0.0, 0.0), "clear_options changed the policy"
    assert _same(_integrate_ex(chem, mech, V, F, K), _yardstick(chem, mech, V, F, K, (5, 0.0, 0.0)))


def test_p5_common_block_entry(chem):
    """mistra_chem_integrate_common_status under a policy: the cell's result is the yardstick's, ATOL / RTOL in the COMMON block stay the options' values."""
    mech = "tot"
    V, F, K = _cells(mech)
    nv, nf, nr = V.shape[1], F.shape[1], K.shape[1]
    chem.set_policy(mech, *POLICY)
    want = _yardstick(chem, mech, V[:1], F[:1], K[:1], POLICY)
    gdata = np.zeros(nv + nf + nr + 2 + 2 * nv + 8)
    gdata[:nv], gdata[nv:nv + nf], gdata[nv + nf:nv + nf + nr] = V[0], F[0], K[0]
    tin, tout, ierr, nsng, te, he = C.c_double(R.TIN), C.c_double(R.TOUT), C.c_int32(0), C.c_int32(0), C.c_double(0), C.c_double(0)
    L = chem.lib()
    rc = L.mistra_chem_integrate_common_status(MID[mech], gdata.ctypes.data_as(C.c_void_p), C.byref(tin), C.byref(tout), C.byref(ierr), C.byref(te), C.byref(he),
                                               C.byref(nsng))
    assert rc == 0, L.mistra_chem_last_error()
    o = nv + nf + nr + 2
    assert gdata[:nv].tobytes() == want["var"][0].tobytes() and ierr.value == want["ierr"][0]
    assert tin.value == want["th"][0, 0] and gdata[o + 2 * nv] == want["th"][0, 1]
    assert (gdata[o:o + nv] == 1.0e-25).all() and (gdata[o + nv:o + 2 * nv] == 1.0e-3).all(), "ATOL / RTOL of the COMMON block are the options', not the cell's"


# ---- 6. the host batch over two device slots
def test_p6_two_device_slots_with_a_ragged_split(chem):
    mech = "tot"
    g = load_golden(mech)
    V, F, K = (np.ascontiguousarray(g[k][:5]) for k in ("var_in", "fix", "rconst"))
    V = V * np.array([1.0, 3.0, 0.5, 7.0, 0.25]).reshape(5, 1)      # five maxima
    chem.set_policy(mech, *POLICY)
    one = _integrate_ex(chem, mech, V, F, K)
    assert _same(one, _yardstick(chem, mech, V, F, K, POLICY))
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    assert chem.get_policy(mech) is None, "finalize drops a policy the environment did not ask for"
    plain = _integrate_ex(chem, mech, V, F, K)
    chem.set_policy(mech, *POLICY)
    assert _same(_integrate_ex(chem, mech, V, F, K), one), "the split over two slots differs from one device"
    assert not _same(plain, one)


# ---- 7. the column driver
def _chain(chem, col, mech, ks, step, policy, hstart=None):
    """the column step from the public device-resident pieces on copies of col's rows: pack -> rates_env_from_c -> update_rconst -> cell_atol ->
    rosenbrock_cells -> budgets -> unpack (tests/test_gpu_step_reuse.py: _chain_step, with the yardstick as its integrator)"""
    import torch
    dev = torch.device("cuda", 0)
    kk = np.asarray(ks, np.int64) - 1
    nl = len(kk)
    scal, env = col.inputs(mech, ks)
    d = {key: _T(col.a[key][kk]) for key in KEYS}
    var = torch.zeros((nl, SR.NVAR[mech]), dtype=torch.float64, device=dev)
    fix = torch.zeros((nl, SR.NFIX[mech]), dtype=torch.float64, device=dev)
    chem.pack(mech, d["s1"], d["s3"], d["sl1"], d["sion1"], _T(scal), var, fix)
    envd = _T(env)
    chem.rates_env_from_c(mech, var, fix, envd)
    rct = chem.update_rconst(mech, envd)
    y = _yardstick(chem, mech, var, fix, rct, policy, None, DT * step, DT * step + DT, hstart)
    var = _T(y["var"])
    chem.budgets(mech, var, fix, rct, DT, None, d["bgs"])
    chem.unpack(mech, var, d["s1"], d["s3"], d["sl1"], d["sion1"])
    torch.cuda.synchronize()
    out = {key: d[key].cpu().numpy() for key in KEYS}
    out.update(ierr=y["ierr"], stats=y["stats"], th=y["th"])
    return out


def _device_step(chem, col, mech, ks, step):
    """the same step through mistra_chem_drive_device on copies of col's rows"""
    import torch
    dev = torch.device("cuda", 0)
    kk = np.asarray(ks, np.int64) - 1
    nl = len(kk)
    scal, env = col.inputs(mech, ks)
    d = {key: _T(col.a[key][kk]) for key in KEYS}
    var = torch.zeros((nl, SR.NVAR[mech]), dtype=torch.float64, device=dev)
    fix = torch.zeros((nl, SR.NFIX[mech]), dtype=torch.float64, device=dev)
    ierr = torch.empty(nl, dtype=torch.int32, device=dev)
    stats = torch.empty((nl, 8), dtype=torch.int32, device=dev)
    th = torch.empty((nl, 2), dtype=torch.float64, device=dev)
    chem.drive(mech, d["s1"], d["s3"], d["sl1"], d["sion1"], _T(scal), _T(env), var, fix, DT * step, DT, ierr, stats, th, None, d["bgs"])
    torch.cuda.synchronize()
    out = {key: d[key].cpu().numpy() for key in KEYS}
    out.update(ierr=ierr.cpu().numpy(), stats=stats.cpu().numpy(), th=th.cpu().numpy())
    return out


def _column(mech):
    g = SR._load("BTZ96" if mech == "tot" else "base1")
    return g, SR.Column(g).layers(mech)


@pytest.mark.parametrize("mech", MECHS)
def test_p7_column_driver(chem, mech):
    """mistra_chem_drive and mistra_chem_drive_device under policy (Rodas3, 1e-13, 1e-25) against the explicit chain: the model arrays out, bgs, ierr,
    stats, t_h.  gas, aer: 8 layers, then 1, then 8 others (the arena still holds the first batch); tot: 2 layers."""
    g, ks = _column(mech)
    SR._maps(chem, g)
    batches = [ks[:2]] if mech == "tot" else [ks[:8], ks[8:9], ks[9:17]]
    assert all(len(b) for b in batches) and len(batches[-1]) == (2 if mech == "tot" else 8)
    col = SR.Column(g)
    plain = SR._host_step(chem, col.copy(), mech, batches[0], 0)
    chem.set_policy(mech, *POLICY)
    for b in batches:
        chain = _chain(chem, col, mech, b, 0, POLICY)
        dev = _device_step(chem, col, mech, b, 0)
        for key in KEYS + ("ierr", "stats", "th"):
            assert dev[key].tobytes() == chain[key].tobytes(), "mistra_chem_drive_device, %d layers: %s" % (len(b), key)
        host = SR._host_step(chem, col, mech, b, 0)
        SR._assert_same(col, b, host, chain, "mistra_chem_drive, %d layers" % len(b))
        assert (host[0] == 1).all()
        if b is batches[0]:
            assert not np.array_equal(host[1], plain[1]), "the policy changed no counter: the test cannot tell it from none"


def test_p7_column_driver_budget_levels(chem):
    """bg of COMMON /budg/ under a policy: three of eight gas layers are budget levels; their rows of bg are the explicit chain's (budgets on the state
    the yardstick left), every other row of bg stays as it was.  mistra_chem_drive and mistra_chem_drive_device."""
    import torch
    mech = "gas"
    g, ks = _column(mech)
    SR._maps(chem, g)
    ks = ks[:8]
    kk = np.asarray(ks, np.int64) - 1
    nl, nr = len(ks), 331
    level = np.array([2, 0, 0, 5, 0, 0, 0, 1], np.int32)      # kl (1-based) where the layer is a budget level, else 0
    lev = level > 0
    bg0 = 0.25 + np.arange(SR.NLEV * SR.NRXN * 2, dtype=np.float64).reshape(SR.NLEV, SR.NRXN, 2) / 1024.0
    chem.set_policy(mech, *POLICY)
    col = SR.Column(g)
    scal, env = col.inputs(mech, ks)
    # the chain: as _chain, with bg rows per cell
    d = {key: _T(col.a[key][kk]) for key in KEYS}
    dev = torch.device("cuda", 0)
    var = torch.zeros((nl, SR.NVAR[mech]), dtype=torch.float64, device=dev)
    fix = torch.zeros((nl, SR.NFIX[mech]), dtype=torch.float64, device=dev)
    chem.pack(mech, d["s1"], d["s3"], d["sl1"], d["sion1"], _T(scal), var, fix)
    envd = _T(env)
    chem.rates_env_from_c(mech, var, fix, envd)
    rct = chem.update_rconst(mech, envd)
    y = _yardstick(chem, mech, var, fix, rct, POLICY, None, 0.0, DT)
    rows = np.ascontiguousarray(bg0[np.where(lev, level - 1, 0), :nr])      # [nl, nr, 2]; the rows of layers that are no level are not compared
    bgc = _T(rows)
    chem.budgets(mech, _T(y["var"]), fix, rct, DT, bgc, d["bgs"])
    torch.cuda.synchronize()
    want_bg, want_bgs = bgc.cpu().numpy()[lev], d["bgs"].cpu().numpy()
    assert not np.array_equal(want_bg, rows[lev])
    # mistra_chem_drive_device: bg per layer of the batch
    d2 = {key: _T(col.a[key][kk]) for key in KEYS}
    var2, fix2, bg2 = torch.zeros_like(var), torch.zeros_like(fix), _T(rows)
    ierr = torch.empty(nl, dtype=torch.int32, device=dev)
    stats = torch.empty((nl, 8), dtype=torch.int32, device=dev)
    chem.drive(mech, d2["s1"], d2["s3"], d2["sl1"], d2["sion1"], _T(scal), _T(env), var2, fix2, 0.0, DT, ierr, stats, None, bg2, d2["bgs"])
    torch.cuda.synchronize()
    assert bg2.cpu().numpy()[lev].tobytes() == want_bg.tobytes() and d2["bgs"].cpu().numpy().tobytes() == want_bgs.tobytes(), "mistra_chem_drive_device"
    assert np.array_equal(stats.cpu().numpy(), y["stats"])
    # mistra_chem_drive: bg by level
    bg = bg0.copy()
    a = col.a
    host = chem.drive_host(mech, np.asarray(ks, np.int32), a["s1"], a["s3"], a["sl1"], a["sion1"], scal, env, 0.0, DT, bg=bg, bg_level=level, bgs=a["bgs"])
    assert np.array_equal(host[1], y["stats"]) and (host[0] == 1).all()
    assert bg[level[lev] - 1, :nr].tobytes() == want_bg.tobytes(), "mistra_chem_drive: bg rows of the budget levels"
    assert a["bgs"][kk].tobytes() == want_bgs.tobytes()
    untouched = bg0.copy()
    untouched[level[lev] - 1, :nr] = bg[level[lev] - 1, :nr]
    assert bg.tobytes() == untouched.tobytes(), "bg outside the levels' rows was written"


def test_p7_two_mechanisms_side_by_side_keep_their_policies(chem):
    g = SR._load("base1")
    SR._maps(chem, g)
    col = SR.Column(g)
    kg, ka = col.layers("gas")[:8], col.layers("aer")[:8]
    pol = {"gas": (5, 0.0, 0.0), "aer": (2, FACTOR, FLOOR)}
    for mech, p in pol.items():
        chem.set_policy(mech, *p)
    chains = {"gas": _chain(chem, col, "gas", kg, 0, pol["gas"]), "aer": _chain(chem, col, "aer", ka, 0, pol["aer"])}
    hg = SR._host_step(chem, col, "gas", kg, 0, begin_only=True)
    ha = SR._host_step(chem, col, "aer", ka, 0, begin_only=True)
    chem.drive_host_end("aer")
    chem.drive_host_end("gas")
    SR._assert_same(col, kg, hg[:3], chains["gas"], "gas beside aer")
    SR._assert_same(col, ka, ha[:3], chains["aer"], "aer beside gas")


# ---- 8. step reuse with a policy
def test_p8_step_reuse_with_a_policy(chem):
    g = SR._load("base1")
    SR._maps(chem, g)
    mech = "gas"
    ks = SR.Column(g).layers(mech)[:8]
    kk = np.asarray(ks, np.int64) - 1
    chem.set_step_reuse(mech, True)
    chem.set_policy(mech, *POLICY)
    assert not chem.get_step_memory(mech, N).any()
    col = SR.Column(g)
    for step in range(2):
        hstart = chem.get_step_memory(mech, N)[kk]
        assert (hstart > 0).all() if step else not hstart.any()
        chain = _chain(chem, col, mech, ks, step, POLICY, hstart)
        host = SR._host_step(chem, col, mech, ks, step)
        SR._assert_same(col, ks, host, chain, "step %d under reuse and policy" % step)
        want = np.zeros(N)
        want[kk[host[0] == 1]] = host[2][host[0] == 1, 1]
        assert np.array_equal(chem.get_step_memory(mech, N), want)
    assert chem.get_step_memory(mech, N).any()
    chem.set_policy(mech, 4, FACTOR, FLOOR)
    assert not chem.get_step_memory(mech, N).any(), "set_policy keeps the step memory"
    SR._host_step(chem, col, mech, ks, 2)
    assert chem.get_step_memory(mech, N).any()
    chem.clear_policy(mech)
    assert not chem.get_step_memory(mech, N).any(), "clear_policy keeps the step memory"
    # with a column step open: refused with step_is_open's text, the old policy stays
    chem.set_policy(mech, 3)
    pending = SR._host_step(chem, col, mech, ks, 3, begin_only=True)
    for change in (lambda: chem.set_policy(mech, *POLICY), lambda: chem.clear_policy(mech)):
        with pytest.raises(chem.MistraChemError) as e:
            change()
        assert "a column step of the gas mechanism is open (mistra_chem_drive_begin)" in str(e.value)
    assert chem.get_policy(mech) == chem.Policy(3, 0.0, 0.0)
    chem.drive_host_end(mech)
    assert (pending[0] == 1).all()


# ---- 9. a user slot
def test_p9_user_slot(chem):
    import user_mech_cases as uc
    uc.ensure_tables()
    name = "demo_g"
    V, F, K = uc.batch(name, load_golden(uc.DEMOS[name][0]), 3)
    plain = _integrate_ex(chem, name, V, F, K)
    policy = (2, FACTOR, FLOOR)
    chem.set_policy(name, *policy)
    assert chem.get_policy(name) == chem.Policy(*policy)
    got = _integrate_ex(chem, name, V, F, K)
    ipar, rpar, _, rtol = R.base_options("gas")
    res, th = chem.rosenbrock_cells(name, V, F, K, R.TIN, R.TOUT, ipar, rpar, chem.cell_atol(name, V, FACTOR, FLOOR), np.full((3, 1), 1.0e-3))
    assert _same(got, dict(var=res.var, ierr=res.ierr, stats=res.stats, th=np.ascontiguousarray(th[:, :2])))
    assert _same(got, _yardstick(chem, name, V, F, K, policy))
    dev, ok = _integrate_device(chem, name, V, F, K)
    assert ok and _same(dev, got)
    with pytest.raises(chem.MistraChemError) as e:
        chem.set_policy(name, 4, FACTOR, FLOOR)
    assert "user mechanism slot 0 (demo_g) has no kernel for this Rosenbrock method" in str(e.value)
    assert chem.get_policy(name) == chem.Policy(*policy)
    chem.clear_policy(name)
    assert _same(_integrate_ex(chem, name, V, F, K), plain)


# ---- 10. the environment of a linked model binary
def test_p10_environment(chem):
    """In fresh processes: MISTRA_CHEM_ATOL_REL_T and MISTRA_CHEM_METHOD_T reach the integrator (the counters of the explicit policy), and a value that
    cannot be read makes mistra_chem_init fail with the variable's name."""
    mech = "tot"
    V, F, K = _cells(mech)
    chem.set_policy(mech, *POLICY)
    want = _integrate_ex(chem, mech, V, F, K)
    chem.clear_policy(mech)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from mistra_amd import chem\n"
            "from conftest import load_golden\n"
            "import ros_options_py as R\n"
            "try:\n"
            "    chem.init(0)\n"
            "except chem.MistraChemError as e:\n"
            "    print('init-error', e)\n"
            "    sys.exit(0)\n"
            "g = load_golden('tot')\n"
            "c = list(R.cells_of(g['var_in'].shape[0]))\n"
            "res, th = chem.integrate_ex('tot', g['var_in'][c], g['fix'][c], g['rconst'][c], R.TIN, R.TOUT)\n"
            "print('stats', res.stats.ravel().tolist(), res.var.tobytes().hex()[:64])\n" % (REPO, os.path.join(REPO, "tests")))

    def child(**policy_env):
        env = {k: v for k, v in os.environ.items() if not k.startswith(("MISTRA_CHEM_METHOD", "MISTRA_CHEM_ATOL_REL"))}
        env.update(policy_env)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip()
    assert child(MISTRA_CHEM_METHOD="ros3", MISTRA_CHEM_METHOD_T="RODAS3", MISTRA_CHEM_ATOL_REL_T="1e-13") == \
        "stats %s %s" % (want["stats"].ravel().tolist(), want["var"].tobytes().hex()[:64])
    bad = child(MISTRA_CHEM_ATOL_REL_T="1e-13,zero")
    assert bad.startswith("init-error") and "MISTRA_CHEM_ATOL_REL_T=1e-13,zero" in bad


# ---- 11. from Fortran
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_p11_from_fortran(chem, tmp_path):
    """shim/shim_driver DP: MISTRA_SET_POLICY_g / _a (Rodas3, 1e-13, 1e-25), then the staged base1 column step (gas and aer layers) through the
    single-pass batched driver: the model arrays, ierr, /Statistics/, exit time and last step size of the same step through mistra_chem_drive from Python."""
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    g = SR._load("base1")
    SR._maps(chem, g)
    col = SR.Column(g)
    py = {}
    for mech in ("gas", "aer"):
        chem.set_policy(mech, *POLICY)
        py[mech] = SR._host_step(chem, col, mech, col.layers(mech), 0)
    col0 = SR.Column(g)
    j1, j5, nl = col0.a["s1"].shape[1], col0.a["s3"].shape[1], len(g["k"])
    assert not (g["mech"] == 2).any() and len(col.layers("gas")) + len(col.layers("aer")) == nl
    bg = np.zeros((SR.NLEV, SR.NRXN, 2))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array(POLICY, np.float64).tofile(f)
        np.array([N, j1, j5, SR.NLEV, SR.NRXN, nl, 1], np.float64).tofile(f)
        for mech in MECHS:      # (tot has no layers in this step: its maps are never used)
            src = mech if mech + "_gas_m2k" in g else "gas"
            for key in ("gas_m2k", "gas_k2m", "rad_m2k", "rad_k2m"):
                g[src + "_" + key].astype(np.float64).tofile(f)
        np.zeros(SR.NLEV).tofile(f)      # no budget levels
        for key in ("s1", "s3", "sl1", "sion1"):
            col0.a[key].tofile(f)
        bg.tofile(f)
        col0.a["bgs"].tofile(f)
        for i in range(nl):
            np.array([g["mech"][i] + 1, g["k"][i], g["scal"][i, 0], g["scal"][i, 1]], np.float64).tofile(f)
            g["env"][i, :SR.NENV[MECHS[g["mech"][i]]]].tofile(f)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("MISTRA_CHEM_METHOD", "MISTRA_CHEM_ATOL_REL"))}
    subprocess.run([DRIVER, "DP", str(fin), str(fout)], check=True, timeout=300, env=env)
    raw = np.fromfile(fout, np.float64)
    off = 0
    for key in ("s1", "s3", "sl1", "sion1"):
        got = raw[off:off + col0.a[key].size].reshape(col0.a[key].shape)
        assert got.tobytes() == col.a[key].tobytes(), "%s after the step differs from the Python run" % key
        off += got.size
    off += bg.size
    assert raw[off:off + col0.a["bgs"].size].tobytes() == col.a["bgs"].tobytes()
    off += col0.a["bgs"].size
    rec = raw[off:off + 13 * nl].reshape(nl, 13)
    for m, mech in enumerate(("gas", "aer")):
        mine = rec[rec[:, 0] == m + 1]
        assert np.array_equal(mine[:, 1].astype(int), np.asarray(col.layers(mech)))
        assert np.array_equal(mine[:, 2].astype(np.int32), py[mech][0])
        assert np.array_equal(mine[:, 3:11].astype(np.int32), py[mech][1]), "/Statistics/ from Fortran %s, from Python %s" % (mine[:, 5].tolist(), py[mech][1][:, 2].tolist())
        assert mine[:, 11:13].tobytes() == np.ascontiguousarray(py[mech][2][:, :2]).tobytes()
