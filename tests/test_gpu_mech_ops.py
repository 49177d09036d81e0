"""The operators on the GPU (-m gpu): mistra_chem_ops_ex / _device on the captured cells of tests/golden/column_BTZ96.npz (68 gas,
31 aer, 49 tot).  vdot and jvs are the oracle's values; vdot, the prepared matrix and the fun_rhs row are the integrator's own first step bit for bit
(mistra_chem_debug_first_step_ex); the solves are held to the row-wise backward error of tests/mech_ops_bounds.py, measured on the reference side by
tests/test_mech_ops.py; explicit rows, shifts, cells and the two entries are invariant bit for bit; zero pivots are KppDecomp_x's.  Outputs go into caller
arrays with one row more than the call and a poison of its own in every entry: everything the call does not name stays as it was."""
import os
import subprocess

import numpy as np
import pytest

import mech_ops_bounds as MB
import mech_ops_py as MO
from conftest import MECHS, REPO

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "shim", "shim_driver")
SHIFT0 = 1.0 / (1.0e-3 * MO.GAMMA1)


@pytest.fixture(scope="module")
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def ref(oracles):
    """per mechanism, computed once and left unchanged: the captured cells, the oracle's vdot and jvs of every cell, the pattern"""
    out = {}
    for m in MECHS:
        V, F, K = MO.column_cells(m)
        orc = oracles[m]
        vdot = np.array([orc.fun(V[c], F[c], K[c]) for c in range(len(V))])
        jvs = np.array([orc.jac_sp(V[c], F[c], K[c]) for c in range(len(V))])
        for a in (V, F, K, vdot, jvs):
            a.setflags(write=False)
        out[m] = dict(V=V, F=F, K=K, vdot=vdot, jvs=jvs, pat=MO.pattern(m))
    return out


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _poison(shape, dtype=np.float64):
    """an array with a value of its own in every entry, none of which a result can be"""
    n = int(np.prod(shape))
    return (-(1.0e3 + np.arange(n))).astype(dtype).reshape(shape)


def _dev(chem, mech, V, F, K, want_vdot=False, want_jvs=False, shift=None, rhs=None, fun_rhs=False, extra=1):
    """the device entry into poisoned caller arrays with `extra` rows more than the call -> OpsResult of numpy arrays (the parts the call names), after
    checking that every entry behind them still holds its poison"""
    import torch
    nvar, nnz, n = V.shape[1], chem.DIMS[mech][3], V.shape[0]
    solve = shift is not None
    nrow = (1 if fun_rhs else 0) + (0 if rhs is None else rhs.shape[0])
    bufs = {}
    if want_vdot:
        bufs["vdot"] = _poison((n + extra, nvar))
    if want_jvs:
        bufs["jvs"] = _poison((n + extra, nnz))
    if solve:
        bufs["x"] = _poison((nrow + extra, n, nvar))
        bufs["ising"] = _poison((n + extra,), np.int32)
    dev = {k: _T(v) for k, v in bufs.items()}
    sh = None if not solve else (shift if np.isscalar(shift) else _T(np.asarray(shift, np.float64)))
    r = chem.ops(mech, _T(V), _T(F), _T(K), want_vdot, want_jvs, shift=sh, rhs=None if rhs is None else _T(rhs), fun_rhs=fun_rhs, **dev)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    used = {"vdot": n * nvar, "jvs": n * nnz, "x": nrow * n * nvar, "ising": n}
    for k, v in got.items():
        assert v.reshape(-1)[used[k]:].tobytes() == bufs[k].reshape(-1)[used[k]:].tobytes(), "%s: entries behind the call's were written" % k
        assert not np.any(v.reshape(-1)[:used[k]] == bufs[k].reshape(-1)[:used[k]]), "%s: an entry the call names was not written" % k
    return chem.OpsResult(*(None if x is None else x.cpu().numpy() for x in r))


def _same(a, b, what=""):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---- 1. Fun_x and Jac_SP_x
@pytest.mark.parametrize("mech", MECHS)
def test_o1_vdot_and_jvs_are_the_oracles(chem, mech, ref):
    """every captured cell in one launch: vdot = Oracle.fun, jvs = Oracle.jac_sp (np.array_equal: the sign of an exactly cancelling computed sum is not
    asserted — the gather-sum starts at 0.0, the generated code at its first term); the fill-in slots are +0.0 by bytes; each alone gives the same bits"""
    from mistra_amd import mechtab
    R = ref[mech]
    r = _dev(chem, mech, R["V"], R["F"], R["K"], True, True)
    assert np.array_equal(r.vdot, R["vdot"]) and np.array_equal(r.jvs, R["jvs"])
    t = mechtab.load(mech)
    fill = np.flatnonzero(np.diff(t.jv_ptr) == 0)
    assert fill.size == t.nnz - {"gas": 945, "aer": 2831, "tot": 4709}[mech]
    assert r.jvs[:, fill].tobytes() == np.zeros((len(R["V"]), fill.size)).tobytes()
    assert r.x is None and r.ising is None
    _same(_dev(chem, mech, R["V"], R["F"], R["K"], True, False).vdot, r.vdot, "vdot alone")
    _same(_dev(chem, mech, R["V"], R["F"], R["K"], False, True).jvs, r.jvs, "jvs alone")
    _same(chem.fun(mech, _T(R["V"]), _T(R["F"]), _T(R["K"])).cpu().numpy(), r.vdot, "chem.fun")
    _same(chem.jac_sp(mech, _T(R["V"][:1]), _T(R["F"][:1]), _T(R["K"][:1])).cpu().numpy(), r.jvs[:1], "chem.jac_sp, one cell")


# ---- 2. the integrator's own first step
@pytest.mark.parametrize("mech", MECHS)
def test_o2_tie_to_the_first_step_dump(chem, mech, ref):
    """mistra_chem_debug_first_step_ex on the same cells at hstart = 1e-3, H from the dump: its Fcn0 is vdot, its prepared Ghimj is (-jvs) with
    shift = 1.0/(1.0*H*gamma1) added on the diagonal slots (the -0.0 fill-ins included), its K(1) is the fun_rhs row of x at that shift — by bytes"""
    R = ref[mech]
    n = min(16, len(R["V"]))
    V, F, K = R["V"][:n], R["F"][:n], R["K"][:n]
    fs = chem.debug_first_step(mech, V, F, K, 0.0, 10.0, hstart=np.full(n, 1.0e-3))
    H = fs.h[:, 0]
    assert np.all(H > 0)
    shift = 1.0 / (1.0 * H * MO.GAMMA1)
    r = _dev(chem, mech, V, F, K, True, True, shift=shift, fun_rhs=True)
    assert np.all(r.ising == 0)
    _same(r.vdot, np.ascontiguousarray(fs.fcn0), "Fcn0")
    diag = R["pat"][2]
    a = np.array([MO.prepared(r.jvs[c], diag, shift[c]) for c in range(n)])
    _same(a, np.ascontiguousarray(fs.ghimj), "Ghimj as prepared")
    assert np.signbit(a[:, np.flatnonzero(r.jvs[0] == 0.0)]).any()      # (the -0.0 fill-ins are in the comparison)
    _same(r.x[0], np.ascontiguousarray(fs.k1), "K(1)")


# ---- 3. the bound on x
@pytest.mark.parametrize("mech", MECHS)
def test_o3_backward_error_within_ten_times_the_oracles(chem, mech, ref, oracles):
    """the cases of tests/mech_ops_bounds.py (eight cells, four shifts, the cell's vdot — as the fun_rhs row and as an explicit row —, its var and a
    seeded normal vector): the row-wise backward error of every solve, formed in long double from the oracle's A, is within 10x the oracle's own worst
    over its six re-association variants.  Measured on the MI355X (mech_ops_bounds.GPU_OMEGA): see there."""
    crow, icol, diag = ref[mech]["pat"]
    idx, V, F, K = MB.cells(mech)
    vdot, jvs = ref[mech]["vdot"][idx], ref[mech]["jvs"][idx]
    rows = MB.rhs_rows(mech, vdot, V)
    worst = 0.0
    for sh in MB.shifts():
        r = _dev(chem, mech, V, F, K, shift=sh, rhs=rows, fun_rhs=True)
        assert np.all(r.ising == 0) and np.isfinite(r.x).all()
        for c in range(len(V)):
            a = MO.prepared(jvs[c], diag, sh)
            for j in range(4):
                b = vdot[c] + 0.0 if j == 0 else rows[j - 1, c]
                w = MO.backward_error(a, crow, icol, r.x[j, c], b)
                worst = max(worst, w)
        print("%s shift %.6g: worst omega so far %.3e" % (mech, sh, worst))
    print("%s: kernel worst omega %.3e, bound %.3e (oracle %.3e)" % (mech, worst, MB.OMEGA_BOUND[mech], MB.ORACLE_OMEGA[mech]))
    assert worst <= MB.OMEGA_BOUND[mech]


# ---- 4. invariances, bit for bit
@pytest.mark.parametrize("mech", MECHS)
def test_o4_an_explicit_row_does_not_depend_on_its_place(chem, mech, ref):
    """an explicit row gives the same x as row 0 of 1, row 1 of 2 and row 8 of 9, with and without fun_rhs, with and without vdot / jvs asked for"""
    R = ref[mech]
    n = 3
    V, F, K = R["V"][:n], R["F"][:n], R["K"][:n]
    rng = np.random.default_rng(4)
    row = rng.standard_normal((1, n, V.shape[1]))
    others = rng.standard_normal((8, n, V.shape[1])) * np.abs(V).max()
    for sh in (SHIFT0, 1.0e-4):
        want = _dev(chem, mech, V, F, K, shift=sh, rhs=row).x[0]
        for fun_rhs in (False, True):
            for wv, wj in ((False, False), (True, True)):
                o = 1 if fun_rhs else 0
                _same(_dev(chem, mech, V, F, K, wv, wj, shift=sh, rhs=row, fun_rhs=fun_rhs).x[o], want, "row 0 of 1")
                _same(_dev(chem, mech, V, F, K, wv, wj, shift=sh, rhs=np.concatenate([others[:1], row]), fun_rhs=fun_rhs).x[o + 1], want, "row 1 of 2")
                _same(_dev(chem, mech, V, F, K, wv, wj, shift=sh, rhs=np.concatenate([others, row]), fun_rhs=fun_rhs).x[o + 8], want, "row 8 of 9")


@pytest.mark.parametrize("mech", MECHS)
def test_o5_shifts_and_cells(chem, mech, ref):
    """nshift = 1 equals nshift = ncell with equal entries; per-cell shifts that all differ give each cell the x it has alone; a cell alone, first of 2,
    last of 3 and inside all captured cells gives the same rows"""
    R = ref[mech]
    V, F, K = R["V"], R["F"], R["K"]
    n = len(V)
    rows = np.ascontiguousarray(np.stack([V, np.random.default_rng(5).standard_normal(V.shape)]))
    shared = _dev(chem, mech, V, F, K, True, True, shift=SHIFT0, rhs=rows, fun_rhs=True)
    each = _dev(chem, mech, V, F, K, True, True, shift=np.full(n, SHIFT0), rhs=rows, fun_rhs=True)
    for a, b in zip(shared, each):
        _same(a, b, "nshift 1 / ncell")
    shifts = SHIFT0 * (1.0 + np.arange(n) / 7.0)
    differ = _dev(chem, mech, V, F, K, shift=shifts, rhs=rows, fun_rhs=True)
    assert np.all(differ.ising == 0)
    c = n // 2
    for cells in ([c], [c, 0], [1, 0, c]):
        got = _dev(chem, mech, V[cells], F[cells], K[cells], True, True, shift=SHIFT0, rhs=rows[:, cells], fun_rhs=True)
        k = cells.index(c)
        _same(got.x[:, k], shared.x[:, c], "cell %d in a batch of %d" % (c, len(cells)))
        _same(got.vdot[k], shared.vdot[c])
        _same(got.jvs[k], shared.jvs[c])
    for k in (0, c, n - 1):
        alone = _dev(chem, mech, V[k:k + 1], F[k:k + 1], K[k:k + 1], shift=shifts[k:k + 1], rhs=rows[:, k:k + 1], fun_rhs=True)
        _same(alone.x[:, 0], differ.x[:, k], "cell %d alone at its own shift" % k)


@pytest.mark.parametrize("mech", MECHS)
def test_o6_the_host_form_gives_the_device_forms_bits(chem, mech, ref):
    R = ref[mech]
    n = 5
    V, F, K = R["V"][:n], R["F"][:n], R["K"][:n]
    rows = np.ascontiguousarray(np.stack([V, R["vdot"][:n]]))
    shifts = SHIFT0 / (1.0 + np.arange(n))
    want = _dev(chem, mech, V, F, K, True, True, shift=shifts, rhs=rows, fun_rhs=True)
    bufs = dict(vdot=_poison((n + 1, V.shape[1])), jvs=_poison((n + 1, chem.DIMS[mech][3])), x=_poison((4, n, V.shape[1])), ising=_poison((n + 1,), np.int32))
    keep = {k: v.copy() for k, v in bufs.items()}
    got = chem.ops(mech, V, F, K, True, True, shift=shifts, rhs=rows, fun_rhs=True, **bufs)
    for a, b in zip(got, want):
        _same(a, b, "host / device")
    for k, used in (("vdot", n * V.shape[1]), ("jvs", n * chem.DIMS[mech][3]), ("x", 3 * n * V.shape[1]), ("ising", n)):
        assert bufs[k].reshape(-1)[used:].tobytes() == keep[k].reshape(-1)[used:].tobytes(), k
    x, ising = chem.linsolve(mech, V, F, K, SHIFT0, rhs=rows[:1])
    _same(x, _dev(chem, mech, V, F, K, shift=SHIFT0, rhs=rows[:1]).x, "chem.linsolve")
    assert np.all(ising == 0)


# ---- 5. zero pivots
@pytest.mark.parametrize("mech", MECHS)
def test_o7_zero_pivots_are_kppdecomps(chem, mech, ref, oracles):
    """shift[c] = J(i,i) read from the oracle, for a low and a high i: ising[c] = i + 1 as Oracle.decomp returns, the cell's x rows are +0.0, its vdot and
    jvs are produced, the other cells of the batch are unaffected; shift = 0: ising is the oracle's"""
    R = ref[mech]
    diag = R["pat"][2]
    n = 5
    V, F, K = R["V"][:n], R["F"][:n], R["K"][:n]
    rows = np.ascontiguousarray(V[None])
    shifts = np.full(n, SHIFT0)
    hit = {}
    for c, pick in ((1, 1), (3, -2)):
        i = np.flatnonzero(R["jvs"][c][diag] != 0.0)[pick]
        shifts[c] = R["jvs"][c][diag[i]]
        hit[c] = oracles[mech].decomp(MO.prepared(R["jvs"][c], diag, shifts[c]))[1]
        assert hit[c] == i + 1
    plain = _dev(chem, mech, V, F, K, True, True, shift=SHIFT0, rhs=rows, fun_rhs=True)
    r = _dev(chem, mech, V, F, K, True, True, shift=shifts, rhs=rows, fun_rhs=True)
    assert r.ising.tolist() == [0, hit[1], 0, hit[3], 0]
    _same(r.vdot, plain.vdot)
    _same(r.jvs, plain.jvs)
    for c in range(n):
        if c in hit:
            _same(r.x[:, c], np.zeros((2, V.shape[1])), "rows of a cell with a zero pivot")
        else:
            _same(r.x[:, c], plain.x[:, c], "a cell beside one with a zero pivot")
    z = _dev(chem, mech, V, F, K, shift=0.0, rhs=rows)
    want = [oracles[mech].decomp(MO.prepared(R["jvs"][c], diag, 0.0))[1] for c in range(n)]
    assert z.ising.tolist() == want, (z.ising.tolist(), want)
    for c in range(n):
        if want[c]:
            _same(z.x[:, c], np.zeros((1, V.shape[1])))


# ---- 6. Fortran
@pytest.mark.parametrize("mech", MECHS)
def test_o8_fortran_bindings(chem, mech, ref, tmp_path):
    """FUN_BATCH_x, JAC_SP_BATCH_x and LINSOLVE_BATCH_x (shim/mistra_kpp_shim.f90) on two cells from one Fortran program: the Python results by bytes"""
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    R = ref[mech]
    V, F, K = R["V"][:2], R["F"][:2], R["K"][:2]
    rows = np.ascontiguousarray(np.stack([V, R["vdot"][:2]]))
    shifts = np.array([SHIFT0, 1.0e-4])
    want = chem.ops(mech, V, F, K, True, True, shift=shifts, rhs=rows, fun_rhs=True)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([2.0, 2.0, 1.0, 2.0]).tofile(f)
        shifts.tofile(f)
        for c in range(2):
            np.concatenate([V[c], F[c], K[c]]).tofile(f)
        rows.tofile(f)
    subprocess.run([DRIVER, "P" + mech[0].upper(), str(fin), str(fout)], check=True, timeout=300)
    out = np.fromfile(fout)
    nv, nz = V.shape[1], chem.DIMS[mech][3]
    parts = np.split(out, np.cumsum([2 * nv, 2 * nz, 3 * 2 * nv]))
    _same(parts[0].reshape(2, nv), want.vdot, "FUN_BATCH")
    _same(parts[1].reshape(2, nz), want.jvs, "JAC_SP_BATCH")
    _same(parts[2].reshape(3, 2, nv), want.x, "LINSOLVE_BATCH")
    assert parts[3].tolist() == want.ising.tolist() == [0.0, 0.0]
