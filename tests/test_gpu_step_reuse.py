"""Step reuse of the batched driver on the GPU (-m gpu; include/mistra_chem.h: mistra_chem_set_step_reuse, OPT-IN and not the reference's behaviour): with
reuse on, mistra_chem_drive(_begin) starts every layer at the last accepted step size of the layer's previous column step of the mechanism, kept in a
device-side memory keyed by the model layer k.

What a step under reuse must compute is stated twice.  (a) The explicit device-resident chain of the public pieces — pack, rates_env_from_c, the rate kernel,
integrate_into(hstart=...), budgets, unpack — given the memory as read before the step: bit for bit.  (b) The oracle started at the same first steps
(Oracle.integrate_batch(hstart=...), the form of tests/test_gpu_parity.py::test_opt_in_hstart_reuse) on the step's packed C and the device's RCONST: IERR and
/Statistics/ identical, VAR within the mechanism's bound of tests/parity_bounds.py.  Off is today's path, bit for bit.

Columns: tests/golden/drivecol_Joyce2014.npz (148 gas layers), drivecol_BTZ96.npz (68 gas + 46 aer + 34 tot); integrate_tot.npz for the host-buffer entry.
Consecutive steps run on the arrays the step before left, with the captured step's rates (step s covers 10 s .. 10 (s + 1))."""
import os
import subprocess

import numpy as np
import pytest

import ros_options_py as R
from conftest import MECHS, REPO, load_golden, rel_diff
from parity_bounds import PARITY_RTOL

pytestmark = pytest.mark.gpu
NVAR = {"gas": 102, "aer": 257, "tot": 417}
NFIX = {"gas": 3, "aer": 5, "tot": 7}
NENV = {"gas": 74, "aer": 330, "tot": 544}
N, NBGS, NLEV, NRXN = 150, 122, 15, 1627      # global_params.f90: n, nlev, nrxn; bud_s_g.f:63
POISON = -7.25
DT = 10.0
KEYS = ("s1", "s3", "sl1", "sion1", "bgs")
DRIVER = os.path.join(REPO, "shim", "shim_driver")


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    for mech in MECHS:
        c.set_step_reuse(mech, False)
    yield c
    if c.device_count() != 1:      # whatever a test initialised: the other modules' fixtures start from init(0)
        c.finalize()
        c.init(0)
    for mech in MECHS:             # and from the reference's path
        c.set_step_reuse(mech, False)
        c.clear_options(mech)


_COLUMNS = {}


def _load(case):
    if case not in _COLUMNS:
        _COLUMNS[case] = dict(np.load(os.path.join(REPO, "tests", "golden", "drivecol_%s.npz" % case)))
    return _COLUMNS[case]


class Column:
    """The model's arrays in front of a captured step.  rows: {model layer k: index of the captured layer whose data stand in row k} (default: the
    capture's own layers); every other row is poisoned."""

    def __init__(self, g, rows=None):
        self.g = g
        self.src = rows if rows is not None else {int(k): i for i, k in enumerate(g["k"])}
        ks = np.array(sorted(self.src), np.int64)
        idx = [self.src[int(k)] for k in ks]
        self.a = {}
        for key in ("s1", "s3", "sl1", "sion1"):
            self.a[key] = np.full((N, g[key + "_in"].shape[1]), POISON)
            self.a[key][ks - 1] = g[key + "_in"][idx]
        self.a["bgs"] = np.full((N, NBGS, 2), POISON)
        self.a["bgs"][ks - 1] = g["bgs_in"][idx].reshape(-1, NBGS, 2)

    def copy(self):
        c = Column.__new__(Column)
        c.g, c.src, c.a = self.g, self.src, {k: v.copy() for k, v in self.a.items()}
        return c

    def layers(self, mech):
        m = MECHS.index(mech)
        return [k for k in sorted(self.src) if self.g["mech"][self.src[k]] == m]

    def inputs(self, mech, ks):
        idx = [self.src[int(k)] for k in ks]
        return np.ascontiguousarray(self.g["scal"][idx]), np.ascontiguousarray(self.g["env"][idx, :NENV[mech]])


def _maps(chem, g):
    for m, mech in enumerate(MECHS):
        if (g["mech"] == m).any():
            chem.set_species_maps(mech, g[mech + "_gas_m2k"], g[mech + "_gas_k2m"], g[mech + "_rad_m2k"], g[mech + "_rad_k2m"])


def _host_step(chem, col, mech, ks, step, want_c=False, begin_only=False):
    """one column step of `mech` for the layers ks through mistra_chem_drive(_begin) on col's arrays -> (ierr, stats, t_h[, c_packed])"""
    scal, env = col.inputs(mech, ks)
    a = col.a
    return chem.drive_host(mech, np.asarray(ks, np.int32), a["s1"], a["s3"], a["sl1"], a["sion1"], scal, env, DT * step, DT, bgs=a["bgs"], want_c=want_c,
                           begin_only=begin_only)


def _chain_step(chem, col, mech, ks, step, hstart=None):
    """the same step from the public device-resident pieces on copies of col's rows (col is left alone) -> dict: the rows after the step, ierr, stats, th
    [nl, 2], C as packed, VAR as integrated, RCONST"""
    import torch
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    kk = np.asarray(ks, np.int64) - 1
    nl = len(kk)
    scal, env = col.inputs(mech, ks)
    d = {key: T(col.a[key][kk]) for key in KEYS}
    var = torch.zeros((nl, NVAR[mech]), dtype=torch.float64, device=dev)      # KPP's dummy products start from 0, as in mistra_chem_drive
    fix = torch.zeros((nl, NFIX[mech]), dtype=torch.float64, device=dev)
    chem.pack(mech, d["s1"], d["s3"], d["sl1"], d["sion1"], T(scal), var, fix)
    c_packed = torch.cat([var, fix], dim=1).cpu().numpy()
    envd = T(env)
    chem.rates_env_from_c(mech, var, fix, envd)
    rct = chem.update_rconst(mech, envd)
    ierr = torch.empty(nl, dtype=torch.int32, device=dev)
    stats = torch.empty((nl, 8), dtype=torch.int32, device=dev)
    th = torch.empty((nl, 2), dtype=torch.float64, device=dev)
    chem.integrate_into(mech, var, fix, rct, var, ierr, stats, DT * step, DT * step + DT, texit_hexit=th, hstart=None if hstart is None else T(hstart))
    var_out = var.cpu().numpy()
    chem.budgets(mech, var, fix, rct, DT, None, d["bgs"])
    chem.unpack(mech, var, d["s1"], d["s3"], d["sl1"], d["sion1"])
    torch.cuda.synchronize()
    out = {key: d[key].cpu().numpy() for key in KEYS}
    out.update(ierr=ierr.cpu().numpy(), stats=stats.cpu().numpy(), th=th.cpu().numpy(), c=c_packed, var=var_out, rct=rct.cpu().numpy())
    return out


def _assert_same(col, ks, host, chain, what):
    """the arrays of col after a host step, and what the step returned, against the chain's: every bit"""
    kk = np.asarray(ks, np.int64) - 1
    for key in KEYS:
        assert np.array_equal(col.a[key][kk], chain[key]), "%s: %s differs from the explicit chain" % (what, key)
    assert np.array_equal(host[0], chain["ierr"]), "%s: ierr" % what
    assert np.array_equal(host[1], chain["stats"]), "%s: /Statistics/ %s vs the chain's %s" % (what, host[1][:, 2].tolist(), chain["stats"][:, 2].tolist())
    assert np.array_equal(host[2][:, :2], chain["th"]), "%s: exit time / last step size" % what
    if len(host) > 3:
        assert np.array_equal(host[3], chain["c"]), "%s: C as packed" % what


def _reuse_step(chem, col, mech, ks, step, what, want_c=False):
    """A step under reuse, checked (a) against the explicit chain started at the memory as read before the step and (c) for the memory it leaves.
    -> (host result, chain result, the first steps used)"""
    before = chem.get_step_memory(mech, N)
    hstart = before[np.asarray(ks, np.int64) - 1]
    chain = _chain_step(chem, col, mech, ks, step, hstart)
    host = _host_step(chem, col, mech, ks, step, want_c=want_c)
    _assert_same(col, ks, host, chain, what)
    want = np.zeros(N)
    ok = host[0] == 1
    want[np.asarray(ks, np.int64)[ok] - 1] = host[2][ok, 1]
    assert np.array_equal(chem.get_step_memory(mech, N), want), "%s: the memory is not Hexit at the step's layers and 0 elsewhere" % what
    return host, chain, hstart


def _forget(chem, mech):
    chem.set_step_reuse(mech, False)
    chem.set_step_reuse(mech, True)
    assert not chem.get_step_memory(mech, N).any()


def test_1_off_is_todays_path(chem):
    g = _load("Joyce2014")
    _maps(chem, g)
    col = Column(g)
    ks = col.layers("gas")
    assert len(ks) == 148
    first = None
    for step in range(2):
        chain = _chain_step(chem, col, "gas", ks, step)
        host = _host_step(chem, col, "gas", ks, step, want_c=True)
        _assert_same(col, ks, host, chain, "reuse off, step %d" % step)
        assert (host[0] == 1).all()
        if step == 0:
            assert np.array_equal(host[1], g["stats"]), "the captured step's /Statistics/"
            first = (host, col.copy())
        assert not chem.get_step_memory("gas", N).any(), "reuse is off: nothing is remembered"
    # on: the first step finds an empty memory
    chem.set_step_reuse("gas", True)
    assert chem.get_step_reuse("gas") and not chem.get_step_memory("gas", N).any()
    col_on = Column(g)
    host_on = _host_step(chem, col_on, "gas", ks, 0, want_c=True)
    for key in KEYS:
        assert np.array_equal(col_on.a[key], first[1].a[key]), key
    for x, y in zip(host_on, first[0]):
        assert np.array_equal(x, y)


def test_2_three_consecutive_steps_of_a_gas_column(chem, oracles):
    g = _load("Joyce2014")
    _maps(chem, g)
    ks = Column(g).layers("gas")
    off, col = [], Column(g)
    for step in range(3):
        off.append(_host_step(chem, col, "gas", ks, step))
    chem.set_step_reuse("gas", True)
    col, on = Column(g), []
    for step in range(3):
        host, chain, hstart = _reuse_step(chem, col, "gas", ks, step, "step %d" % step, want_c=True)
        assert (host[0] == 1).all()
        assert (hstart > 0).all() if step else not hstart.any()
        # (b) the oracle at the same first steps, on the step's packed C and the device's rate constants: every layer
        c = host[3]
        want, ierr, st = oracles["gas"].integrate_batch(c[:, :NVAR["gas"]], c[:, NVAR["gas"]:], chain["rct"], DT * step, DT * step + DT, hstart=hstart)
        d = rel_diff(chain["var"], want).max()
        print("step %d: Nstp %d..%d (sum %d; reuse off %d), VAR %.2e from the oracle at the same first steps (bound %.0e)"
              % (step, host[1][:, 2].min(), host[1][:, 2].max(), host[1][:, 2].sum(), off[step][1][:, 2].sum(), d, PARITY_RTOL["gas"]))
        assert np.array_equal(host[0], ierr)
        assert np.array_equal(host[1], st), "/Statistics/ differ from the oracle started at the same first steps"
        assert d <= PARITY_RTOL["gas"]
        on.append(host)
    assert sum(int(on[s][1][:, 2].sum()) for s in (1, 2)) < sum(int(off[s][1][:, 2].sum()) for s in (1, 2))


def _layer_set_scenario(chem, g, rows, first, second, third):
    """three steps of gas layer sets under reuse; after the second the memory holds the second set only, so the layers the third adds start from scratch"""
    _forget(chem, "gas")
    col = Column(g, rows)
    _reuse_step(chem, col, "gas", first, 0, "first set")
    mem = chem.get_step_memory("gas", N)
    host2, _, h2 = _reuse_step(chem, col, "gas", second, 1, "second set")
    assert all((h > 0 and h == mem[k - 1]) if k in first else h == 0.0 for k, h in zip(second, h2))
    mem = chem.get_step_memory("gas", N)
    gone = sorted(set(first) - set(second))
    assert not mem[np.asarray(gone, np.int64) - 1].any(), "a layer that sat the step out is still remembered"
    assert (mem[np.asarray(second, np.int64) - 1] > 0).all()
    host3, chain3, h3 = _reuse_step(chem, col, "gas", third, 2, "third set")
    assert all((h > 0 and h == mem[k - 1]) if k in second else h == 0.0 for k, h in zip(third, h3)), "a layer the third step adds does not start from scratch"
    return host3


def test_3_layer_sets_change(chem):
    g = _load("Joyce2014")
    _maps(chem, g)
    chem.set_step_reuse("gas", True)
    ks = Column(g).layers("gas")
    A, B = [k for k in ks if k % 2 == 1], [k for k in ks if k % 2 == 0]
    host3 = _layer_set_scenario(chem, g, None, ks[::-1], A, ks)
    nstp = dict(zip(ks, host3[1][:, 2].tolist()))
    print("third step: Nstp of the carried layers %d..%d, of the layers that start from 1e-3 again %d..%d"
          % (min(nstp[k] for k in A), max(nstp[k] for k in A), min(nstp[k] for k in B), max(nstp[k] for k in B)))
    # one layer per batch, the column's first and last: rows 1 and n = 150 stand in for captured layers
    rows = {1: 0, N: 147}
    _layer_set_scenario(chem, g, rows, [N], [1], [N])
    _layer_set_scenario(chem, g, rows, [1], [N], [1])
    # 65 layers (a ragged last wave), unsorted, rows 1 and 150 among them
    rng = np.random.default_rng(3)
    pick = [1, N] + [int(k) for k in rng.choice(np.arange(2, N), 63, replace=False)]
    order = [int(k) for k in rng.permutation(pick)]
    rows = {k: int(i) for k, i in zip(pick, rng.choice(148, 65, replace=False))}
    assert len(order) == 65 and order != sorted(order)
    keep = order[::2] if 1 in order[::2] else order[1::2]
    _layer_set_scenario(chem, g, rows, order, keep, order[::-1])


def test_4_three_mechanisms_side_by_side(chem):
    g = _load("BTZ96")
    _maps(chem, g)
    base = Column(g)
    layers = {mech: base.layers(mech) for mech in MECHS}
    assert [len(layers[m]) for m in MECHS] == [68, 46, 34]

    def run(side_by_side):
        for mech in MECHS:
            _forget(chem, mech)
        col, outs = base.copy(), []
        for step in range(2):
            res = {}
            for mech in MECHS:
                res[mech] = _host_step(chem, col, mech, layers[mech], step, begin_only=side_by_side)
            if side_by_side:
                for mech in MECHS:
                    chem.drive_host_end(mech)
            outs.append({mech: res[mech][:3] for mech in MECHS})
            mem = {mech: chem.get_step_memory(mech, N) for mech in MECHS}
            for mech in MECHS:      # each mechanism's memory holds its own layers only
                want = np.zeros(N)
                want[np.asarray(layers[mech]) - 1] = res[mech][2][:, 1]
                assert (res[mech][0] == 1).all() and np.array_equal(mem[mech], want), mech
        return col, outs, mem

    col1, o1, m1 = run(False)
    col2, o2, m2 = run(True)
    for key in KEYS:
        assert np.array_equal(col1.a[key], col2.a[key]), "%s differs between the mechanisms one after the other and side by side" % key
    for s in range(2):
        for mech in MECHS:
            for x, y in zip(o1[s][mech], o2[s][mech]):
                assert np.array_equal(x, y), (s, mech)
            assert np.array_equal(m1[mech], m2[mech])
    print("BTZ96, summed Nstp of the first and of the second step: " +
          ", ".join("%s %d -> %d" % (mech, o1[0][mech][1][:, 2].sum(), o1[1][mech][1][:, 2].sum()) for mech in MECHS))
    # a step whose every cell fails (IERR = -6 through the test hook: an error exit) leaves nothing to remember
    chem.debug_set_max_steps(4)
    try:
        for mech in MECHS:
            _forget(chem, mech)
        col = base.copy()
        for mech in MECHS:
            ierr = _host_step(chem, col, mech, layers[mech], 0)[0]
            assert (ierr == -6).all(), (mech, ierr)
            assert not chem.get_step_memory(mech, N).any(), "%s: a failed layer is remembered" % mech
    finally:
        chem.debug_set_max_steps(0)


def test_5_options_restart_and_open_steps(chem):
    g = _load("Joyce2014")
    _maps(chem, g)
    mech = "gas"
    ks = Column(g).layers(mech)
    A = [k for k in ks if k % 2 == 1]
    B = [k for k in ks if k % 2 == 0]
    chem.set_step_reuse(mech, True)
    # ---- RPAR(3) = 0.5 in force: a remembered step goes before it, it serves where there is none
    chem.set_options(mech, *R.option_set(mech, "hstart_0.5"))
    col = Column(g)
    _reuse_step(chem, col, mech, A, 0, "options, first step")
    mem = chem.get_step_memory(mech, N)
    before = col.copy()
    host, chain, hstart = _reuse_step(chem, col, mech, ks, 1, "options, second step")
    explicit = np.where(hstart > 0, hstart, 0.5)
    assert (hstart == 0).sum() == len(B) and np.array_equal(hstart[hstart > 0], mem[np.asarray(A) - 1])
    again = _chain_step(chem, before, mech, ks, 1, explicit)
    for key in ("var", "stats", "th"):
        assert np.array_equal(again[key], chain[key]), "layers without a remembered step do not start at RPAR(3): %s" % key
    # ---- set_options and clear_options empty the memory
    assert chem.get_step_memory(mech, N).any()
    chem.set_options(mech, *R.option_set(mech, "hstart_0.5"))
    assert not chem.get_step_memory(mech, N).any()
    _host_step(chem, Column(g), mech, ks, 0)
    assert chem.get_step_memory(mech, N).any()
    chem.clear_options(mech)
    assert not chem.get_step_memory(mech, N).any()
    # ---- the restart pair: an interrupted run continues like an uninterrupted one
    col = Column(g)
    _host_step(chem, col, mech, ks, 0)
    saved, at_restart = chem.get_step_memory(mech, N), col.copy()
    want = _host_step(chem, col, mech, ks, 1)
    _forget(chem, mech)
    chem.set_step_memory(mech, saved)
    assert np.array_equal(chem.get_step_memory(mech, N), saved)
    got = _host_step(chem, at_restart, mech, ks, 1)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    for key in KEYS:
        assert np.array_equal(at_restart.a[key], col.a[key]), key
    with pytest.raises(chem.MistraChemError):
        chem.set_step_memory(mech, np.full(N, -1.0))
    with pytest.raises(chem.MistraChemError):
        chem.get_step_memory(mech, N - 1)
    # ---- while a step is open the memory is the step's
    r = _host_step(chem, col, mech, ks, 2, begin_only=True)
    try:
        with pytest.raises(chem.MistraChemError, match="is open"):
            chem.set_step_reuse(mech, False)
        with pytest.raises(chem.MistraChemError, match="is open"):
            chem.set_step_memory(mech, saved)
        with pytest.raises(chem.MistraChemError, match="is open"):
            chem.get_step_memory(mech, N)
        assert chem.get_step_reuse(mech)
    finally:
        chem.drive_host_end(mech)
    assert (r[0] == 1).all() and np.array_equal(chem.get_step_memory(mech, N)[np.asarray(ks) - 1], r[2][:, 1])


def test_6_host_buffer_hstart(chem):
    import torch
    mech = "tot"
    g = load_golden(mech)
    V, F, K = g["var_in"][:5], g["fix"][:5], g["rconst"][:5]
    first, th1 = chem.integrate_ex(mech, V, F, K, 0.0, DT)
    assert (first.ierr == 1).all()
    hstart = th1[:, 1].copy()
    hstart[[1, 3]] = 0.0
    res, th = chem.integrate_ex(mech, first.var, F, K, DT, 2 * DT, hstart=hstart)
    plain, _ = chem.integrate_ex(mech, first.var, F, K, DT, 2 * DT)
    assert (res.ierr == 1).all()
    assert np.array_equal(res.stats[[1, 3]], plain.stats[[1, 3]]) and np.array_equal(res.var[[1, 3]], plain.var[[1, 3]])      # entries of 0: the reference's path
    print("tot, second call: Nstp %s from Hexit | 0, %s from 1e-3" % (res.stats[:, 2].tolist(), plain.stats[:, 2].tolist()))
    zero, thz = chem.integrate_ex(mech, first.var, F, K, DT, 2 * DT, hstart=np.zeros(5))
    assert np.array_equal(zero.var, plain.var) and np.array_equal(zero.stats, plain.stats)
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    out, ierr, stats = torch.empty((5, NVAR[mech]), dtype=torch.float64, device=dev), torch.empty(5, dtype=torch.int32, device=dev), torch.empty((5, 8), dtype=torch.int32, device=dev)
    thd = torch.empty((5, 2), dtype=torch.float64, device=dev)
    chem.integrate_into(mech, T(first.var), T(F), T(K), out, ierr, stats, DT, 2 * DT, texit_hexit=thd, hstart=T(hstart))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), res.var) and np.array_equal(ierr.cpu().numpy(), res.ierr) and np.array_equal(stats.cpu().numpy(), res.stats)
    assert np.array_equal(thd.cpu().numpy(), th[:, :2])
    # two device slots: every block of cells takes its own part of hstart
    chem.finalize()
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    two, th2 = chem.integrate_ex(mech, first.var, F, K, DT, 2 * DT, hstart=hstart)
    assert np.array_equal(two.var, res.var) and np.array_equal(two.ierr, res.ierr) and np.array_equal(two.stats, res.stats) and np.array_equal(th2, th)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang (ROCm) not installed")
def test_7_from_fortran(chem, tmp_path):
    """shim/shim_driver D2: MISTRA_STEP_REUSE_x(.true.), then the staged Joyce2014 column step twice in a row.  The first step's /Statistics/ are the captured
    ones; the second step's ierr, /Statistics/ and t_h are those of the same two steps through mistra_chem_drive from Python."""
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "shim")], check=True)
    g = _load("Joyce2014")
    _maps(chem, g)
    ks = Column(g).layers("gas")
    chem.set_step_reuse("gas", True)
    col = Column(g)
    py = [_host_step(chem, col, "gas", ks, step) for step in range(2)]
    col0 = Column(g)
    j1, j5, nl = col0.a["s1"].shape[1], col0.a["s3"].shape[1], len(ks)
    bg = np.zeros((NLEV, NRXN, 2))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([N, j1, j5, NLEV, NRXN, nl, 2], np.float64).tofile(f)
        for mech in MECHS:      # (aer and tot have no layers in this step: their maps are never used)
            for key in ("gas_m2k", "gas_k2m", "rad_m2k", "rad_k2m"):
                g["gas_" + key].astype(np.float64).tofile(f)
        np.zeros(NLEV).tofile(f)      # no budget levels
        for key in ("s1", "s3", "sl1", "sion1"):
            col0.a[key].tofile(f)
        bg.tofile(f)
        col0.a["bgs"].tofile(f)
        for i in range(nl):
            np.array([1, g["k"][i], g["scal"][i, 0], g["scal"][i, 1]], np.float64).tofile(f)
            g["env"][i, :NENV["gas"]].tofile(f)
    env = {k: v for k, v in os.environ.items() if k != "MISTRA_CHEM_HSTART_REUSE"}
    subprocess.run([DRIVER, "D2", str(fin), str(fout)], check=True, timeout=300, env=env)
    raw = np.fromfile(fout, np.float64)
    off = 0
    for key in ("s1", "s3", "sl1", "sion1"):
        got = raw[off:off + col0.a[key].size].reshape(col0.a[key].shape)
        assert np.array_equal(got, col.a[key]), "%s after the second step differs from the Python run" % key
        off += got.size
    off += bg.size
    assert np.array_equal(raw[off:off + col0.a["bgs"].size].reshape(N, NBGS, 2), col.a["bgs"])
    off += col0.a["bgs"].size
    steps = raw[off:off + 14 * nl * 2].reshape(2, nl, 14)
    assert off + steps.size == raw.size
    for s in range(2):
        assert np.array_equal(steps[s, :, 1].astype(int), g["k"]) and (steps[s, :, 0] == 1).all()
    assert np.array_equal(steps[0, :, 3:11].astype(np.int32), g["stats"]), "first step: the captured /Statistics/"
    for s in range(2):
        assert np.array_equal(steps[s, :, 2].astype(np.int32), py[s][0])
        assert np.array_equal(steps[s, :, 3:11].astype(np.int32), py[s][1]), "step %d: /Statistics/ from Fortran %s, from Python %s" % (s, steps[s, :, 5].tolist(), py[s][1][:, 2].tolist())
        assert np.array_equal(steps[s, :, 11:14], py[s][2])
