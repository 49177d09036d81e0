"""The user mechanism slots on the GPU (-m gpu): the two demo tables (tests/user_mech_cases.py) through every entry a user slot has.  Inputs: cells 0,
16 and 31 of the captured gas / aer sets, cut to the tables through their .json maps.  Expected values: the oracle on the SAME table; bounds:
tests/user_mech_bounds.py (the oracle's own spread under re-association, x10, held by tests/test_user_mech.py together with the condition that no
variant changes a counter on these cells — so IERR and all eight counters must be identical here).  A launch takes three cells, or 1 / 3 / 65 where
the batch edges are the subject."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import user_mech_bounds as ub
import user_mech_cases as uc
from conftest import MECHS, REPO, load_golden, rel_diff

pytestmark = pytest.mark.gpu
DEMO_NAMES = tuple(uc.DEMOS)
POISON_D, POISON_I = -7.77e77, -777
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module", autouse=True)
def demo_tables():
    uc.ensure_tables()


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
    for mech in MECHS + DEMO_NAMES:
        c.clear_options(mech)


def _golden(name):
    return load_golden(uc.DEMOS[name][0])


def _expect(name, run, n):
    """the oracle's result of `run` on the n cells of uc.batch: (VAR, IERR, counters, Texit, Hexit)"""
    idx = [i % len(uc.CELLS) for i in range(n)]
    return tuple(a[idx] for a in ub.oracle_run(name, run))


def _check(name, run, var, ierr, stats, te=None, he=None):
    n = var.shape[0]
    w_var, w_ierr, w_st, w_te, w_he = _expect(name, run, n)
    d_var = rel_diff(var, w_var).max()
    d_th = ub.th_diff(te, he, w_te, w_he) if te is not None else 0.0
    print("%s %s, %d cells: VAR %.3e (bound %.1e), exit time / last step size %.3e (bound %s), Nstp %s" %
          (name, run, n, d_var, ub.VAR_RTOL[(name, run)], d_th, ub.TH_RTOL.get((name, run)), stats[:3, 2].tolist()))
    assert np.array_equal(ierr, w_ierr), (ierr, w_ierr)
    assert np.array_equal(stats, w_st), "the counters differ from the oracle's"
    assert d_var <= ub.VAR_RTOL[(name, run)]
    if te is not None:
        assert d_th <= ub.TH_RTOL[(name, run)]


def _same(a, b):
    (ra, ta), (rb, tb) = a, b
    return np.array_equal(ra.var, rb.var) and np.array_equal(ra.ierr, rb.ierr) and np.array_equal(ra.stats, rb.stats) and np.array_equal(ta, tb)


@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("name", DEMO_NAMES)
def test_integrate_ex_and_integrate_device_against_the_oracle(chem, name, n):
    """Host-buffer and device-buffer entries at 1, 3 and 65 cells.  The caller's output arrays have one row more than the call and every entry is
    poisoned: the rows of the call are written entry by entry, the row behind them is untouched."""
    import torch
    mid, _ = chem._mech_id(name)
    nvar = chem.DIMS[name][0]
    V, F, K = uc.batch(name, _golden(name), n)
    out, ierr, stats, th = np.full((n + 1, nvar), POISON_D), np.full(n + 1, POISON_I, np.int32), np.full((n + 1, 8), POISON_I, np.int32), np.full((n + 1, 3), POISON_D)
    rc = chem.lib().mistra_chem_integrate_ex(mid, n, V.ctypes.data_as(_dp), F.ctypes.data_as(_dp), K.ctypes.data_as(_dp), 0.0, 10.0, out.ctypes.data_as(_dp),
                                            ierr.ctypes.data_as(_ip), stats.ctypes.data_as(_ip), th.ctypes.data_as(_dp))
    assert rc == 0, chem.lib().mistra_chem_last_error()
    for a, p in ((out, POISON_D), (ierr, POISON_I), (stats, POISON_I), (th, POISON_D)):
        assert (a[n] == p).all(), "the row behind the call was written"
        assert not (a[:n] == p).any(), "an entry of the call's rows was not written"
    _check(name, "base", out[:n], ierr[:n], stats[:n], th[:n, 0], th[:n, 1])
    # the device entry on caller-owned tensors gives the host entry's bits
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    d_out = torch.full((n + 1, nvar), POISON_D, dtype=torch.float64, device=dev)
    d_ierr = torch.full((n + 1,), POISON_I, dtype=torch.int32, device=dev)
    d_stats = torch.full((n + 1, 8), POISON_I, dtype=torch.int32, device=dev)
    d_th = torch.full((n + 1, 2), POISON_D, dtype=torch.float64, device=dev)
    chem.integrate_into(name, T(V), T(F), T(K), d_out[:n], d_ierr[:n], d_stats[:n], 0.0, 10.0, texit_hexit=d_th[:n])
    torch.cuda.synchronize()
    for a, p, host in ((d_out, POISON_D, out), (d_ierr, POISON_I, ierr), (d_stats, POISON_I, stats), (d_th, POISON_D, th[:, :2])):
        a = a.cpu().numpy()
        assert (a[n] == p).all(), "the row behind the device call was written"
        assert np.array_equal(a[:n], host[:n]), "the device entry differs from the host entry"
    if n == 3:      # ... and through chem.integrate under the slot's other names
        for alias in ("user%d" % (mid - 3), mid):
            assert np.array_equal(chem.integrate(alias, V, F, K).var, out[:n])
        assert name + ": nt=" in chem.describe(name)


@pytest.mark.parametrize("name", DEMO_NAMES)
def test_first_step_dump_is_bit_exact(chem, name):
    from mistra_amd import mechtab
    from oracle.oracle import Oracle
    o, t = Oracle(name), mechtab.load(name)
    V, F, K = uc.batch(name, _golden(name), 3)
    d = chem.debug_first_step(name, V, F, K)
    for i in range(3):
        assert d.h[i, 0] == 1.0e-3
        assert np.array_equal(d.fcn0[i], o.fun(V[i], F[i], K[i])), "Fun differs from the oracle"
        G = -o.jac_sp(V[i], F[i], K[i])
        G[t.diag] += 1.0 / (1.0e-3 * 0.43586652150845899941601945119356)
        assert np.array_equal(d.ghimj[i], G) and np.array_equal(np.signbit(d.ghimj[i]), np.signbit(G)), "the prepared Ghimj differs from the oracle"
    _check(name, "base", d.var, d.ierr, d.stats)


@pytest.mark.parametrize("run", ["rtol_1e-5", "vector_tol"])
@pytest.mark.parametrize("name", DEMO_NAMES)
def test_options_and_rosenbrock_with_ros3(chem, name, run):
    """set_options against the restatement of Rosenbrock_x over the oracle's routines; the per-call entries (host and device) with the same options
    give those bits without options in force; Rodas3 is a method a user slot does not have."""
    import torch
    V, F, K = uc.batch(name, _golden(name), 3)
    ipar, rpar, atol, rtol = ub.options_for(name, run)
    chem.set_options(name, ipar, rpar, atol, rtol)
    got = chem.get_options(name)
    assert np.array_equal(got.ipar, ipar) and np.array_equal(got.rtol, rtol if run == "vector_tol" else np.full_like(rtol, rtol[0]))
    res, th = chem.integrate_ex(name, V, F, K, 0.0, 10.0)
    _check(name, run, res.var, res.ierr, res.stats, th[:, 0], th[:, 1])
    chem.clear_options(name)
    assert chem.get_options(name) is None
    assert _same(chem.rosenbrock(name, V, F, K, 0.0, 10.0, ipar, rpar, atol, rtol), (res, th)), "rosenbrock_ex differs from the options in force"
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    d_res, d_th = chem.rosenbrock(name, T(V), T(F), T(K), 0.0, 10.0, ipar, rpar, atol, rtol)
    torch.cuda.synchronize()
    assert np.array_equal(d_res.var.cpu().numpy(), res.var) and np.array_equal(d_res.ierr.cpu().numpy(), res.ierr)
    assert np.array_equal(d_res.stats.cpu().numpy(), res.stats) and np.array_equal(d_th.cpu().numpy(), th[:, :2])
    # without options in force the product kernel is back
    _check(name, "base", *chem.integrate(name, V, F, K))
    bad = ipar.copy()
    bad[3] = 4
    for args in ((V, F, K), (T(V), T(F), T(K))):
        with pytest.raises(chem.MistraChemError, match=r"user mechanism slot \d \(%s\) has no kernel for this Rosenbrock method" % name):
            chem.rosenbrock(name, *args, 0.0, 10.0, bad, rpar, atol, rtol)
    with pytest.raises(chem.MistraChemError, match="has no step-control trace"):
        chem.rosenbrock_trace(name, V, F, K, 0.0, 10.0, ipar, rpar, atol, rtol)


@pytest.mark.parametrize("name", DEMO_NAMES)
def test_per_cell_first_step(chem, name):
    """mistra_chem_integrate_hstart_ex (and the device entry's hstart) against the oracle's integrate_batch(hstart=): every cell starts at the last step
    size of its base run"""
    import torch
    V, F, K = uc.batch(name, _golden(name), 3)
    h = ub.oracle_run(name, "base")[4].copy()
    res, th = chem.integrate_ex(name, V, F, K, 0.0, 10.0, hstart=h)
    _check(name, "hstart", res.var, res.ierr, res.stats)
    assert not np.array_equal(res.stats, ub.oracle_run(name, "base")[2]), "the first step size was not taken"
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    out, ierr, stats = torch.empty((3, V.shape[1]), dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.int32, device=dev), torch.empty((3, 8), dtype=torch.int32, device=dev)
    chem.integrate_into(name, T(V), T(F), T(K), out, ierr, stats, 0.0, 10.0, hstart=T(h))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), res.var) and np.array_equal(stats.cpu().numpy(), res.stats)


@pytest.mark.parametrize("name", DEMO_NAMES)
def test_a_batch_split_over_two_device_slots_is_bitwise_the_same(chem, name):
    V, F, K = uc.batch(name, _golden(name), 65)
    one = chem.integrate_ex(name, V, F, K, 0.0, 10.0)
    chem.init_devices([0, 0])
    assert chem.device_count() == 2
    assert _same(chem.integrate_ex(name, V, F, K, 0.0, 10.0), one)
    chem.singular_rows(name, 64)      # (the last cell lives on the second slot; no cell met a zero pivot, the rows themselves mean nothing)


def _permuted_table(name, seed=3):
    """The table with its reactions renumbered by a seeded permutation: the same sizes, the same sums in the same order — and other contents in every
    list that names a reaction -> (file bytes, perm) with new reaction perm[r] = old reaction r"""
    from mistra_amd import mechderive, mechtab
    t = mechtab.load(name)
    perm = np.random.default_rng(seed).permutation(t.nreact)      # old r -> new perm[r]
    inv = np.argsort(perm)                                         # new q -> old inv[q]
    a_ptr, a_fac = [0], []
    for q in range(t.nreact):
        a_fac += t.a_fac[t.a_ptr[inv[q]]:t.a_ptr[inv[q] + 1]].tolist()
        a_ptr.append(len(a_fac))
    tab = {k: getattr(t, k) for k in ("nvar", "nfix", "nreact", "nnz", "crow", "icol", "diag", "b_ptr", "b_fac", "vd_ptr", "vd_coef", "jv_ptr", "jv_idx", "jv_coef", "consts")}
    tab.update(a_ptr=np.array(a_ptr, np.int32), a_fac=np.array(a_fac, np.int32), b_rct=perm[t.b_rct].astype(np.int32), vd_idx=perm[t.vd_idx].astype(np.int32))
    return mechderive.table_bytes(tab), perm


def test_a_table_of_the_same_sizes_and_other_contents_runs_and_other_sizes_are_refused(chem, tmp_path):
    """The kernels depend on a table's sizes only: the slot of demo_a runs demo_a with its reactions renumbered (the schedule is compiled at init) and,
    fed the rate constants in that numbering, gives demo_a's bits.  A table of other sizes under the slot's name fails the init with the
    existing text."""
    name = "demo_a"
    V, F, K = uc.batch(name, _golden(name), 3)
    want = chem.integrate_ex(name, V, F, K, 0.0, 10.0)
    src = os.path.join(REPO, "mistra_amd", "mech")
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    raw, perm = _permuted_table(name)
    assert raw != open(os.path.join(src, name + ".mech"), "rb").read()
    (tmp_path / (name + ".mech")).write_bytes(raw)
    Kp = np.empty_like(K)
    Kp[:, perm] = K
    old = os.environ.get("MISTRA_MECH_DIR")
    try:
        os.environ["MISTRA_MECH_DIR"] = str(tmp_path)
        chem.finalize()
        chem.init(0)
        assert _same(chem.integrate_ex(name, V, F, Kp, 0.0, 10.0), want)
        shutil.copy(os.path.join(src, "demo_g.mech"), tmp_path / (name + ".mech"))
        chem.finalize()
        with pytest.raises(chem.MistraChemError, match="demo_a: mechanism table does not match the compiled kernel sizes"):
            chem.init(0)
        # a directory WITHOUT the slot's table (a caller's own MISTRA_MECH_DIR from before the library had slots): the library comes up, gas, aer and
        # tot and the other slot run, and the slot's entries say what is missing
        os.remove(tmp_path / (name + ".mech"))
        g = load_golden("gas")
        chem.init(0)
        assert chem.integrate("gas", g["var_in"][:2], g["fix"][:2], g["rconst"][:2]).ierr.tolist() == [1, 1]
        Vg, Fg, Kg = uc.batch("demo_g", _golden("demo_g"), 3)
        _check("demo_g", "base", *chem.integrate("demo_g", Vg, Fg, Kg))
        with pytest.raises(chem.MistraChemError, match=r"user mechanism slot 1: demo_a.mech was not in the mechanism directory"):
            chem.integrate_ex(name, V, F, K, 0.0, 10.0)
        assert chem.describe(name) == ""
    finally:
        if old is None:
            del os.environ["MISTRA_MECH_DIR"]
        else:
            os.environ["MISTRA_MECH_DIR"] = old
        chem.finalize()
        chem.init(0)
    assert _same(chem.integrate_ex(name, V, F, K, 0.0, 10.0), want)


_NOSLOTS_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mistra_amd import chem
assert chem.lib().mistra_chem_user_mechs() == 0 and chem.user_mechs() == []
z = dict(np.load(sys.argv[2]))
out = {}
for mech in ("gas", "aer", "tot"):
    res, th = chem.integrate_ex(mech, z[mech + "_var"], z[mech + "_fix"], z[mech + "_rconst"], 0.0, 10.0)
    out.update({mech + "_var": res.var, mech + "_ierr": res.ierr, mech + "_stats": res.stats, mech + "_th": th})
np.savez(sys.argv[3], **out)
"""


def test_gas_aer_tot_give_the_bits_of_a_library_without_user_slots(chem, golden, tmp_path):
    """The shipped mechanisms beside the user slots: VAR, IERR, the counters and exit time / step sizes are, bit for bit, those of the SAME sources built
    without user slots (the twin library the build links beside the product, run here in a process of its own), before and after the user slots
    have run and had options in force; and they match the captured reference calls as tests/test_gpu_parity.py holds them."""
    import subprocess
    import sys
    from mistra_amd.build import LIB_NOSLOTS
    from parity_bounds import PARITY_RTOL
    assert os.path.exists(LIB_NOSLOTS), "the build links %s beside a library with user slots" % LIB_NOSLOTS
    cells = {mech: {k: np.ascontiguousarray(golden[mech][k][:3]) for k in ("var_in", "fix", "rconst")} for mech in MECHS}
    np.savez(tmp_path / "in.npz", **{mech + "_" + k.replace("var_in", "var"): v for mech in MECHS for k, v in cells[mech].items()})
    (tmp_path / "noslots.py").write_text(_NOSLOTS_SCRIPT)
    env = dict(os.environ, MISTRA_CHEM_LIB=LIB_NOSLOTS, MISTRA_MECH_DIR=os.path.join(REPO, "mistra_amd", "mech"))
    subprocess.run([sys.executable, str(tmp_path / "noslots.py"), REPO, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True, env=env, timeout=120)
    z = dict(np.load(tmp_path / "out.npz"))

    def run(mech):
        c = cells[mech]
        return chem.integrate_ex(mech, c["var_in"], c["fix"], c["rconst"], 0.0, 10.0)

    def same_as_noslots(mech, got):
        res, th = got
        return (np.array_equal(res.var, z[mech + "_var"]) and np.array_equal(res.ierr, z[mech + "_ierr"]) and np.array_equal(res.stats, z[mech + "_stats"])
                and np.array_equal(th, z[mech + "_th"]))

    for mech in MECHS:
        got = run(mech)
        assert same_as_noslots(mech, got), "%s: the library with user slots differs from the one without" % mech
        g = golden[mech]
        assert rel_diff(got[0].var, g["var_out"][:3]).max() <= PARITY_RTOL[mech] and np.array_equal(got[0].stats, g["stats"][:3])
    for name in DEMO_NAMES:
        V, F, K = uc.batch(name, _golden(name), 3)
        chem.set_options(name, *ub.options_for(name, "rtol_1e-5"))
        chem.integrate_ex(name, V, F, K, 0.0, 10.0)
    for mech in MECHS:
        assert chem.get_options(mech) is None
        assert same_as_noslots(mech, run(mech)), "%s: changed by runs of the user slots" % mech
