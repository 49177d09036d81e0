"""The size classes' edges of the user mechanism slots on the GPU (-m gpu): the four tables of tests/user_edge_cases.py in the slots of the two twin
libraries mistra_amd/build.py: build_edge_twins links.  One child process per twin (MISTRA_CHEM_LIB and MISTRA_MECH_DIR in its environment) runs every
kernel of the twin's two tables and hands the results back through an .npz; the tests hold them to the oracle on the SAME table.  Bounds:
tests/user_edge_bounds.py (the oracle's own spread under re-association, x10, held by tests/test_user_edges.py together with the condition that no
variant changes a counter on the test cells — so IERR and all eight counters must be identical here).

Per table the child runs
  VARIANT 2   the first-step dump on cells 0, 16 and 31
  VARIANT 0   mistra_chem_integrate_ex at 1, 3 and 65 cells into poisoned arrays one row longer than the call, and the device-buffer entry on
              caller-owned tensors
  VARIANT 3   Rosenbrock_x with RelTol = 1e-5, then a plain call with no options in force
  VARIANT 0   two crafted zero pivots (the method of tests/test_gpu_phases.py::test_zero_pivot_paths), in the first and in the last row the method
              applies to: rows 2 and 62 of 64 (edge_g64, both tail rows: it has no others), 2 and 126 of 128 (edge_a128), 2 and 127 of 129 (edge_a129),
              0 and 416 of 417 (edge_t417)
and the second twin tot's product kernel on edge_t417's cells (printed beside edge_t417's figures, not asserted)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import user_edge_bounds as eb
import user_edge_cases as ec
import user_mech_bounds as ub
from conftest import REPO, load_golden, rel_diff
from test_gpu_phases import C21, C31, C32, GAMMA, P, _first_order_losses, emu      # noqa: F401  (the emulator fixture and the constants of the phase tests)

pytestmark = pytest.mark.gpu
POISON_D, POISON_I = -7.77e77, -777
BATCHES = (1, 3, 65)
TWIN_OF = {name: twin for twin, names in ec.TWINS.items() for name in names}
ZP_TIN, ZP_TOUT = 0.0, 1.5e-3

_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import ctypes as C
import torch
from mistra_amd import chem
names = sys.argv[4].split(",")
assert chem.user_mechs() == names, chem.user_mechs()
z = dict(np.load(sys.argv[2]))
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
PD, PI = %r, %r
chem.init(0)
dev = torch.device("cuda", 0)
T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
out = {}
for name in names:
    mid, _ = chem._mech_id(name)
    nvar = chem.DIMS[name][0]
    V, F, K = z[name + "_var"], z[name + "_fix"], z[name + "_rconst"]
    idx = lambda n: [i %% 3 for i in range(n)]
    # VARIANT 2: the first-step dump
    d = chem.debug_first_step(name, V, F, K)
    for k in d._fields:
        out["%%s_dump_%%s" %% (name, k)] = getattr(d, k)
    # VARIANT 0: host and device entries into poisoned arrays one row longer than the call
    for n in %r:
        v, f, k = (np.ascontiguousarray(a[idx(n)]) for a in (V, F, K))
        o, ierr, st, th = np.full((n + 1, nvar), PD), np.full(n + 1, PI, np.int32), np.full((n + 1, 8), PI, np.int32), np.full((n + 1, 3), PD)
        rc = chem.lib().mistra_chem_integrate_ex(mid, n, v.ctypes.data_as(dp), f.ctypes.data_as(dp), k.ctypes.data_as(dp), 0.0, 10.0, o.ctypes.data_as(dp),
                                                ierr.ctypes.data_as(ip), st.ctypes.data_as(ip), th.ctypes.data_as(dp))
        assert rc == 0, chem.lib().mistra_chem_last_error()
        d_o = torch.full((n + 1, nvar), PD, dtype=torch.float64, device=dev)
        d_ierr = torch.full((n + 1,), PI, dtype=torch.int32, device=dev)
        d_st = torch.full((n + 1, 8), PI, dtype=torch.int32, device=dev)
        d_th = torch.full((n + 1, 2), PD, dtype=torch.float64, device=dev)
        chem.integrate_into(name, T(v), T(f), T(k), d_o[:n], d_ierr[:n], d_st[:n], 0.0, 10.0, texit_hexit=d_th[:n])
        torch.cuda.synchronize()
        for key, a in (("var", o), ("ierr", ierr), ("stats", st), ("th", th), ("dvar", d_o), ("dierr", d_ierr), ("dstats", d_st), ("dth", d_th)):
            out["%%s_n%%d_%%s" %% (name, n, key)] = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    # VARIANT 3: Rosenbrock_x's options, then no options in force
    res, th = chem.rosenbrock(name, V, F, K, 0.0, 10.0, z["ipar"], z["rpar"], z[name + "_atol"], z[name + "_rtol"])
    out.update({name + "_opt_var": res.var, name + "_opt_ierr": res.ierr, name + "_opt_stats": res.stats, name + "_opt_th": th})
    assert chem.get_options(name) is None
    res, th = chem.integrate_ex(name, V, F, K, 0.0, 10.0)
    out.update({name + "_again_var": res.var, name + "_again_ierr": res.ierr, name + "_again_stats": res.stats, name + "_again_th": th})
    # the crafted zero pivots
    for case in ("first", "last"):
        res = chem.integrate(name, V[:1], F[:1], z["%%s_zp_%%s" %% (name, case)], %r, %r)
        out.update({"%%s_zp_%%s_var" %% (name, case): res.var, "%%s_zp_%%s_ierr" %% (name, case): res.ierr, "%%s_zp_%%s_stats" %% (name, case): res.stats,
                    "%%s_zp_%%s_rows" %% (name, case): chem.singular_rows(name, 0)})
    if name == "edge_t417":      # tot's product kernel (512 threads, dense tail block, chain passes) on the same cells
        res, th = chem.integrate_ex("tot", V, F, K, 0.0, 10.0)
        out.update({"tot_var": res.var, "tot_ierr": res.ierr, "tot_stats": res.stats})
np.savez(sys.argv[3], **out)
""" % (POISON_D, POISON_I, BATCHES, ZP_TIN, ZP_TOUT)


def _cells(name):
    return ec.cut_inputs(name, load_golden(ec.EDGES[name][0]))


def _zero_pivot_rates(name):
    """-> {"first" | "last": (species, RCONST [1, NREACT])}: all rate constants zero but one first-order loss with k = -1 / (H gamma), H = 1e-3, of the
    lowest and of the highest species the method applies to"""
    t = ec.tables(name)
    losses = {}
    for r, s in _first_order_losses(t):
        losses.setdefault(s, r)
    out = {}
    for case, s in (("first", min(losses)), ("last", max(losses))):
        K = np.zeros((1, t.nreact))
        K[0, losses[s]] = -1.0 / (1.0e-3 * GAMMA[0])
        out[case] = (s, K)
    return out


_results = {}


def _twin_results(twin, tmp_path_factory):
    """Runs the twin's child process once -> its .npz as a dict"""
    if twin not in _results:
        assert None not in _results.values(), "an earlier child process did not finish: no further one is started"
        from mistra_amd.build import edge_twin_lib
        ec.ensure_tables()
        lib = edge_twin_lib(twin)
        assert os.path.exists(lib), "the build links %s" % lib
        tmp = tmp_path_factory.mktemp(twin)
        inp = {}
        for name in ec.TWINS[twin]:
            V, F, K = _cells(name)
            ipar, rpar, atol, rtol = eb.options_for(name, "rtol_1e-5")
            inp.update({name + "_var": V, name + "_fix": F, name + "_rconst": K, "ipar": ipar, "rpar": rpar, name + "_atol": atol, name + "_rtol": rtol})
            for case, (_, Kz) in _zero_pivot_rates(name).items():
                inp["%s_zp_%s" % (name, case)] = Kz
        np.savez(tmp / "in.npz", **inp)
        (tmp / "child.py").write_text(_CHILD)
        env = dict(os.environ, MISTRA_CHEM_LIB=lib, MISTRA_MECH_DIR=ec.EDGE_DIR)
        _results[twin] = None
        # (a child that fails, is killed or runs into its time limit leaves None behind: no other child is started after it, on the same card)
        subprocess.run([sys.executable, str(tmp / "child.py"), REPO, str(tmp / "in.npz"), str(tmp / "out.npz"), ",".join(ec.TWINS[twin])], check=True, env=env,
                       timeout=120)
        _results[twin] = dict(np.load(tmp / "out.npz"))
    assert _results[twin] is not None, "the child process of %s did not finish" % twin
    return _results[twin]


@pytest.fixture()
def got(request, tmp_path_factory):
    """the child's results of the test's table, keys without the table's name"""
    name = request.node.callspec.params["name"]
    z = _twin_results(TWIN_OF[name], tmp_path_factory)
    return {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "_")}


def _check(name, run, var, ierr, stats, te=None, he=None):
    n = var.shape[0]
    idx = [i % len(ec.CELLS) for i in range(n)]
    w_var, w_ierr, w_st, w_te, w_he = (a[idx] for a in eb.oracle_run(name, run))
    d_var = rel_diff(var, w_var).max()
    d_th = ub.th_diff(te, he, w_te, w_he) if te is not None else 0.0
    print("%s %s, %d cells: VAR %.3e (bound %.1e), exit time / last step size %.3e (bound %.1e), Nstp %s" %
          (name, run, n, d_var, eb.VAR_RTOL[(name, run)], d_th, eb.TH_RTOL[(name, run)], stats[:3, 2].tolist()))
    assert np.array_equal(ierr, w_ierr), (ierr, w_ierr)
    assert np.array_equal(stats, w_st), "the counters differ from the oracle's: %s, oracle %s" % (stats[:3].tolist(), w_st[:3].tolist())
    assert d_var <= eb.VAR_RTOL[(name, run)]
    if te is not None:
        assert d_th <= eb.TH_RTOL[(name, run)]


@pytest.mark.parametrize("name", ec.NAMES)
def test_first_step_dump(got, emu, name):      # noqa: F811
    """H = 1e-3; Fun and the prepared Ghimj bit for bit against the oracle, sign bits included; the factors, the pivots' reciprocals and K1..K3 bit
    for bit against the emulated kernel programs at the table's workgroup size; the factors against the oracle's KppDecomp, tail rows un-scaled, within
    1e-10 of the row maximum (the bound of tests/test_schedule.py)."""
    o, t = ec.oracle(name), ec.tables(name)
    V, F, K = _cells(name)
    h_emu = emu.emu_create(ec.path(name).encode(), ec.TRAITS[name]["NT"])
    assert h_emu
    tail_h = emu.emu_tail_h(h_emu)
    assert tail_h == t.nvar - 64 * ec.TRAITS[name]["TAIL_REGS"]
    worst = 0.0
    for i in range(len(ec.CELLS)):
        v, f, k = (np.ascontiguousarray(x[i]) for x in (V, F, K))
        H = got["dump_h"][i, 0]
        assert H == 1.0e-3
        fcn0 = o.fun(v, f, k)
        assert np.array_equal(got["dump_fcn0"][i], fcn0) and np.array_equal(np.signbit(got["dump_fcn0"][i]), np.signbit(fcn0)), "Fun differs from the oracle"
        G = -o.jac_sp(v, f, k)
        G[t.diag] += 1.0 / (1.0e-3 * GAMMA[0])
        assert np.array_equal(got["dump_ghimj"][i], G) and np.array_equal(np.signbit(got["dump_ghimj"][i]), np.signbit(G)), "the prepared Ghimj differs from the oracle"
        lu = np.ascontiguousarray(got["dump_lu"][i])
        lu_emu, r_emu, x = G.copy(), np.empty(t.nvar), fcn0.copy()
        assert emu.emu_lu(h_emu, P(lu_emu), P(r_emu), P(x)) == 0
        assert np.array_equal(lu, lu_emu), "factors differ from the emulated kernel programs"
        assert np.array_equal(got["dump_r"][i], r_emu), "pivot reciprocals differ from the emulated kernel programs"
        lu_ref, ier = o.decomp(G)
        assert ier == 0
        lu_un = lu.copy()
        for r in range(tail_h, t.nvar):
            lu_un[t.diag[r] + 1:t.crow[r + 1]] *= lu_un[t.diag[r]]
        rowmax = np.repeat(np.array([np.abs(lu_ref[t.crow[r]:t.crow[r + 1]]).max() for r in range(t.nvar)]), np.diff(t.crow))
        worst = max(worst, (np.abs(lu_un - lu_ref) / rowmax).max())
        assert (np.abs(lu_un - lu_ref) / rowmax).max() <= 1e-10
        k1, k2, k3 = got["dump_k1"][i], got["dump_k2"][i], got["dump_k3"][i]
        fcn = o.fun(v + k1, f, k)
        e1 = x.copy()
        assert emu.emu_solve_backward(h_emu, P(lu), P(e1)) == 0
        e2 = np.ascontiguousarray((fcn + (C21 / H) * k1) + (H * GAMMA[1]) * 0.0)
        assert emu.emu_solve_kernel_form(h_emu, P(lu), P(e2)) == 0
        e3 = np.ascontiguousarray(((fcn + (C31 / H) * k1) + (C32 / H) * k2) + (H * GAMMA[2]) * 0.0)
        assert emu.emu_solve_kernel_form(h_emu, P(lu), P(e3)) == 0
        assert np.array_equal(k1, e1) and np.array_equal(k2, e2) and np.array_equal(k3, e3), "K vectors differ from the emulated solve programs"
    print("%s: Fun and Ghimj bit-exact, factors and K1..K3 the emulator's bits at %d threads (tail from row %d); factors vs KppDecomp %.2e of the row maximum"
          % (name, ec.TRAITS[name]["NT"], tail_h, worst))
    # the integration the dump kernel carried to its end
    _check(name, "base", got["dump_var"], got["dump_ierr"], got["dump_stats"])


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("name", ec.NAMES)
def test_integrate_ex_and_the_device_entry_against_the_oracle(got, name, n):
    """The call's rows are written entry by entry, the row behind them is untouched; IERR and the counters are the oracle's, VAR and exit time / last
    step size within the bounds; the device entry on caller-owned tensors gives the host entry's bytes."""
    out, ierr, stats, th = (got["n%d_%s" % (n, k)] for k in ("var", "ierr", "stats", "th"))
    assert out.shape == (n + 1, ec.SIZES[name][0])
    for a, p in ((out, POISON_D), (ierr, POISON_I), (stats, POISON_I), (th, POISON_D)):
        assert (a[n] == p).all(), "the row behind the call was written"
        assert not (a[:n] == p).any(), "an entry of the call's rows was not written"
    _check(name, "base", out[:n], ierr[:n], stats[:n], th[:n, 0], th[:n, 1])
    for key, p, host in (("dvar", POISON_D, out), ("dierr", POISON_I, ierr), ("dstats", POISON_I, stats), ("dth", POISON_D, th[:, :2])):
        a = got["n%d_%s" % (n, key)]
        assert (a[n] == p).all(), "the row behind the device call was written"
        assert a[:n].tobytes() == np.ascontiguousarray(host[:n]).tobytes(), "the device entry differs from the host entry"


@pytest.mark.parametrize("name", ec.NAMES)
def test_rosenbrock_with_options_and_back(got, name):
    """Rosenbrock_x with RelTol = 1e-5 against ros_options_py.rosenbrock over the oracle; the plain call after it gives the base bytes again."""
    th = got["opt_th"]
    _check(name, "rtol_1e-5", got["opt_var"], got["opt_ierr"], got["opt_stats"], th[:, 0], th[:, 1])
    assert not np.array_equal(got["opt_stats"], eb.oracle_run(name, "base")[2]), "the options were not in force"
    for key in ("var", "ierr", "stats", "th"):
        assert got["again_" + key].tobytes() == np.ascontiguousarray(got["n3_" + key][:3]).tobytes(), "%s: the plain call after the options run differs from the base run" % key


@pytest.mark.parametrize("case", ["first", "last"])
@pytest.mark.parametrize("name", ec.NAMES)
def test_zero_pivot(got, name, case):
    """An exact zero on the diagonal of Ghimj at the first attempt: a failed decomposition, H halved, the step goes on.  IERR, the counters (Nsng
    among them) and the row mistra_chem_singular_rows reports are the oracle's.  edge_g64 has no head rows: both of its rows are found by the tail chain's path."""
    o, t = ec.oracle(name), ec.tables(name)
    V, F, _ = _cells(name)
    s, K = _zero_pivot_rates(name)[case]
    G = -o.jac_sp(V[0], F[0], K[0])
    G[t.diag] += 1.0 / (1.0e-3 * GAMMA[0])
    assert G[t.diag[s]] == 0.0      # the premise
    _, ier = o.decomp(G)
    assert ier == s + 1
    want, ierr, st = o.integrate_batch(V[:1], F[:1], K, ZP_TIN, ZP_TOUT)
    nsng = int(st[0, 7])
    assert int(ierr[0]) == 1 and nsng in (1, 2)      # (2: the halved step is accepted and leaves exactly 1e-3 to the interval's end, the zero comes back)
    tail_h = t.nvar - 64 * ec.TRAITS[name]["TAIL_REGS"]
    print("%s zero pivot in row %d of %d (%s row): counters %s" % (name, s, t.nvar, "tail" if s >= tail_h else "head", got["zp_%s_stats" % case].tolist()))
    assert np.array_equal(got["zp_%s_ierr" % case], ierr)
    assert np.array_equal(got["zp_%s_stats" % case], st), (got["zp_%s_stats" % case], st)
    assert got["zp_%s_rows" % case][:nsng].tolist() == [ier] * nsng      # (Ghimj is diagonal but for this one entry: no other pivot can vanish)
    assert np.allclose(got["zp_%s_var" % case], want, rtol=1e-9, atol=1e-300)


def test_edge_t417_beside_tots_product_kernel(tmp_path_factory):
    """Printed, not asserted: edge_t417 (256 threads, no dense tail block, no chain passes) and tot's product kernel (512 threads) on the same cells,
    each against the oracle, beside PARITY_RTOL["tot"]."""
    from parity_bounds import PARITY_RTOL
    z = _twin_results(TWIN_OF["edge_t417"], tmp_path_factory)
    w_var, _, w_st = eb.oracle_run("edge_t417", "base")[:3]
    print("edge_t417 vs oracle %.3e, tot product kernel vs oracle %.3e, edge_t417 vs tot product kernel %.3e (PARITY_RTOL[tot] %.1e); counters equal: %s" %
          (rel_diff(z["edge_t417_n3_var"][:3], w_var).max(), rel_diff(z["tot_var"], w_var).max(), rel_diff(z["edge_t417_n3_var"][:3], z["tot_var"]).max(),
           PARITY_RTOL["tot"], np.array_equal(z["tot_stats"], w_st)))
