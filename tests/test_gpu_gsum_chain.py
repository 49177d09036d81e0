"""Chain passes of the gather-sum machine on the GPU (-m gpu; schedule.hpp: GsumChain): tot's long Vdot sums run as broadcast-DPP chains on a
wave with no rows of its own.  The operators entry gives Fun_x and Jac_SP_x at any state: vdot and jvs are held to the oracle's Fun / Jac_SP
bit for bit (NaNs by position) at 1, 3 and 65 cells, on a captured cell, the all-zero state, and states with -0.0 or a NaN in a factor of a
reaction that feeds a 108-term species / of the reaction behind the 58-term Jacobian entry; outputs go into poisoned caller arrays one row
larger than the call.  One integration of three captured cells through the product kernel and one through the Rodas4 unit equal, byte for
byte, those of the twin library the build links without chain passes (run in a process of its own)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
MECH = "tot"
RODAS4 = 5


@pytest.fixture(scope="module")
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def states(golden):
    """the base states, computed once and left unchanged: name -> (var, fix, rconst) of one cell"""
    from mistra_amd import mechtab
    t = mechtab.load(MECH)
    g = golden[MECH]
    V, F, K = g["var_in"][0].copy(), g["fix"][0].copy(), g["rconst"][0].copy()
    nterm = np.diff(t.vd_ptr)
    s108 = int(np.argmax(nterm))
    assert nterm[s108] == 108
    # a variable species that is a factor of a reaction among the terms of the 108-term sum
    fac_v = next(int(f) for r in t.vd_idx[t.vd_ptr[s108]:t.vd_ptr[s108 + 1]] for f in t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]] if f < t.nvar)
    jterm = np.diff(t.jv_ptr)
    k58 = int(np.argmax(jterm))
    assert jterm[k58] == 58
    fac_j = next(int(f) for b in t.jv_idx[t.jv_ptr[k58]:t.jv_ptr[k58 + 1]] for f in t.b_fac[t.b_ptr[b]:t.b_ptr[b + 1]] if f < t.nvar)
    out = {"captured": (V, F, K), "zero": (np.zeros_like(V), F, K)}
    for label, fac in (("vdot108", fac_v), ("jvs58", fac_j)):
        for what, value in (("negzero", -0.0), ("nan", np.nan)):
            W = V.copy()
            W[fac] = value
            out["%s_%s" % (label, what)] = (W, F, K)
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def _T(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=torch.device("cuda", 0))


def _poison(shape):
    return (-(1.0e3 + np.arange(int(np.prod(shape))))).astype(np.float64).reshape(shape)


def _same_but_nans(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaNs in other positions" % what
    assert got[~nan].tobytes() == want[~nan].tobytes(), "%s: differs from the oracle in %d entries" % (
        what, int((got[~nan].view(np.uint64) != want[~nan].view(np.uint64)).sum()))


@pytest.mark.parametrize("n", [1, 3, 65])
def test_vdot_and_jvs_are_the_oracles_bits(chem, oracles, states, n):
    import torch
    names = list(states)
    pick = [names[i % len(names)] for i in range(n)] if n > 1 else None
    batches = [pick] if pick else [[nm] for nm in names]      # one cell: every state in a call of its own
    nvar, nnz = chem.DIMS[MECH][0], chem.DIMS[MECH][3]
    orc = oracles[MECH]
    for batch in batches:
        V, F, K = (np.array([states[nm][i] for nm in batch]) for i in range(3))
        m = len(batch)
        want_v = np.array([orc.fun(V[c], F[c], K[c]) for c in range(m)])
        want_j = np.array([orc.jac_sp(V[c], F[c], K[c]) for c in range(m)])
        pv, pj = _poison((m + 1, nvar)), _poison((m + 1, nnz))
        dv, dj = _T(pv), _T(pj)
        chem.ops(MECH, _T(V), _T(F), _T(K), True, True, vdot=dv, jvs=dj)
        torch.cuda.synchronize()
        gv, gj = dv.cpu().numpy(), dj.cpu().numpy()
        assert gv[m:].tobytes() == pv[m:].tobytes() and gj[m:].tobytes() == pj[m:].tobytes(), "the row behind the call's was written"
        print(batch, "vdot entries differing from the oracle:", int((gv[:m].view(np.uint64) != want_v.view(np.uint64)).sum()),
              "jvs:", int((gj[:m].view(np.uint64) != want_j.view(np.uint64)).sum()), "NaNs:", int(np.isnan(want_v).sum()), int(np.isnan(want_j).sum()))
        _same_but_nans(gv[:m], want_v, "vdot %s" % batch)
        _same_but_nans(gj[:m], want_j, "jvs %s" % batch)
        if any("nan" in nm for nm in batch):
            assert np.isnan(want_v).any() or np.isnan(want_j).any(), "the NaN reaches a sum"


_TWIN_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mistra_amd import chem
z = dict(np.load(sys.argv[2]))
res, th = chem.integrate_ex("tot", z["var"], z["fix"], z["rconst"], 0.0, 10.0)
r4, th4 = chem.rosenbrock("tot", z["var"], z["fix"], z["rconst"], 0.0, 10.0, ipar=[0, 0, 0, %d])
np.savez(sys.argv[3], var=res.var, ierr=res.ierr, stats=res.stats, th=th, var4=r4.var, ierr4=r4.ierr, stats4=r4.stats, th4=th4)
""" % RODAS4


def test_integrations_give_the_bytes_of_the_build_without_chain_passes(chem, golden, tmp_path):
    from mistra_amd.build import LIB_NOCHAIN
    assert os.path.exists(LIB_NOCHAIN), "the build links %s beside the product" % LIB_NOCHAIN
    g = golden[MECH]
    V, F, K = (np.ascontiguousarray(g[k][:3]) for k in ("var_in", "fix", "rconst"))
    np.savez(tmp_path / "in.npz", var=V, fix=F, rconst=K)
    (tmp_path / "twin.py").write_text(_TWIN_SCRIPT)
    env = dict(os.environ, MISTRA_CHEM_LIB=LIB_NOCHAIN, MISTRA_MECH_DIR=os.path.join(REPO, "mistra_amd", "mech"))
    subprocess.run([sys.executable, str(tmp_path / "twin.py"), REPO, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True, env=env, timeout=120)
    z = dict(np.load(tmp_path / "out.npz"))
    res, th = chem.integrate_ex(MECH, V, F, K, 0.0, 10.0)
    r4, th4 = chem.rosenbrock(MECH, V, F, K, 0.0, 10.0, ipar=[0, 0, 0, RODAS4])
    assert res.ierr.tolist() == [1, 1, 1] and r4.ierr.tolist() == [1, 1, 1]
    for got, key in ((res.var, "var"), (res.ierr, "ierr"), (res.stats, "stats"), (th, "th"), (r4.var, "var4"), (r4.ierr, "ierr4"), (r4.stats, "stats4"), (th4, "th4")):
        assert got.tobytes() == z[key].tobytes(), "%s differs from the build without chain passes" % key
