"""Table streams that start on a ring filled ahead of them (-m gpu): ros3_kernel.hip's gsum_run_bar and the barrier form of the head
sweeps fill their look-ahead ring in front of a barrier, gsum_run_pair's second program takes its ring over from the stream before.  What such a ring holds at its second and later uses — after a rejected attempt, a halved step, an
early exit of a neighbouring launch — the first-step dump tests do not reach.  Here launches of 8 cells mix the paths through the step
loop, on the product kernel and on the options kernel (the same executors), for all three mechanisms:

    launch A, 0 -> 1.5e-3 s:   captured cells (aer, tot: 50 to 100 short steps each), one crafted zero pivot (Nsng = 1, the step goes on),
                               six in a row (IERR = -8), a NaN cell (IERR = -7);
    launch B, 0 -> 10 s:       captured cells and the NaN cell under the Max_no_steps hook (IERR = -6);
    launch D, 0 -> 1.5e-3 s:   launch A's cells under that hook: IERR = -6 (the zero-pivot cell, which carries on past its failed decomposition
                               into the bound; the NaN cell; aer, tot: captured cells) next to -8 and (gas, aer) cells that finish, in one launch;
    launch C:                  steps rejected AFTER accepted ones (Nrej > 0), on the inputs tests/parity_bounds.py: REJECT_CASES picked because
                               every re-association of the oracle leaves their IERR and /Statistics/ alone — gas: 0.5 -> 0 s (TOUT < TIN);
                               tot: 0.02 -> 0 s (TOUT < TIN, IERR = -7 from a finite state); aer: 0 -> 3600 s (no backward aer input is that
                               stable: parity_bounds.py).

A launch has ONE interval and ONE step limit, which is why the paths are spread over four launches and not one; the crafted cells stay
out of the 10 s launch (a loss with a negative rate constant grows out of the number range there).

Checked per launch: IERR and /Statistics/ identical to the oracle's; values within the bounds of tests/parity_bounds.py (PARITY_RTOL;
launch C: REJECT_RTOL of its case; cells the oracle leaves finite); the same launch enqueued twice on one stream without a
synchronisation between gives bit-identical outputs, also a tot launch directly behind a gas launch.  (The repeat catches ring contents that
depend on what ran before; a ring primed with the same wrong row every time is the oracle comparison's to catch.)"""
import numpy as np
import pytest

import ros_options_py as R
from conftest import MECHS, rel_diff
import parity_bounds as pb
from parity_bounds import PARITY_RTOL

pytestmark = pytest.mark.gpu
GAMMA1 = 0.43586652150845899941601945119356e+00      # Ros3_x (gas.f:1616)


@pytest.fixture()
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    yield c
    c.debug_set_max_steps(0)
    for mech in MECHS:
        c.clear_options(mech)


def _first_order_losses(t):
    """(reaction, species) for reactions A = k*V(s) whose only effect on s is the loss -A, one per species (as tests/test_gpu_phases.py)"""
    out, seen = [], set()
    for r in range(t.nreact):
        fac = t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]]
        if len(fac) != 1 or fac[0] >= t.nvar or int(fac[0]) in seen:
            continue
        s = int(fac[0])
        terms = [(int(t.vd_idx[p]), float(t.vd_coef[p])) for p in range(t.vd_ptr[s], t.vd_ptr[s + 1])]
        if (r, -1.0) in terms:
            seen.add(s)
            out.append((r, s))
    return out


def _launches(mech, g):
    """-> {name: (V, F, K, tin, tout, max_steps, bound on rel_diff)}"""
    from mistra_amd.mechtab import load
    t = load(mech)
    n = g["var_in"].shape[0]
    losses = _first_order_losses(t)
    assert len(losses) >= 6
    cap = [0, 1 % n, 2 % n, n // 2, n - 1]
    V = g["var_in"][[0, 0, 0, 0] + cap[1:]].copy()
    F = g["fix"][[0, 0, 0, 0] + cap[1:]].copy()
    K = g["rconst"][[0, 0, 0, 0] + cap[1:]].copy()
    for cell, nzero in ((1, 1), (2, 6)):      # first-order losses with k = -1/(H*gamma): an exact zero on Ghimj's diagonal at H, H/2, ...
        K[cell] = 0.0
        for i in range(nzero):
            K[cell, losses[i][0]] = -1.0 / ((1.0e-3 / 2 ** i) * GAMMA1)
    V[3] = np.nan
    idx = [i % n for i in range(6)] + [0, n - 1]
    VB, FB, KB = g["var_in"][idx].copy(), g["fix"][idx].copy(), g["rconst"][idx].copy()
    VB[6] = np.nan
    case = {"gas": "gas_day_backward", "aer": "aer_hour", "tot": "tot_backward_fails"}[mech]
    _, VC, FC, KC, tin, tout = pb.reject_case_inputs(case)
    rows = [i % VC.shape[0] for i in range(8)]
    return {"A": (V, F, K, 0.0, 1.5e-3, 0, PARITY_RTOL[mech]), "B": (VB, FB, KB, 0.0, 10.0, 5, PARITY_RTOL[mech]),
            "D": (V, F, K, 0.0, 1.5e-3, 5, PARITY_RTOL[mech]),
            "C": (VC[rows], FC[rows], KC[rows], tin, tout, 0, pb.REJECT_RTOL[case])}


def _enqueue(chem, mech, V, F, K, tin, tout):
    """one launch on torch's current stream, no synchronisation: -> device tensors (var, ierr, stats)"""
    import torch
    dev = torch.device("cuda", 0)
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)
    n = V.shape[0]
    out = torch.empty((n, V.shape[1]), dtype=torch.float64, device=dev)
    ierr, stats = torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 8), dtype=torch.int32, device=dev)
    chem.integrate_into(mech, T(V), T(F), T(K), out, ierr, stats, tin, tout)
    return out, ierr, stats


def _host(r):
    return tuple(x.cpu().numpy() for x in r)


def _bits_equal(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def expected(golden, oracles):
    """the oracle's result of every launch, computed once"""
    from oracle import oracle as om
    want = {}
    for mech in MECHS:
        for name, (V, F, K, tin, tout, max_steps, _) in _launches(mech, golden[mech]).items():
            try:
                om.set_max_steps(max_steps)
                want[mech, name] = oracles[mech].integrate_batch(V, F, K, tin, tout)
            finally:
                om.set_max_steps(0)
    return want


@pytest.mark.parametrize("kernel", ["product", "options"])
@pytest.mark.parametrize("mech", MECHS)
def test_mixed_paths_against_the_oracle_and_repeated(chem, mech, kernel, golden, expected):
    import torch
    if kernel == "options":
        chem.set_options(mech, *R.base_options(mech))      # INTEGRATE_x's own values, through the options instantiation
    seen = set()
    for name, (V, F, K, tin, tout, max_steps, bound) in _launches(mech, golden[mech]).items():
        want, ierr, st = expected[mech, name]
        chem.debug_set_max_steps(max_steps)
        try:
            first = _enqueue(chem, mech, V, F, K, tin, tout)
            second = _enqueue(chem, mech, V, F, K, tin, tout)      # directly behind, same stream
            torch.cuda.synchronize()
        finally:
            chem.debug_set_max_steps(0)
        first, second = _host(first), _host(second)
        got, gi, gs = first
        finite = np.isfinite(want).all(axis=1)
        d = rel_diff(got[finite], want[finite])
        print("%s %s launch %s: IERR %s  Nstp %s  Nrej %s  Ndec %s  Nsng %s  max rel diff %.3e (bound %.1e)"
              % (mech, kernel, name, gi.tolist(), gs[:, 2].tolist(), gs[:, 4].tolist(), gs[:, 5].tolist(), gs[:, 7].tolist(), d.max(), bound))
        assert np.array_equal(gi, ierr), (gi, ierr)
        assert np.array_equal(gs, st), (gs, st)
        assert np.isfinite(got[finite]).all() and d.max() <= bound
        assert _bits_equal(first, second), "the same launch, repeated on the same stream, gave other bits"
        seen |= set(int(x) for x in ierr)
        if name == "A":      # the premises: the paths are really taken
            assert int(st[1, 7]) == 1 and int(ierr[1]) == 1 and int(st[2, 7]) == 6 and int(ierr[2]) == -8 and int(ierr[3]) == -7
        if name == "D":
            assert {-6, -8} <= set(int(x) for x in ierr) and int(ierr[1]) == -6 and (mech == "tot" or 1 in ierr), ierr
        if name == "C":
            assert st[:, 4].max() > 0 and (tout < tin or mech == "aer")
    assert {1, -6, -7, -8} <= seen, seen


def test_tot_launch_directly_behind_a_gas_launch(chem, golden):
    """another mechanism's kernel (another ring placement, other tables) ran on the same stream just before: same bits as on its own"""
    import torch
    V, F, K, tin, tout, _, _ = _launches("tot", golden["tot"])["A"]
    alone = _enqueue(chem, "tot", V, F, K, tin, tout)
    torch.cuda.synchronize()
    gV, gF, gK, gtin, gtout, _, _ = _launches("gas", golden["gas"])["A"]
    _enqueue(chem, "gas", gV, gF, gK, gtin, gtout)
    behind = _enqueue(chem, "tot", V, F, K, tin, tout)
    torch.cuda.synchronize()
    assert _bits_equal(_host(alone), _host(behind))
