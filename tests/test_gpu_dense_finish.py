"""The last 16 pivots of tot's dense tail block, which wave 7 factorises by itself (ros3_kernel.hip: dense_finish): bit identity with the
emulated kernel programs, the signs of zeros included, and every decomposition of a call, not only the first.

Signed zeros.  Fill-in slots start as -0.0 and zero rate constants keep entries at signed zero, so a finished entry of the block can be
either zero — and an update that a finished row took "neutrally" (l = 0) would turn a stored -0.0 into +0.0 without np.array_equal on doubles
seeing it.  The cases: the three captured cells the phase tests use, the same cells with a seeded half of their rate constants set to exactly 0,
and one cell with all of them 0.  The slots of the block's rows and columns 48..63 and the last 16 pivot reciprocals are compared as uint64.
test_cases_reach_signed_zeros (no GPU) holds, on the emulator alone, that these inputs do put both zeros into those slots, that the oracle
integrates each of them to IERR = 1, and lists which cells of the 16x16 are absent from the sparsity pattern.  For tot none is: all 256 cells
are in the pattern (the test asserts it), so the finish's store guard `at != ZERO` is idle there — it never skips a store, and no test can
make it skip one with this mechanism file; it is kept, as in dense_store_panel, for a regenerated mechanism whose pattern has absent cells there.

Those seven cases reach +0.0 only (44 to 240 of the 256 slots, printed per case): every entry of
the last 16x16 has taken, in the Schur steps in front of the block, at least one product with an absent operand, which reads as the +0.0 cell,
and -0.0 + (+0.0) = +0.0.  What does leave -0.0 there is a NEGATIVE pivot among the last 16 (L = (+0.0) * R, U' = (+0.0) * R with R < 0).  So two
more cases: cell 0, and the cell with RCONST = 0, each with the first-order loss of species NVAR - 13 (row 3 of the finish) at the negative
rate constant k = -2/(H*gamma), which makes that row's pivot negative at the first step's H; the oracle integrates both to IERR = 1 (the
species is produced by nothing else that matters in 10 s), and the emulator shows 12 and 24 slots at -0.0, 32 and 216 at +0.0.  All of the
-0.0 coverage comes from these two cases, so each of them is held to at least one -0.0 AND one +0.0 on its own, beside the sum over all nine.

Replication.  256 copies of each of two captured states (one the cloud cell with the most steps of the captured set) in one launch through the
product entry: every copy bit-identical to the first in VAR, IERR and /Statistics/, the statistics the oracle's.  That covers what the first-step
dump cannot: the later decompositions of a call, the finish's buffer against the storers of panel 11, the section without a workgroup barrier."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

GAMMA0 = 0.43586652150845899941601945119356
HSTART = 1.0e-3
SEEDS = (1, 2, 3)      # one per captured cell: which half of its rate constants becomes exactly 0 (seeds the oracle integrates to IERR = 1)
dp = C.POINTER(C.c_double)


def P(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def emu():
    d = os.path.join(REPO, "tests", "emu")
    subprocess.run(["make", "-s", "-C", d], check=True)
    lib = C.CDLL(os.path.join(d, "libschedule_emu.so"))
    lib.emu_create.restype = C.c_void_p
    lib.emu_create.argtypes = [C.c_char_p, C.c_int]
    lib.emu_lu.argtypes = [C.c_void_p, dp, dp, dp]
    return lib, lib.emu_create(os.path.join(REPO, "mistra_amd", "mech", "tot.mech").encode(), 512)


def negative_pivot_reaction(t):
    """the first reaction A = k*V(s), s = NVAR - 13, whose only effect on s is the loss -A: Jac0(s,s) gets exactly -k from it"""
    s = t.nvar - 13
    for r in range(t.nreact):
        fac = t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]]
        if len(fac) == 1 and int(fac[0]) == s and (r, -1.0) in [(int(t.vd_idx[p]), float(t.vd_coef[p])) for p in range(t.vd_ptr[s], t.vd_ptr[s + 1])]:
            return r
    raise AssertionError("species %d has no first-order loss" % s)


def cases(g, t):
    """-> names, VAR, FIX, RCONST of the nine cells"""
    cells = [0, 7, len(g["var_in"]) - 1]
    V, F, K = g["var_in"][cells], g["fix"][cells], g["rconst"][cells]
    Kh = K.copy()
    for i, seed in enumerate(SEEDS):
        Kh[i, np.random.default_rng(seed).permutation(K.shape[1])[:K.shape[1] // 2]] = 0.0
    Kn = np.concatenate([K[:1], np.zeros_like(K[:1])])
    Kn[:, negative_pivot_reaction(t)] = -2.0 / (HSTART * GAMMA0)
    names = ["cell %d" % c for c in cells] + ["cell %d, half of RCONST zero (seed %d)" % (c, s) for c, s in zip(cells, SEEDS)] + ["cell %d, RCONST = 0" % cells[0]]
    names += ["cell %d, a negative pivot in row 3" % cells[0], "cell %d, RCONST = 0 but that one" % cells[0]]
    return (names, np.ascontiguousarray(np.concatenate([V, V, V[:1], V[:1], V[:1]])), np.ascontiguousarray(np.concatenate([F, F, F[:1], F[:1], F[:1]])),
            np.ascontiguousarray(np.concatenate([K, Kh, np.zeros_like(K[:1]), Kn])))


def finish_slots(t):
    """Ghimj slots of the last 16 rows' entries in the last 16 columns, and the 16x16 map of which cells the pattern has"""
    n0 = t.nvar - 16
    slots, present = [], np.zeros((16, 16), bool)
    for r in range(n0, t.nvar):
        for p in range(t.crow[r], t.crow[r + 1]):
            if t.icol[p] >= n0:
                slots.append(p)
                present[r - n0, t.icol[p] - n0] = True
    return np.array(slots), present


def emulated_factors(emu, o, t, v, f, k):
    lib, h = emu
    G = -o.jac_sp(v, f, k)
    G[t.diag] += 1.0 / (HSTART * GAMMA0)
    lu, r, x = G.copy(), np.empty(o.nvar), o.fun(v, f, k)
    assert lib.emu_lu(h, P(lu), P(r), P(x)) == 0
    return lu, r


def test_cases_reach_signed_zeros(emu, golden, oracles):
    from mistra_amd.mechtab import load
    o, t = oracles["tot"], load("tot")
    names, V, F, K = cases(golden["tot"], t)
    slots, present = finish_slots(t)
    print("cells of the last 16x16 absent from the pattern: %s" % ([(int(r), int(c)) for r, c in zip(*np.nonzero(~present))] or "none: the store guard is idle there"))
    assert present.all(), "the pattern has absent cells in the last 16x16 now: the finish's store guard is live, add a case that shows it"
    neg = pos = 0
    for i, name in enumerate(names):
        _, ierr, st = o.integrate_batch(V[i:i + 1], F[i:i + 1], K[i:i + 1])
        assert int(ierr[0]) == 1, "%s: the oracle ends with IERR = %d: choose another seed" % (name, int(ierr[0]))
        lu, r = emulated_factors(emu, o, t, V[i], F[i], K[i])
        assert np.isfinite(lu[slots]).all() and np.isfinite(r[-16:]).all()
        bits = lu[slots].view(np.uint64)
        n_neg, n_pos = int((bits == np.uint64(1) << np.uint64(63)).sum()), int((bits == 0).sum())
        print("%-44s -0.0 in %3d, +0.0 in %3d of the %d slots; Nstp %d" % (name, n_neg, n_pos, len(slots), int(st[0, 2])))
        neg, pos = neg + n_neg, pos + n_pos
        if "negative pivot" in name or "but that one" in name:
            assert n_neg >= 1 and n_pos >= 1 and (r[-16:] < 0).sum() == 1 and r[-13] < 0
    assert neg >= 1 and pos >= 1, "the cases reach -0.0 in %d and +0.0 in %d slots of the finish: they prove nothing about signed zeros" % (neg, pos)


@pytest.mark.gpu
def test_finish_is_bit_identical_to_the_emulator(emu, golden, oracles):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem
    from mistra_amd.mechtab import load
    chem.init(0)
    o, t = oracles["tot"], load("tot")
    names, V, F, K = cases(golden["tot"], t)
    slots, _ = finish_slots(t)
    d = chem.debug_first_step("tot", V, F, K, 0.0, 10.0)
    for i, name in enumerate(names):
        assert d.h[i, 0] == HSTART
        lu, r = emulated_factors(emu, o, t, V[i], F[i], K[i])
        got, want = np.ascontiguousarray(d.lu[i][slots]).view(np.uint64), lu[slots].view(np.uint64)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, "%s: %d of the finish's %d slots differ in their bits from the emulated programs, first: slot %d, %r against %r" % (
            name, len(bad), len(slots), slots[bad[0]], d.lu[i][slots[bad[0]]], lu[slots[bad[0]]])
        assert np.array_equal(np.ascontiguousarray(d.r[i][-16:]).view(np.uint64), r[-16:].view(np.uint64)), "%s: the last 16 pivot reciprocals differ" % name
        # (and nothing else moved: the whole factorisation, as the phase tests hold it)
        assert np.array_equal(np.ascontiguousarray(d.lu[i]).view(np.uint64), lu.view(np.uint64)), "%s: factors outside the finish differ in their bits" % name
        assert np.array_equal(np.ascontiguousarray(d.r[i]).view(np.uint64), r.view(np.uint64))


@pytest.mark.gpu
def test_copies_of_a_cell_integrate_alike(golden, oracles):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem
    chem.init(0)
    g, o = golden["tot"], oracles["tot"]
    cloud = int(np.argmax(g["stats"][:, 2]))
    picks = [0 if cloud != 0 else 1, cloud]
    ncopy = 256
    V, F, K = (np.ascontiguousarray(np.repeat(g[n][picks], ncopy, axis=0)) for n in ("var_in", "fix", "rconst"))
    res = chem.integrate("tot", V, F, K, 0.0, 10.0)
    for j, c in enumerate(picks):
        _, ierr, st = o.integrate_batch(g["var_in"][c:c + 1], g["fix"][c:c + 1], g["rconst"][c:c + 1])
        s = slice(j * ncopy, (j + 1) * ncopy)
        var, ie, stats = np.ascontiguousarray(res.var[s]).view(np.uint64), np.asarray(res.ierr[s]), np.asarray(res.stats[s])
        print("cell %d: %d steps, %d decompositions" % (c, int(st[0, 2]), int(st[0, 5])))
        assert np.all(ie == 1) and int(ierr[0]) == 1
        assert np.array_equal(stats, np.repeat(st, ncopy, axis=0)), "cell %d: statistics differ from the oracle's in copies %s" % (c, np.nonzero((stats != st).any(axis=1))[0][:8])
        odd = np.nonzero((var != var[0]).any(axis=1))[0]
        assert len(odd) == 0, "cell %d: %d of %d copies differ from the first in VAR, first: copy %d" % (c, len(odd), ncopy, odd[0])
