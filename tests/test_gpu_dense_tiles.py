"""tot's dense tail block factorised in 16-pivot tile steps (ros3_kernel.hip: dense_lu, MISTRA_DENSE_TILE_FROM): the whole factorisation bit for bit
the emulated kernel programs', which state the arithmetic per entry in panels of four pivots (tests/emu/schedule_emu.cpp) — the tile steps reorder
the work, not an entry's operations — every decomposition of a call, and the operators' solve, which calls the same functions.

Cases.  The nine of test_gpu_dense_finish.py, and one negative-pivot pair per diagonal tile: the first-order loss of a species of that tile's
rows at the rate constant -2/(Hstart*gamma), on cell 0's rate constants and with every other rate constant zero.  A negative pivot is what
leaves -0.0 in finished entries (L = (+0.0) * R, U' = (+0.0) * R with R < 0), and a tile step that gave a finished entry a neutral update would
turn it into +0.0 unseen by a comparison of doubles: everything here is compared as uint64.

    tile  species (0-based)  block row   on the emulator and the oracle
    0     354                1           one negative reciprocal; the oracle ends the call with IERR = -7: first-step factors only
    1     372                19          one negative reciprocal, IERR = 1
    2     385                32          one negative reciprocal, IERR = 1
    3     NVAR - 13          51          the pair of test_gpu_dense_finish.py

No species of block rows 0 .. 15 with a first-order loss gives a call the oracle integrates to IERR = 1 (row 2's, species 355, has no negative
reciprocal on cell 0's rate constants and ends with IERR = -7 on the zeroed ones), so tile 0's pair is held to the first step's factors alone and
test_cases_hold_their_conditions does not demand IERR = 1 of it.  That test (no GPU) holds every condition the GPU tests rest on, on the emulator
and the oracle alone, so that a case that stops meeting its condition fails there."""
import numpy as np
import pytest

from test_gpu_dense_finish import GAMMA0, HSTART, P, cases, emu, emulated_factors      # noqa: F401  (emu: the module's fixture)

TILE_SPECIES = {0: 354, 1: 372, 2: 385}      # tile 3: NVAR - 13, in the nine cases


def first_order_loss(t, s):
    """test_gpu_dense_finish.negative_pivot_reaction's method for species s: the first reaction A = k*V(s) whose only effect on s is the loss -A"""
    for r in range(t.nreact):
        fac = t.a_fac[t.a_ptr[r]:t.a_ptr[r + 1]]
        if len(fac) == 1 and int(fac[0]) == s and (r, -1.0) in [(int(t.vd_idx[p]), float(t.vd_coef[p])) for p in range(t.vd_ptr[s], t.vd_ptr[s + 1])]:
            return r
    raise AssertionError("species %d has no first-order loss" % s)


def tile_cases(g, t):
    """-> names, VAR, FIX, RCONST, tile (the diagonal tile of the case's negative pivot, or -1) of the nine cases and the pairs of tiles 0 .. 2"""
    names, V, F, K = cases(g, t)
    tile = [-1] * 7 + [3, 3]
    v0, f0, k0 = g["var_in"][:1], g["fix"][:1], g["rconst"][:1]
    Vs, Fs, Ks = [V], [F], [K]
    for k in sorted(TILE_SPECIES):
        s = TILE_SPECIES[k]
        assert 16 * k <= s - (t.nvar - 64) < 16 * k + 16
        Kn = np.concatenate([k0, np.zeros_like(k0)])
        Kn[:, first_order_loss(t, s)] = -2.0 / (HSTART * GAMMA0)
        Vs += [v0, v0]; Fs += [f0, f0]; Ks.append(Kn)
        names += ["cell 0, a negative pivot in tile %d (species %d)" % (k, s), "cell 0, RCONST = 0 but that of species %d" % s]
        tile += [k, k]
    return names, np.ascontiguousarray(np.concatenate(Vs)), np.ascontiguousarray(np.concatenate(Fs)), np.ascontiguousarray(np.concatenate(Ks)), tile


def block_slots(t):
    """Ghimj slots of the dense block: rows and columns NVAR-64 .. NVAR-1 -> slots, their block rows, their block columns"""
    n0 = t.nvar - 64
    s = [(p, r - n0, t.icol[p] - n0) for r in range(n0, t.nvar) for p in range(t.crow[r], t.crow[r + 1]) if t.icol[p] >= n0]
    return tuple(np.array(x) for x in zip(*s))


@pytest.fixture(scope="module")
def want(emu, golden, oracles):
    """the cases and their emulated factors, computed once"""
    from mistra_amd.mechtab import load
    o, t = oracles["tot"], load("tot")
    names, V, F, K, tile = tile_cases(golden["tot"], t)
    lu, r = zip(*(emulated_factors(emu, o, t, V[i], F[i], K[i]) for i in range(len(names))))
    return t, names, V, F, K, tile, np.array(lu), np.array(r)


def test_cases_hold_their_conditions(want, oracles):
    t, names, V, F, K, tile, lu, r = want
    o = oracles["tot"]
    slots, _, _ = block_slots(t)
    assert len(slots) == 4089
    for i, name in enumerate(names):
        assert np.isfinite(lu[i]).all() and np.isfinite(r[i]).all(), "%s: the emulated factors are not finite" % name
        bits = lu[i][slots].view(np.uint64)
        n_neg, n_pos = int((bits == np.uint64(1) << np.uint64(63)).sum()), int((bits == 0).sum())
        ierr = None
        if tile[i] != 0:      # tile 0's pair: the first step's factors only (module docstring)
            _, ie, st = o.integrate_batch(V[i:i + 1], F[i:i + 1], K[i:i + 1])
            ierr = int(ie[0])
            assert ierr == 1, "%s: the oracle ends with IERR = %d" % (name, ierr)
        print("%-52s -0.0 in %3d, +0.0 in %4d of the block's %d slots; negative reciprocals in the block %d; IERR %s" % (
            name, n_neg, n_pos, len(slots), int((r[i][-64:] < 0).sum()), ierr))
        if tile[i] >= 0:
            k = tile[i]
            assert n_neg >= 1 and n_pos >= 1, "%s reaches -0.0 in %d and +0.0 in %d slots of the block" % (name, n_neg, n_pos)
            rt = r[i][t.nvar - 64 + 16 * k:t.nvar - 64 + 16 * k + 16]
            assert (rt < 0).sum() == 1, "%s: %d negative reciprocals in tile %d" % (name, int((rt < 0).sum()), k)


@pytest.mark.gpu
def test_factors_are_bit_identical_to_the_emulator(want):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem
    chem.init(0)
    t, names, V, F, K, tile, lu, r = want
    slots, brow, bcol = block_slots(t)
    d = chem.debug_first_step("tot", V, F, K, 0.0, 10.0)
    for i, name in enumerate(names):
        assert d.h[i, 0] == HSTART
        got, ref = np.ascontiguousarray(d.lu[i]).view(np.uint64), lu[i].view(np.uint64)
        gr, rr = np.ascontiguousarray(d.r[i]).view(np.uint64), r[i].view(np.uint64)
        if np.array_equal(got, ref) and np.array_equal(gr, rr):
            continue
        bad = got[slots] != ref[slots]
        per_tile = {(a, b): int(bad[(brow // 16 == a) & (bcol // 16 == b)].sum()) for a in range(4) for b in range(4)}
        first = slots[np.nonzero(bad)[0][0]] if bad.any() else -1
        raise AssertionError("%s: %d of the %d factor slots differ in their bits from the emulated programs; in the block %d of %d, by tile (row, column) %s, "
                             "first slot %d: %r against %r; reciprocals that differ, by tile: %s of the last 64, %d before them" % (
                                 name, int((got != ref).sum()), len(ref), int(bad.sum()), len(slots), {k: v for k, v in per_tile.items() if v}, first,
                                 d.lu[i][first], lu[i][first], [int((gr[-64:] != rr[-64:])[16 * k:16 * k + 16].sum()) for k in range(4)],
                                 int((gr[:-64] != rr[:-64]).sum())))


@pytest.mark.gpu
def test_copies_of_two_cells_integrate_alike(golden, oracles):
    """256 copies each of two captured states in one launch: every decomposition of a call, and a tile buffer's writers against its readers"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem
    chem.init(0)
    g, o = golden["tot"], oracles["tot"]
    cloud = int(np.argmax(g["stats"][:, 2]))
    picks = [7 if cloud != 7 else 8, cloud]
    ncopy = 256
    V, F, K = (np.ascontiguousarray(np.repeat(g[n][picks], ncopy, axis=0)) for n in ("var_in", "fix", "rconst"))
    res = chem.integrate("tot", V, F, K, 0.0, 10.0)
    for j, c in enumerate(picks):
        _, ierr, st = o.integrate_batch(g["var_in"][c:c + 1], g["fix"][c:c + 1], g["rconst"][c:c + 1])
        s = slice(j * ncopy, (j + 1) * ncopy)
        var, ie, stats = np.ascontiguousarray(res.var[s]).view(np.uint64), np.asarray(res.ierr[s]), np.asarray(res.stats[s])
        print("cell %d: %d steps, %d decompositions" % (c, int(st[0, 2]), int(st[0, 5])))
        assert int(ierr[0]) == 1
        assert np.all(ie == 1), "cell %d: IERR differs from 1 in copies %s" % (c, np.nonzero(ie != 1)[0][:8])
        assert np.array_equal(stats, np.repeat(st, ncopy, axis=0)), "cell %d: statistics differ from the oracle's in copies %s" % (c, np.nonzero((stats != st).any(axis=1))[0][:8])
        odd = np.nonzero((var != var[0]).any(axis=1))[0]
        assert len(odd) == 0, "cell %d: %d of %d copies differ from the first in VAR, first: copy %d" % (c, len(odd), ncopy, odd[0])


@pytest.mark.gpu
def test_operator_solve_is_the_first_steps_k1(golden):
    """the operators' kernel factorises with the same functions: its solve of the cell's own vdot at the first step's shift is K(1) of the dump, by bytes"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem
    chem.init(0)
    g = golden["tot"]
    cells = [0, 7, len(g["var_in"]) - 1]
    V, F, K = (np.ascontiguousarray(g[n][cells]) for n in ("var_in", "fix", "rconst"))
    fs = chem.debug_first_step("tot", V, F, K, 0.0, 10.0, hstart=np.full(len(cells), HSTART))
    H = fs.h[:, 0]
    assert np.all(H > 0)
    r = chem.ops("tot", V, F, K, True, False, shift=1.0 / (1.0 * H * GAMMA0), fun_rhs=True)
    assert np.all(np.asarray(r.ising) == 0)
    assert np.ascontiguousarray(r.x[0]).tobytes() == np.ascontiguousarray(fs.k1).tobytes(), "the operators' solve differs from K(1) of the first step"
