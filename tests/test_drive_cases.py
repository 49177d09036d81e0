"""The cases of tests/drive_cases.py on the CPU: the restated budgets (oracle/pack_py.py: the mechanism table's rate products, the .pack table's sulphur terms)
against what the COMPILED bud_x / bud_s_x of the reference — formula lists of their own — made of the same states (tests/golden/drive_edges_<mech>.npz,
tests/golden/make_drive_edges_golden.py), bit for bit; (a) every other order of the factors of every multi-factor reaction is told apart by a state;
(b) the edge tables: every named edge is reached, counted where it acts; the species maps' legal sets and refusals against a restatement of the C ABI's
checks; and the facts about the tables that budgets_kernel, pack_kernel and the arena of mistra_chem_drive_begin rely on without checking.  The same cases
run on the device in tests/test_gpu_drive_edges.py.  No GPU, no reference tree."""
import os

import numpy as np
import pytest

import drive_cases as dc
from mistra_amd.mechtab import load as load_mech


@pytest.mark.parametrize("mech", dc.MECHS)
def test_fixture_was_made_from_these_states(mech):
    fx, c = dc.fixture(mech), dc.budget_cases(mech)
    assert list(fx["names"]) == c["names"]
    assert str(fx["input_sha256"]) == dc.input_sha256(mech), "the seeded inputs drifted from what the reference saw: run tests/golden/make_drive_edges_golden.py"
    path = os.path.join(dc.GOLD, "drive_edges_%s.npz" % mech)
    assert os.path.getsize(path) <= min(os.path.getsize(os.path.join(dc.GOLD, "drive_%s.npz" % mech)), 1 << 20)
    assert set(fx.files) <= {"bg", "bg1", "bgs", "names", "input_sha256", "provenance"}      # recorded results and names, nothing else
    assert len([n for n in c["names"] if n.startswith("seeded")]) == dc.NB
    # seeded values: full mantissas over many decades, all finite and positive in C and RCONST
    s = c["C"][:dc.NB]
    assert np.isfinite(s).all() and (s > 0).all() and np.log10(s.max() / s.min()) > 20 and (np.frexp(s)[0] != 0.5).mean() > 0.99


@pytest.mark.parametrize("mech", dc.MECHS)
def test_restated_budgets_equal_the_compiled_reference_on_every_state(mech):
    """bit for bit, the sign of every zero included, NaN in the same places; the entries of bgs no term sets and no range accumulates keep the caller's"""
    (wbg, wbgs), (gbg, gbgs) = dc.expected_budgets(mech), dc.restated_budgets(mech)
    c = dc.budget_cases(mech)
    for i, name in enumerate(c["names"]):
        bad = np.nonzero(dc.where_differ(gbg[i], wbg[i]).any(axis=1))[0]
        assert bad.size == 0, "%s, state %r: bg of reactions %s (numbered from 1)" % (mech, name, (bad[:8] + 1).tolist())
        bad = np.nonzero(dc.where_differ(gbgs[i], wbgs[i]).any(axis=1))[0]
        assert bad.size == 0, "%s, state %r: bgs slots %s" % (mech, name, (bad[:8] + 1).tolist())
    tab = dc.table(mech)
    set_ = {s for s, _ in tab["bud_s"]}
    acc = {i for lo, hi in tab["bud_s_acc"] for i in range(lo, hi + 1)}
    for slot in range(1, dc.NBGS + 1):
        if slot not in set_:
            assert dc.same(wbgs[:, slot - 1, 0], c["bgs_in"][:, slot - 1, 0])
        if slot not in acc:
            assert dc.same(wbgs[:, slot - 1, 1], c["bgs_in"][:, slot - 1, 1])
    assert np.isnan(wbg).any() and np.isinf(wbg).any() and (wbg == 0.0).any() and np.isnan(wbgs).any()


@pytest.mark.parametrize("mech", dc.MECHS)
def test_every_other_order_of_every_product_is_told_apart(mech):
    """(a) RCONST(i)*f1*f2*.. left to right in the table's order: for every reaction with at least two distinct factors and every other order of them, a
    state gives other bits.  A regenerated mechanism table whose order stopped agreeing with bud_x.f therefore fails the fixture comparison above."""
    multi = dc.multi_factor_reactions(mech)
    assert len(multi) == {"gas": 244, "aer": 602, "tot": 960}[mech]
    left = dc.orders_not_told_apart(mech)
    assert not left, "%s: no state tells these orders from the table's (reaction numbered from 1, order): %s" % (mech, left[:10])
    print("%s: %d multi-factor reactions, %d other orders, all told apart by %d states" % (mech, len(multi), sum(len(o) for _, o in multi),
                                                                                          len(dc.budget_cases(mech)["names"])))


@pytest.mark.parametrize("mech", dc.MECHS)
def test_every_budget_edge_is_reached(mech):
    """(b) counted in the products and terms themselves; a state that stops reaching its edge fails here by name"""
    reach = dc.budget_reach(mech)
    for e, names in reach.items():
        print("  %-52s %2d state(s): %s" % (e, len(names), ", ".join(names[:3]) + (" ..." if len(names) > 3 else "")))
    missed = [e for e, names in reach.items() if not names]
    assert not missed, "%s: no state reaches %s" % (mech, missed)
    assert ("unset accumulated slot carries a non-zero value" in reach) == bool(dc.UNSET_SLOTS[mech])
    own = {"species +0.0": "=+0.0", "species -0.0": "=-0.0", "species < 0": "<0", "species NaN": "=NaN", "bg: product subnormal": "product subnormal",
           "bgs: term subnormal": "product subnormal", "bg: product underflows to 0": "product underflows to 0", "bgs: term underflows to 0": "product underflows to 0",
           "bg: product overflows": "product overflows", "bgs: term overflows": "product overflows", "cumulative from Inf": "cumulative=Inf", "dt = 0.1": "dt=0.1"}
    for e, tail in own.items():
        assert any(n.endswith(tail) for n in reach[e]), (e, reach[e])


@pytest.mark.parametrize("mech", dc.MECHS)
def test_every_pack_edge_is_reached(mech):
    """(b) each cvv kind in each bin on the FIX entry it feeds, a clamped negative, -0.0 and NaN in sl1 and sion1 (where the mechanism reads them) on the C
    entries and on the clamped model arrays, the hand-over state's -0.0 / NaN / negative entries"""
    reach = dc.pack_reach(mech)
    for e, names in reach.items():
        print("  %-52s %2d layer(s): %s" % (e, len(names), ", ".join(names[:3]) + (" ..." if len(names) > 3 else "")))
    missed = [e for e, names in reach.items() if not names]
    assert not missed, "%s: no layer reaches %s" % (mech, missed)
    bins = dc.cvv_bins(mech)
    assert bins == {"gas": [], "aer": [1, 2], "tot": [1, 2, 3, 4]}[mech]
    for kc in bins:
        for nm, _ in dc.CVV_KINDS:      # alone and with every bin together
            assert reach["cvv%d %s" % (kc, nm)] == ["cvv%d=%s" % (kc, nm), "cvv*=%s" % nm]
    assert dc.arrays_read(mech) == (("sl1",) if mech == "gas" else ("sl1", "sion1"))      # gas_drive reads sl1 only (gas.f:151-156)
    p = dc.pack_cases(mech)
    assert len(p["names"]) == 1 + 7 * (len(bins) + bool(bins)) + 4 + 3 and len(set(p["names"])) == len(p["names"])


@pytest.mark.parametrize("mech", dc.MECHS)
def test_clamped_handover_entries_are_where_the_gpu_tests_expect_them(mech):
    """gas_drive clamps every entry it hands over to sl1 (gas.f:200-217); aer_drive and tot_drive clamp none (they clamp the whole arrays on the way IN,
    tot.f:226-227).  tests/test_gpu_pack.py and tests/test_gpu_drive_edges.py rely on this."""
    tab = dc.table(mech)
    clamped = dc.handover_clamped(mech)
    if mech == "gas":
        assert len(clamped) == len(tab["unpack"]) == 6 and all(cl for *_, cl in tab["unpack"]) and all(cl for *_, cl in tab["pack"]) and not tab["preclamp"]
    else:
        assert clamped == [] and not any(cl for *_, cl in tab["pack"]) and tab["preclamp"]
    assert sorted(c for _, _, _, c, _ in tab["unpack"]) == sorted(c for c, *_ in tab["pack"])      # what is packed is handed back


@pytest.mark.parametrize("mech", dc.MECHS)
def test_table_facts_the_kernels_rely_on(mech):
    tab, t = dc.table(mech), load_mech(mech)
    nvar, nfix = tab["nvar"], tab["nfix"]
    # the arena's FIX is not cleared the way VAR is: every FIX index is set by the fix list
    assert sorted(c for c, _, _ in tab["fix"]) == list(range(nvar + 1, nvar + nfix + 1))
    # pack_kernel assigns in parallel: no C index is set twice by pack + fix
    both = [c for c, *_ in tab["pack"]] + [c for c, _, _ in tab["fix"]]
    assert len(set(both)) == len(both) and all(1 <= c <= nvar for c, *_ in tab["pack"])
    for _, arr, i, kc, _ in tab["pack"]:
        assert arr in ("sl1", "sion1") and 1 <= kc <= tab["nkc"] and 1 <= i <= (tab["j2"] if arr == "sl1" else tab["j6"])
    dst = [(arr, i, kc) for arr, i, kc, _, _ in tab["unpack"]]
    assert len(set(dst)) == len(dst)                       # unpack_kernel: no model entry written twice
    # budgets_kernel: one thread per slot, then one thread per accumulated cell
    ids = [s for s, _ in tab["bud_s"]]
    assert len(set(ids)) == len(ids) and all(1 <= s <= dc.NBGS for s in ids)
    cells = [i for lo, hi in tab["bud_s_acc"] for i in range(lo, hi + 1)]
    assert len(set(cells)) == len(cells) and all(1 <= lo <= hi <= dc.NBGS for lo, hi in tab["bud_s_acc"]), "accumulation ranges overlap: two threads would add to one cell"
    assert set(ids) <= set(cells)                          # every rate that is set is accumulated
    assert tuple(sorted(set(cells) - set(ids))) == dc.UNSET_SLOTS[mech]
    for _, terms in tab["bud_s"]:
        assert terms
        for sign, r, cs in terms:
            assert sign in (1, -1) and 1 <= r <= t.nreact and all(1 <= c <= nvar for c in cs), "a budget term reads a species that is not variable"
    # no shipped slot begins with a negative term (the kernel's `-p` start is reached by no input; a table that gains one needs a state for it here)
    assert [s for s, terms in tab["bud_s"] if terms[0][0] < 0] == []
    assert any(sign < 0 for _, terms in tab["bud_s"] for sign, _, _ in terms[1:]) == (mech != "gas")      # (subtracted later terms exist in aer and tot)
    # bud_x: every factor is a species or one of the table's constants
    assert t.a_fac.min() >= 0 and t.a_fac.max() < nvar + nfix + t.nconst and (np.diff(t.a_ptr) >= 1).all()


@pytest.mark.parametrize("mech", dc.MECHS)
def test_species_map_sets_and_their_refusals(mech):
    """the legal sets pass the restated checks, each refusal set differs from the capture's maps in one mapped species and is refused with ITS text — the
    one the device library must give (tests/test_gpu_drive_edges.py)"""
    sets = dc.map_sets(mech)
    tab = dc.table(mech)
    assert [(len(m[1]), len(m[3])) for m in sets.values()] == [(60, 16), (60, 16), (1, 0), (0, 0), (tab["nvar"] - len(tab["pack"]), 0)]
    for name, maps in sets.items():
        assert dc.refusal_of(mech, maps) is None, name
    good = sets["capture"]
    assert not np.array_equal(sets["s1 reversed"][1], good[1]) and sorted(sets["s1 reversed"][1]) == sorted(good[1])
    texts = []
    for name, text, maps in dc.refusal_sets(mech):
        assert dc.refusal_of(mech, maps) == text, name
        changed = {int(j) for j in np.nonzero((maps[0] != good[0]).any(axis=1))[0]}
        assert len(changed) == 1 or (name == "gas_k2m not the inverse" and not changed), name
        assert sum(int((a != b).sum()) for a, b in zip(maps, good)) <= 2 and np.array_equal(maps[2], good[2]) and np.array_equal(maps[3], good[3])
        texts.append(text)
    assert set(texts) == {dc.REFUSE_RANGE, dc.REFUSE_TWICE, dc.REFUSE_INVERSE, dc.REFUSE_PACKED} and texts.count(dc.REFUSE_RANGE) == 4
    src = open(os.path.join(dc.REPO, "mistra_amd", "csrc", "capi.cpp")).read()
    for text in set(texts):
        assert text in src, "the refusal %r is no longer in mistra_chem_set_species_maps" % text
    for name in sets:      # one ordinary layer under every legal set: the restatement writes every mapped species
        lay = dc.map_layer(mech, name)
        m2k = sets[name][0]
        if len(m2k):
            assert dc.same(lay["C"][m2k[:, 0] - 1], lay["s1"][m2k[:, 1] - 1]) and dc.same(lay["s1_out"], lay["c_out"][sets[name][1] - 1])
