"""The seeded liq_parm cases of tests/liq_cases.py, on the CPU: do they reach what they are there for?  Every condition below is computed from the inputs
and the restatements' results alone, so that a GPU test (tests/test_gpu_liq_synth.py) cannot pass because a branch or a chunk edge was never reached.
Then the bounds of the comparisons that pass through exp / log: the restatements' own movement when each of those returns the next double up or down
(liq_cases.MathShim), 10x of which — or the project's 1e-14 where that is more — is the bound (tests/parity_bounds.py: LIQ_SYNTH_RTOL).
The restatements are the scalar ones that tests/test_pack.py and tests/test_rates.py pin against the captured layers; nothing here is vectorised."""
import math

import numpy as np
import pytest

import liq_cases as L
from parity_bounds import LIQ_SYNTH_FLOOR, LIQ_SYNTH_RTOL, check_constant


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_fast_k_mt_cases_reach_every_edge(mech):
    calls, exp = L.kmt_calls(mech), L.kmt_expected(mech)
    tab = L.kmt_py.load(mech)
    lex = np.array(tab["lex"]) - 1
    assert sum(len(c["t"]) for c in calls) <= 24
    assert {c["ka"] for c in calls} == {0, 1, 4, 52, 69, 70} and {c["ifeed"] for c in calls} == {0, 2} and {c["nkc_l"] for c in calls} == {2, 4}
    nkt = tab["nkt"]
    kws = [c["kw"] for c in calls]
    assert any((k == 0).all() for k in kws) and any((k == nkt).all() for k in kws)
    assert any((k == 0).any() and (k == nkt).any() and len(set(k.tolist())) > 10 for k in kws)
    assert sum(np.array_equal(k, np.load(L.os.path.join(L.GOLD, "kmt_%s.npz" % mech))["kw"]) for k in kws) >= 2
    edges = set()                 # what a bin that is written (cm > 0, cw > 0) looks like to the kernel's chunk loop
    combos = {b: set() for b in range(4)}
    regimes, wet_nonzero, wet_could = set(), 0, 0
    for c, (xk, vt) in zip(calls, exp):
        nl = len(c["t"])
        assert c["t"].min() >= 230 and c["t"].max() <= 300 and c["p"].min() >= 5e4 and c["p"].max() <= 1.02e5
        assert len(set(c["xkmt0"].ravel().tolist())) == c["xkmt0"].size and len(set(c["vt0"].ravel().tolist())) == c["vt0"].size
        assert (c["alpha"][:, lex] == 0).any() and (c["alpha"][:, lex] > 0).sum() > 0.8 * nl * len(lex)
        for i in range(nl):
            ff = c["ff"][i]
            if c["stokes"][i]:
                assert not (ff[c["rq"] > 10.0] != 0).any() and (ff != 0).sum() > 1000
            else:
                assert (ff != 0).mean() >= 0.5 and len(set(ff[ff != 0].tolist())) == (ff != 0).sum()
            assert {(c["cm"][i, b] > 0, c["cw"][i, b] > 0) for b in range(4)} == {(True, True), (True, False), (False, True), (False, False)}
            for b in range(4):
                mask, ncell = L.kmt_bin_cells(c, b + 1)
                live = mask & (ff != 0)
                cm_on, cw_on = c["cm"][i, b] > 0, c["cw"][i, b] > 0
                if b < c["nkc_l"]:
                    combos[b].add((cm_on, cw_on))
                # ---- xkmt: rewritten for every exchanged species exactly where cm > 0 and cw > 0, poison elsewhere
                written = xk[i, b] != c["xkmt0"][i, b]
                if b < c["nkc_l"] and cm_on and cw_on:
                    assert written[lex].all() and written.sum() == len(lex)
                    if ncell == 0:
                        edges.add("empty")
                        assert (xk[i, b][lex] == 0).all()
                    else:
                        nchunk = -(-ncell // L.KMT_CELLS)
                        last = np.zeros(mask.size, bool)
                        ia0 = ((2 if c["ifeed"] == 2 else 1) if b in (0, 2) else c["ka"] + 1) - 1
                        last[ia0 * nkt + (nchunk - 1) * L.KMT_CELLS: ia0 * nkt + ncell] = True
                        tail_live = bool((live.ravel() & last).any())      # the last chunk holds a cell that counts: the drain iteration matters
                        if ncell == nkt and tail_live:
                            edges.add("one row")
                        if ncell % L.KMT_CELLS == 0 and tail_live:
                            edges.add("exact")
                        if ncell % L.KMT_CELLS != 0 and tail_live:
                            edges.add("ragged")
                        if live.any():
                            assert (xk[i, b][lex] > 0).all()
                        else:
                            edges.add("no cell in range")
                else:
                    assert not written.any()
                # ---- vt: every bin 1..nkc_l with cw > 0, whatever cm
                if b < c["nkc_l"] and cw_on:
                    assert vt[i, b] >= 0
                    if live.any():
                        wet_could += 1
                        wet_nonzero += int(vt[i, b] > 0)
                        if not c["stokes"][i]:
                            regimes |= {bool(x) for x in (c["rq"][live] <= 10.0)}
                    if not cm_on:
                        edges.add("vt without chemistry")
                else:
                    assert vt[i, b] == c["vt0"][i, b]
    assert edges == {"empty", "one row", "exact", "ragged", "no cell in range", "vt without chemistry"}, edges
    for b in range(4):
        assert len(combos[b]) == 4, "bin %d misses a (cm, cw) combination" % (b + 1)
    assert regimes == {True, False}
    assert wet_could >= 20 and wet_nonzero >= 0.9 * wet_could      # the bounded vt comparison is about numbers, not zeros
    sc, sl = L.KMT_STOKES
    sv = exp[sc][1][sl]
    assert ((sv > 0) & (calls[sc]["cw"][sl] > 0)).any()


def test_cw_rc_cases_reach_every_row_of_the_table():
    calls, exp = L.cwrc_calls(), L.cwrc_expected()
    assert {(c["nka"], c["nkt"]) for c in calls} == {(70, 70), (1, 1), (64, 32), (65, 32), (37, 53), (5, 2048)}
    assert {c["ifeed"] for c in calls} == {0, 2}
    inside = edge = False
    for c in calls:
        rows = L.CWRC_CHUNK // c["nkt"]
        assert rows >= 1
        if c["nka"] > rows and 0 < c["ka"] < c["nka"]:
            edge |= c["ka"] % rows == 0
            inside |= c["ka"] % rows != 0
        if c["nka"] > 1:
            assert (c["kw"] == 0).any() and (c["kw"] == c["nkt"]).any() or (c["nka"], c["nkt"]) == (70, 70)
    assert inside and edge and any(c["ka"] == 0 for c in calls) and any(c["ka"] == c["nka"] for c in calls)
    assert any(c["ifeed"] == 2 and c["ka"] >= 2 and (c["ff"][:, 0] != 0).any() for c in calls)      # a first row that ifeed = 2 must leave out
    seen = {b: set() for b in range(4)}
    below = set()
    at = {b: set() for b in (0, 1)}
    for c, ((rc, cw, cm, cv, bl), (rcd, cwd)) in zip(calls, exp):
        crys, deli = c["crys4"][:2], c["crys4"][2:]
        assert np.array_equal(cm > 0, cv > 0) and np.array_equal(cw == 0, rc == 0)
        for i in range(len(c["feu"])):
            feu, is_below = float(c["feu"][i]), bool(bl[i])
            below.add(is_below)
            assert is_below == (feu < crys.min())
            for b in range(4):
                cws, on = cw[i, b] * 1e12, bool(cv[i, b] > 0)      # (the un-scaled sum to 1e-16: every case keeps a factor 3 from the thresholds)
                if cws == 0:
                    seen[b].add("zero sum")
                    assert not on
                if b >= 2:
                    big = cws >= L.CWMD
                    assert 0.2 * L.CWMD < cws < 0.5 * L.CWMD or cws > 2 * L.CWMD or cws == 0
                    seen[b].add("below" if is_below and big else "on" if big and on else "small" if not big and not on and not is_below else "-")
                    assert on == (big and not is_below)
                    continue
                big, cl, ge_c, ge_d = cws >= L.CWM, bool(c["cloud"][i, b]), feu >= crys[b], feu >= deli[b]
                assert 0.2 * L.CWM < cws < 0.5 * L.CWM or cws > 2 * L.CWM or cws == 0
                assert on == (not is_below and big and ((cl and ge_c) or ge_d))
                if is_below:
                    seen[b].add("below" if big else "-")
                    continue
                if not big and ((cl and ge_c) or ge_d):
                    seen[b].add("small sum, humid enough")
                if big:
                    seen[b].add(("cloud, " if cl else "no cloud, ") + ("above deliquescence" if ge_d else "between" if ge_c else "under its crystallisation"))
                    for name, th in (("crys", crys[b]), ("deli", deli[b])):
                        for tag, v in (("-", math.nextafter(th, -math.inf)), ("=", float(th)), ("+", math.nextafter(th, math.inf))):
                            if feu == v:
                                at[b].add((name + tag, cl, on))
    assert below == {True, False}
    for b in (0, 1):
        want = {"zero sum", "below", "small sum, humid enough"} | {c + h for c in ("cloud, ", "no cloud, ") for h in ("above deliquescence", "between", "under its crystallisation")}
        assert seen[b] >= want, (b, want - seen[b])
        # at each threshold exactly, one step under and one step over it, with the cloud flag both ways: the comparison is >=
        assert at[b] >= {("crys-", True, False), ("crys=", True, True), ("crys+", True, True), ("crys=", False, False), ("deli-", False, False),
                         ("deli=", False, True), ("deli+", False, True), ("deli-", True, True)}, (b, at[b])
    for b in (2, 3):
        assert seen[b] >= {"zero sum", "below", "on", "small"}, (b, seen[b])
    # the dry routine on the same grids: both bins with and without particles
    assert all(any((d[1][:, b] == 0).any() for _, d in exp) and any((d[1][:, b] > 0).any() for _, d in exp) for b in (0, 1))


@pytest.mark.parametrize("mech", ["gas", "aer", "tot"])
def test_dry_rates_cases_reach_both_branches(mech):
    cases, exp = L.dry_cases(mech), L.dry_expected(mech)
    assert tuple(len(c["tt"]) for c in cases) == (1, 64, 65, 200)
    tt = np.concatenate([c["tt"] for c in cases])
    rcd = np.concatenate([c["rcd"] for c in cases])
    assert tt.min() >= 200 and tt.max() <= 310 and tt.min() < 215 and tt.max() > 295
    assert (rcd == 0).any() and (rcd < 0).any() and (rcd > 0).mean() > 0.7
    xk = np.concatenate([e[0] for e in exp])
    assert np.array_equal(xk == 0, np.broadcast_to((rcd <= 0)[:, :, None], xk.shape))      # x1 = 0 exactly where rcd <= 0
    assert all((e[0][0] != 0).any() for e in exp)
    if mech == "gas":
        h0 = np.concatenate([c["henry4"] for c in cases])
        assert all(((h0[:, 1:] > 0).any(), (h0[:, 1:] == 0).any(), (h0[:, 1:] < 0).any()))
        h = np.concatenate([e[2] for e in exp])
        assert np.array_equal(h[:, 1:][h0[:, 1:] <= 0], h0[:, 1:][h0[:, 1:] <= 0]) and (h[:, 0] > 0).all()
        assert (h != 0).mean() >= 0.7      # what the bounded comparison of henry4 sees: HNO3's in every layer, the others where positive


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_liq_cases_reach_dry_bins_and_the_temperature_range(mech):
    cases, exp = L.liq_cases(mech), L.liq_expected(mech)
    assert tuple(len(c["tt"]) for c in cases) == (1, 300)
    nkc_eq = L.liq_py.load(mech)["equil"]["nkc"]
    h_exp, h_plain = L.henry_exp_species(mech)
    f_exp, f_plain, b_exp, b_plain = L.equil_exp_species(mech)
    assert len(h_exp) > 20 and len(h_plain) > 5 and len(f_exp) > 5 and len(f_plain) > 5 and len(b_plain) > 5
    for c, e in zip(cases, exp):
        assert c["tt"].min() >= 200 and c["tt"].max() <= 320 and 0.1 <= c["xgamma"].min() and c["xgamma"].max() <= 3
        assert (e["henry"][:, h_exp] > 0).all() and (e["henry"][:, h_plain] > 0).any()            # the bounded comparison covers every exp entry
        assert (e["vmean"] != 0).sum(axis=1).min() >= 90 and (e["vmean"] == 0).any()
        wet = c["conv2"][:, :nkc_eq] > 0
        assert wet.any()
        for arr, before, ex in ((e["xkef"], c["xkef0"], f_exp), (e["xkeb"], c["xkeb0"], b_exp)):
            assert (arr[:, :nkc_eq][~wet] == 0).all() and np.array_equal(arr[:, nkc_eq:], before[:, nkc_eq:])
            if len(ex):
                assert (arr[:, :nkc_eq][wet][:, ex] != 0).mean() >= 0.9
    big = cases[1]
    assert big["tt"].min() < 205 and big["tt"].max() > 315
    for b in range(L.NKC):
        assert (big["conv2"][:, b] > 0).any() and (big["conv2"][:, b] == 0).any() and (big["conv2"][:, b] < 0).any()


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_st_coeff_cases_reach_zero_and_positive_inputs(mech):
    cases, exp = L.stc_cases(mech), L.stc_expected(mech)
    assert tuple(len(e) for e in cases) == (1, 300) and len(exp) == 8
    env = cases[1]
    assert env[:, 0].min() >= 230 and env[:, 0].max() <= 310 and env[:, 0].min() < 235 and env[:, 0].max() > 305
    for col, top in ((1, 1.2e-9), (2, 1.2e-9), (3, 4.5e-10), (4, 1.05e-10)):
        assert (env[:, col] == 0).any() and (env[:, col] > 0).any() and env[:, col].max() <= top
    assert env[:, 3].max() > 4e-10 and env[:, 4].max() > 5e-11
    assert ((env[:, 1] > 0) & (env[:, 2] > 0) & (env[:, 3] > 0)).sum() > 100      # a_n2o5 with every branch taken
    assert ((env[:, 1] > 0) & (env[:, 2] == 0)).any() and ((env[:, 1] == 0) & (env[:, 2] > 0)).any()
    differ = 0
    for s, (jo, bu) in enumerate(L.STC_SWITCHES):
        plain = L.stc_plain_species(mech, jo, bu)
        rest = np.setdiff1d(np.arange(exp[2 * s].shape[1]), plain)
        assert len(plain) > 200 and len(rest) >= 3
        assert (exp[2 * s + 1][:, rest] != 0).mean() >= 0.9
        differ += int(not np.array_equal(exp[2 * s + 1], exp[1]))
    assert differ >= 1      # a switch changes the coefficients


def test_bounds_of_the_synthetic_comparisons_follow_the_restatements_own_movement(capsys):
    """Per routine: the worst relative movement of the restatement over the seeded cases when exp, log, log10, pow and sqrt return the next double up or
    down; LIQ_SYNTH_RTOL holds 10x to 100x of it, or the project's 1e-14 where 10x is less.  (v_mean and the gas speeds of dry_rates are not bounded
    here: sqrt is correctly rounded on both sides, they are compared bit for bit.)"""
    measured = {}
    for mech in ("aer", "tot"):
        measured["henry"] = max(measured.get("henry", 0.0), L.spread(lambda: L.henry_compute(mech)))
        measured["equil_co"] = max(measured.get("equil_co", 0.0), L.spread(lambda: L.equil_compute(mech)))
        measured["vt"] = max(measured.get("vt", 0.0), L.spread(lambda: L.kmt_vt(mech)))
        measured["st_coeff"] = max(measured.get("st_coeff", 0.0), L.spread(lambda: L.stc_compute(mech)))
    for mech in ("gas", "aer", "tot"):
        # xeq and the gas routine's henry4: columns 1.. of each case's tuple (column 0, xkmtd, has no exp)
        measured["dry_rates"] = max(measured.get("dry_rates", 0.0), L.spread(lambda: [a for case in L.dry_compute(mech) for a in case[1:]]))
    with capsys.disabled():
        print("\n    movement of the restatements under last-place freedom: " + "  ".join("%s %.2e" % kv for kv in sorted(measured.items())))
    assert set(measured) == set(LIQ_SYNTH_RTOL)
    for name, s in measured.items():
        assert s > 0.0, name
        check_constant("LIQ_SYNTH_RTOL[%s]" % name, LIQ_SYNTH_RTOL[name], s, floor=LIQ_SYNTH_FLOOR)
    assert L.kmt_py.math is math and L.liq_py.math is math and L.rates_py.math is math
