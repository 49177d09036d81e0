"""The liq_parm device kernels (mistra_amd/csrc/pack.hip, the st_coeff programs through rates.hip) on the seeded cases of tests/liq_cases.py (-m gpu),
against the order-faithful restatements that tests/test_pack.py and tests/test_rates.py pin to the captured layers.  The captured fixtures reach one ka,
one kw vector, ifeed = 0, no droplet bin and 281-288 K; these cases reach the empty, one-row, exact and ragged bins of fast_k_mt_kernel's chunk pipeline,
every chunking of cw_rc_kernel's grid and every row of its on/off table, the second block and the rcd <= 0 branch of dry_rates_kernel, and the model's
temperature range — tests/test_liq_cases.py holds, on the CPU, that they do.

What has no library function in it is compared bit for bit on WHOLE arrays that start from a poison different in every entry: what a routine must leave
alone is read back from it.  What passes through exp / log is held to tests/parity_bounds.py: LIQ_SYNTH_RTOL (10x the restatements' own movement under
last-place freedom, at least 1e-14), entry by entry — an entry that is 0 in the restatement is 0 on the device.  Each test also runs a few layers one
call each: the same bits as in the batch.

ifeed = 2 (the first aerosol class left out of bins 1 and 3: `ial = 2` in kpp.f90:2258-2262 for cw_rc and kpp.f90:4638-4642 for dry_cw_rc, `iia_0 = 2` in
kpp.f90:2606-2607 | 2877-2878 for fast_k_mt_t | fast_k_mt_a) cannot be captured from the namelist the fixtures come from; it is covered here by the restatements alone."""
import numpy as np
import pytest

import liq_cases as L
from parity_bounds import LIQ_SYNTH_RTOL

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem
    chem.init(0)
    dev = torch.device("cuda", 0)
    return torch, chem, (lambda a: torch.tensor(np.ascontiguousarray(a), device=dev))


def _bounded(name, what, got, want, tally):
    ok, worst, same = L.close(got, want, LIQ_SYNTH_RTOL[name])
    tally[0] += int(np.asarray(want).size - same)
    tally[1] = max(tally[1], worst)
    assert ok, "%s: %s differs from the restatement by %.3e (bound %.1e)" % (name, what, worst, LIQ_SYNTH_RTOL[name])


def _run_kmt(chem, T, mech, c, sl, with_vt=True):
    xk, vt = T(c["xkmt0"][sl]), T(c["vt0"][sl])
    a = (mech, T(c["ff"][sl]), T(c["rq"]), c["kw"], c["ka"], c["ifeed"], c["nkc_l"], T(c["cw"][sl]), T(c["cm"][sl]), T(c["freep"][sl]), T(c["alpha"][sl]), T(c["vmean"][sl]), xk)
    if with_vt:
        chem.fast_k_mt(*a, T(c["t"][sl]), T(c["p"][sl]), vt)
    else:
        chem.fast_k_mt(*a)
    return xk.cpu().numpy(), vt.cpu().numpy()


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_mass_transfer_coefficients_of_seeded_layers(mech):
    """fast_k_mt_kernel over liq_cases.KMT_CALLS: xkmt bit for bit (poison kept where cm <= 0 or cw <= 0 or kc > nkc_l or the species is not exchanged),
    vt of the Stokes-only layer bit for bit, vt elsewhere within LIQ_SYNTH_RTOL['vt'] (poison kept where cw <= 0)."""
    torch, chem, T = _gpu()
    calls, exp = L.kmt_calls(mech), L.kmt_expected(mech)
    bits, tally = 0, [0, 0.0]
    for ci, (c, (xk_want, vt_want)) in enumerate(zip(calls, exp)):
        what = "call %d (ka %d, ifeed %d, nkc_l %d)" % (ci, c["ka"], c["ifeed"], c["nkc_l"])
        xk, vt = _run_kmt(chem, T, mech, c, slice(None))
        assert np.array_equal(xk, xk_want), "xkmt of %s: %d entries differ, layers / bins %s" % (
            what, int((xk != xk_want).sum()), sorted({(int(i), int(b) + 1) for i, b, _ in zip(*np.nonzero(xk != xk_want))}))
        bits += xk.size
        keep = (c["cw"] <= 0) | (np.arange(L.NKC)[None, :] >= c["nkc_l"])
        assert np.array_equal(vt[keep], c["vt0"][keep]), "vt of %s written for a bin without liquid water" % what
        assert np.array_equal(vt[c["stokes"]], vt_want[c["stokes"]]), "vt of the Stokes-only layer of %s" % what
        bits += int(keep.sum() + (~keep[c["stokes"]]).sum())
        _bounded("vt", "vt of " + what, vt, vt_want, tally)
        x2, v2 = _run_kmt(chem, T, mech, c, slice(None), with_vt=False)      # the xkmt half alone: same bits, vt untouched
        assert np.array_equal(x2, xk) and np.array_equal(v2, c["vt0"])
        for i in range(len(c["t"])):                                          # one layer per call
            x1, v1 = _run_kmt(chem, T, mech, c, slice(i, i + 1))
            assert np.array_equal(x1[0], xk[i]) and np.array_equal(v1[0], vt[i]), "layer %d of %s alone differs from the batch" % (i, what)
    print("%s fast_k_mt: %d entries bit for bit (xkmt whole, vt kept or Stokes); %d vt entries not bit-identical, worst %.2e (bound %.1e)" % (
        mech, bits, tally[0], tally[1], LIQ_SYNTH_RTOL["vt"]))
    # ---- what the host refuses (nothing is launched)
    c = calls[0]
    x = T(c["xkmt0"])
    a = lambda kw, ka, nkc_l: (mech, T(c["ff"]), T(c["rq"]), kw, ka, c["ifeed"], nkc_l, T(c["cw"]), T(c["cm"]), T(c["freep"]), T(c["alpha"]), T(c["vmean"]), x)
    kw_bad = np.array(c["kw"])
    kw_bad[5] = c["rq"].shape[1] + 1
    for bad in ((kw_bad, c["ka"], 4), (c["kw"], c["rq"].shape[0] + 1, 4), (c["kw"], c["ka"], 0)):
        with pytest.raises(chem.MistraChemError):
            chem.fast_k_mt(*a(*bad))
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), c["xkmt0"])


def test_particle_bin_moments_of_seeded_grids():
    """cw_rc_kernel over liq_cases.CWRC_CALLS, wet and dry: every output of every layer bit for bit."""
    torch, chem, T = _gpu()
    calls, exp = L.cwrc_calls(), L.cwrc_expected()
    bits = 0
    for c, (wet_want, dry_want) in zip(calls, exp):
        what = "grid %d x %d, ka %d, ifeed %d" % (c["nka"], c["nkt"], c["ka"], c["ifeed"])
        a = (c["rq"], c["e"], c["kw"], c["ka"], c["ifeed"])
        wet = chem.cw_rc(c["ff"], *a, c["feu"], c["cloud"], c["crys4"])
        for got, want, key in zip(wet, wet_want, ("rc", "cw", "cm", "conv2", "below")):
            assert np.array_equal(got, want), "%s of %s: layers / bins %s" % (key, what, np.argwhere(got != want).tolist()[:8])
            bits += got.size
        dry = chem.cw_rc(c["ff"], *a, dry=True)
        for got, want, key in zip(dry, dry_want, ("rcd", "cwd")):
            assert np.array_equal(got, want), "%s of %s: layers / bins %s" % (key, what, np.argwhere(got != want).tolist()[:8])
            bits += got.size
        for i in (0, len(c["feu"]) - 1):                                      # one layer per call
            one = chem.cw_rc(c["ff"][i:i + 1], *a, c["feu"][i:i + 1], c["cloud"][i:i + 1], c["crys4"])
            assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, wet)), "layer %d of %s alone differs from the batch" % (i, what)
            one = chem.cw_rc(c["ff"][i:i + 1], *a, dry=True)
            assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, dry))
    print("cw_rc / dry_cw_rc: %d entries of %d calls bit for bit" % (bits, len(calls)))
    # ---- what the host refuses
    c = calls[0]
    kw_bad = np.array(c["kw"])
    kw_bad[3] = c["nkt"] + 1
    with pytest.raises(chem.MistraChemError):
        chem.cw_rc(c["ff"], c["rq"], c["e"], kw_bad, c["ka"], c["ifeed"], c["feu"], c["cloud"], c["crys4"])
    with pytest.raises(chem.MistraChemError):
        chem.cw_rc(c["ff"], c["rq"], c["e"], c["kw"], c["nka"] + 1, c["ifeed"], c["feu"], c["cloud"], c["crys4"])
    with pytest.raises(chem.MistraChemError):
        chem.cw_rc(np.zeros((1, 1, 2049)), np.ones((1, 2049)), np.ones(2049), np.zeros(1, np.int32), 0, 0, dry=True)


@pytest.mark.parametrize("mech", ["gas", "aer", "tot"])
def test_dry_aerosol_uptake_of_seeded_layers(mech):
    """dry_rates_kernel at 1, 64, 65 and 200 layers: xkmtd bit for bit (aer, tot: the speeds come in; gas: IEEE square root), 0 exactly where rcd <= 0;
    xeq and the gas routine's Henry constants within LIQ_SYNTH_RTOL['dry_rates'], entries <= 0 of henry4 kept."""
    torch, chem, T = _gpu()
    cases, exp = L.dry_cases(mech), L.dry_expected(mech)
    bits, tally = 0, [0, 0.0]
    for c, want in zip(cases, exp):
        a = (c["tt"], c["freep"], c["rcd"])
        got = chem.dry_rates(*a, None, c["henry4"]) if mech == "gas" else chem.dry_rates(*a, c["vmean4"])
        what = "%d layers" % len(c["tt"])
        assert np.array_equal(got[0], want[0]), "xkmtd of %s" % what
        bits += got[0].size
        _bounded("dry_rates", "xeq of " + what, got[1], want[1], tally)
        if mech == "gas":
            _bounded("dry_rates", "henry4 of " + what, got[2], want[2], tally)
            kept = c["henry4"][:, 1:] <= 0
            assert np.array_equal(got[2][:, 1:][kept], c["henry4"][:, 1:][kept])
            assert np.array_equal(got[2][:, 1:], want[2][:, 1:]), "henry4 of %s: 1/(h*FCT) has no library function in it" % what
            bits += got[2][:, 1:].size
        for i in (0, len(c["tt"]) - 1):
            one = chem.dry_rates(*(x[i:i + 1] for x in a), None, c["henry4"][i:i + 1]) if mech == "gas" else chem.dry_rates(*(x[i:i + 1] for x in a), c["vmean4"][i:i + 1])
            assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, got))
    print("%s dry_rates: %d entries bit for bit; %d of xeq / henry4 not bit-identical, worst %.2e (bound %.1e)" % (mech, bits, tally[0], tally[1], LIQ_SYNTH_RTOL["dry_rates"]))


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_henry_speeds_and_equilibria_of_seeded_layers(mech):
    """henry_kernel, v_mean_kernel and equil_co_kernel at 1 and 300 layers, 200-320 K: v_mean and every entry without exp bit for bit, the others within
    LIQ_SYNTH_RTOL; equilibrium constants of bins with conv2 <= 0 exactly 0, of bins and species the routine does not set the poison they held."""
    torch, chem, T = _gpu()
    cases, exp = L.liq_cases(mech), L.liq_expected(mech)
    h_exp, h_plain = L.henry_exp_species(mech)
    f_exp, f_plain, b_exp, b_plain = L.equil_exp_species(mech)
    ns = L.nspec(mech)
    bits, th, te = 0, [0, 0.0], [0, 0.0]

    def run(c, sl):
        nl = len(c["tt"][sl])
        h = torch.full((nl, ns), float("nan"), dtype=torch.float64, device="cuda:0")
        v = torch.full((nl, ns), float("nan"), dtype=torch.float64, device="cuda:0")
        chem.henry(mech, T(c["tt"][sl]), h)
        chem.v_mean(mech, T(c["tt"][sl]), v)
        ef, eb = T(c["xkef0"][sl]), T(c["xkeb0"][sl])
        chem.equil_co(mech, T(c["tt"][sl]), T(c["conv2"][sl]), T(c["xgamma"][sl]), ef, eb)
        torch.cuda.synchronize()
        return h.cpu().numpy(), v.cpu().numpy(), ef.cpu().numpy(), eb.cpu().numpy()

    for c, e in zip(cases, exp):
        what = "%d layers" % len(c["tt"])
        h, v, ef, eb = run(c, slice(None))
        assert np.array_equal(v, e["vmean"]), "v_mean of %s" % what
        rest = np.setdiff1d(np.arange(ns), h_exp)
        assert np.array_equal(h[:, rest], e["henry"][:, rest]), "henry of %s, species without a temperature law" % what
        _bounded("henry", "henry of " + what, h, e["henry"], th)
        bits += v.size + h[:, rest].size
        for got, want, ex, key in ((ef, e["xkef"], f_exp, "xkef"), (eb, e["xkeb"], b_exp, "xkeb")):
            rest = np.setdiff1d(np.arange(ns), ex)
            assert np.array_equal(got[:, :, rest], want[:, :, rest]), "%s of %s: entries without exp, dry bins, untouched entries" % (key, what)
            _bounded("equil_co", key + " of " + what, got, want, te)
            bits += got[:, :, rest].size
        for i in (0, len(c["tt"]) - 1):
            one = run(c, slice(i, i + 1))
            assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, (h, v, ef, eb)))
    print("%s henry / v_mean / equil_co: %d entries bit for bit; henry %d not bit-identical, worst %.2e (bound %.1e); xkef / xkeb %d, worst %.2e (bound %.1e)" % (
        mech, bits, th[0], th[1], LIQ_SYNTH_RTOL["henry"], te[0], te[1], LIQ_SYNTH_RTOL["equil_co"]))


@pytest.mark.parametrize("mech", ["aer", "tot"])
def test_accommodation_coefficients_of_seeded_layers(mech):
    """the st_coeff programs at 1 and 300 layers under every setting of lpJoyce14bc and lpBuxmann15alph, 230-310 K, cw(1), cm(1) and the two sion1 entries at
    0 and positive: coefficients without a library function bit for bit, the others within LIQ_SYNTH_RTOL['st_coeff']; the whole array written."""
    torch, chem, T = _gpu()
    cases, exp = L.stc_cases(mech), L.stc_expected(mech)
    ns = L.nspec(mech)
    bits, tally = 0, [0, 0.0]
    for s, (jo, bu) in enumerate(L.STC_SWITCHES):
        plain = L.stc_plain_species(mech, jo, bu)
        for ci, env in enumerate(cases):
            want = exp[2 * s + ci]

            def run(sl):
                out = torch.full((len(env[sl]), ns), float("nan"), dtype=torch.float64, device="cuda:0")
                chem.st_coeff(mech, T(env[sl]), out, jo, bu)
                torch.cuda.synchronize()
                return out.cpu().numpy()

            got = run(slice(None))
            what = "%d layers, lpJoyce14bc %s, lpBuxmann15alph %s" % (len(env), jo, bu)
            assert np.isfinite(got).all()
            assert np.array_equal(got[:, plain], want[:, plain]), "alpha of %s: literal coefficients" % what
            bits += got[:, plain].size
            _bounded("st_coeff", "alpha of " + what, got, want, tally)
            for i in (0, len(env) - 1):
                assert np.array_equal(run(slice(i, i + 1))[0], got[i])
    print("%s st_coeff: %d entries bit for bit; %d not bit-identical, worst %.2e (bound %.1e)" % (mech, bits, tally[0], tally[1], LIQ_SYNTH_RTOL["st_coeff"]))
