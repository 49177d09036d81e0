"""Chain passes of the gather-sum machine (schedule.hpp: GsumChain), on the host: the programs the kernel runs for Vdot — lean rows plus
chain passes — are evaluated by the restatement of tests/gsum_chain_host.py (numpy float64, one rounding per operation, a chain step as
A + p) and held to the full program's sums bit for bit, for gas, aer, tot and both demo slots.  Only Vdot sums are chained: the JVS program
has no passes, so there is no chained JVS output whose ownership could be checked."""
import ctypes

import numpy as np
import pytest

import gsum_chain_host as H

MECHS = ["gas", "aer", "tot", "demo_g", "demo_a"]


@pytest.fixture(scope="module")
def lib():
    return H.load_lib()


@pytest.fixture(scope="module")
def programs(lib):
    n = 3 + lib.mistra_chem_user_mechs()
    lib.mistra_chem_mech_name.restype = ctypes.c_char_p
    out = {}
    for mech in range(n):
        name = lib.mistra_chem_mech_name(mech).decode()
        nvar = ctypes.c_int()
        assert lib.mistra_chem_dims(mech, ctypes.byref(nvar), None, None, None) == 0
        out[name] = dict(nvar=nvar.value, full=H.program(lib, mech, H.FULL_VDOT), lean=H.program(lib, mech, H.LEAN_VDOT),
                         passes=H.program(lib, mech, H.PASSES), jvs=H.program(lib, mech, H.JVS))
    return out


def vdot_out(P, nvar, mask=None):
    """ros3_kernel.hip: vdot_out — where lane t's outputs go"""
    nt, nq = P["nt"], P["nq"]
    t = np.arange(nt)
    addr = np.where(t < nvar, P["xs"] + 8 * t, P["trash"]).astype(np.int64)
    if nq == 1:
        stride = np.where(t < nvar, 8 * nt, 0).astype(np.int64)
    else:
        stride = np.where(t + nt < nvar, 8 * nt, P["trash"] - addr).astype(np.int64)
    if mask is not None:
        for w in range(P["nw"]):
            for l in range(64):
                if (int(mask[w]) >> l) & 1:
                    addr[w * 64 + l] = P["trash"]
    return addr, stride


def image(Q, seed, specials):
    """an LDS image whose source array holds seeded values of mixed sign and size with +0.0, -0.0 and subnormals among them; specials:
    (cell, value) pairs written on top"""
    P = Q["full"]
    top = max(int((Q[k]["recs"][:, :, :4] & ~np.uint32(7)).max()) for k in ("full", "lean", "passes")) // 8 + 2
    rng = np.random.default_rng(seed)
    M = np.zeros(max(top, P["trash"] // 8 + 2))
    nsrc = top - P["src"] // 8
    v = rng.standard_normal(nsrc) * 10.0 ** rng.integers(-12, 12, nsrc)
    kind = rng.integers(0, 12, nsrc)
    v[kind == 0] = 0.0
    v[kind == 1] = -0.0
    v[kind == 2] = 5e-324 * rng.integers(1, 1 << 40, (kind == 2).sum())
    v[kind == 3] = -5e-324 * rng.integers(1, 1 << 40, (kind == 3).sum())
    M[P["src"] // 8:top] = v
    for cell, value in specials:
        M[cell] = value
    M[P["zero"] // 8] = 0.0
    return M


def chained_source_cells(Q):
    """source cells (indices into M) of the terms of the chained sums, per chained species"""
    P = Q["passes"]
    cells = {}
    for w in range(P["nw"]):
        for p in range(int(P["rows"][w]) // 2):
            r0, r1 = P["recs"][int(P["wave_base"][w]) + 2 * p], P["recs"][int(P["wave_base"][w]) + 2 * p + 1]
            if int(r0[0, 0] & 7) == 0:
                continue
            addr = np.concatenate([r0[:, :4], r1[:, :3]], axis=1).astype(np.int64) & ~7
            for R in range(4):
                out = int(r1[16 * R, 3]) // 8
                if out == P["trash"] // 8:      # a 16-lane row without a sum
                    continue
                cells[out] = sorted(set(int(a) // 8 for a in addr[16 * R:16 * R + 16].ravel()) - {P["zero"] // 8})
    return cells


def evaluate(Q, M0):
    nvar = Q["nvar"]
    Mf, Mk = M0.copy(), M0.copy()
    H.run_rows(Q["full"], Mf, *vdot_out(Q["full"], nvar))
    stores = H.run_rows(Q["lean"], Mk, *vdot_out(Q["lean"], nvar, Q["passes"]["mask"]))
    for cell, n in H.run_passes(Q["passes"], Mk).items():
        stores[cell] = stores.get(cell, 0) + n
    xs = Q["full"]["xs"] // 8
    return Mf[xs:xs + nvar], Mk[xs:xs + nvar], stores


@pytest.mark.parametrize("name", MECHS)
def test_kernel_programs_equal_the_full_sums(programs, name):
    if name not in programs:
        pytest.skip("the library was built without this user slot")
    Q = programs[name]
    xs = Q["full"]["xs"] // 8
    chained = chained_source_cells(Q)
    cases = [("finite", [])]
    if chained:
        some = [c for cells in chained.values() for c in cells[:3]]
        cases.append(("zeros", [(c, (0.0, -0.0)[i & 1]) for i, c in enumerate(some)]))
        cases.append(("nan", [(cells[len(cells) // 2], np.nan) for cells in list(chained.values())[::2]]))
        cases.append(("inf", [(cells[0], np.inf) for cells in chained.values()]))
        cases.append(("subnormal", [(c, 5e-324 * (3 + i)) for i, c in enumerate(some)]))
    for seed, (label, specials) in enumerate(cases):
        full, kern, stores = evaluate(Q, image(Q, 100 + seed, specials))
        nan = np.isnan(full)
        assert (np.isnan(kern) == nan).all(), (name, label)
        assert (full[~nan].view(np.uint64) == kern[~nan].view(np.uint64)).all(), (name, label)
        if label in ("nan", "inf"):
            assert (~np.isfinite(full)).any(), "the special value reaches a chained sum"
        # every species' cell is written exactly once, by its lane's flush or by a pass
        assert all(stores.get(xs + s, 0) == 1 for s in range(Q["nvar"])), (name, label)


@pytest.mark.parametrize("name", MECHS)
def test_mask_and_passes_agree(programs, name):
    if name not in programs:
        pytest.skip("the library was built without this user slot")
    Q = programs[name]
    P, nt = Q["passes"], Q["passes"]["nt"]
    chained = sorted(int(s) for s in P["chained"] if s >= 0)
    masked = sorted(w * 64 + l for w in range(P["nw"]) for l in range(64) if (int(P["mask"][w]) >> l) & 1)
    assert chained == masked and all(s < Q["nvar"] for s in chained)
    assert not chained or (Q["passes"]["nq"] == 0 and Q["lean"]["nq"] == 1 and nt >= Q["nvar"])
    assert sorted(chained_source_cells(Q)) == [Q["full"]["xs"] // 8 + s for s in chained]
    assert bool(P["on"]) == bool(chained) == bool(P["npass"])
    for p, w in enumerate(P["pass_wave"]):
        assert 0 <= w < P["nw"]
    assert int(P["rows"].sum()) >= 2 * P["npass"] and (P["rows"] % 4 == 0).all() and (Q["lean"]["rows"] % 4 == 0).all()


@pytest.mark.parametrize("name", ["gas", "aer", "demo_g", "demo_a"])
def test_mechanisms_without_the_trait_run_the_full_program(programs, name):
    if name not in programs:
        pytest.skip("the library was built without this user slot")
    Q = programs[name]
    assert not Q["passes"]["on"] and Q["passes"]["npass"] == 0 and not Q["passes"]["rows"].any() and not Q["passes"]["mask"].any()
    assert Q["lean"]["recs"].tobytes() == Q["full"]["recs"].tobytes()
    assert (Q["lean"]["rows"] == Q["full"]["rows"]).all() and (Q["lean"]["wave_base"] == Q["full"]["wave_base"]).all()


def test_tot_pole_is_shorter(programs):
    Q = programs["tot"]
    P = Q["passes"]
    print("tot Vdot rows per wave: full", Q["full"]["rows"].tolist(), "lean", Q["lean"]["rows"].tolist(), "pass rows", P["rows"].tolist(),
          "passes on waves", P["pass_wave"].tolist(), "chained species", [int(s) for s in P["chained"]])
    print("pole rows %d -> %d, modelled ticks (fun_jac + fun) %d -> %d" % (P["pole_rows_full"], P["pole_rows_lean"], P["pole_cycles_full"], P["pole_cycles_lean"]))
    assert P["on"]
    assert P["pole_rows_lean"] < P["pole_rows_full"] and P["pole_cycles_lean"] < P["pole_cycles_full"]
    assert int(Q["lean"]["rows"].max()) == P["pole_rows_lean"] and int(Q["full"]["rows"].max()) == P["pole_rows_full"]
