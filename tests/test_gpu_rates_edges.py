"""Update_RCONST_x on the device (-m gpu) at the rate laws' guards and at the batch sizes where the launch changes shape.  The inputs are the edge cases
of tests/rates_cases.py (tests/test_rates_cases.py proves on the CPU that each guard, clamp and threshold is reached by one of them); the expected
values are the COMPILED REFERENCE's (tests/golden/rates_edges_<mech>.npz, tests/golden/make_rates_edges_golden.py).

  edges        through mistra_chem_update_rconst_device into a caller-owned, poisoned output of ncell + 1 rows: every row written in full, the row
               behind untouched, zeros and NaN where the reference has them, programs without a library call bit for bit, the others to
               parity_bounds.RATES_EDGES_RTOL (10x the restatement's own movement under last-place freedom of exp / pow / log10, floor 1e-13)
  batch shape  the kernel cuts the cells into blocks of 64 lanes and the reactions into 4 * gy chunks, gy from the cell count: a cell's row is the same
               bits whatever the count — 1 cell to 131 073, idle lanes, the capped split, a split in between and gy = 1
  env <- C     mistra_chem_rates_env_from_c_device writes the concentration slots and nothing else
  host path    mistra_chem_update_rconst (numpy in, numpy out) gives the device-buffer path's bits

Tried against this file with a scratch copy of rates.hip: `d > 0.0` -> `d >= 0.0` in uplim, uplim's max(c, 0) dropped, `r < r_end` -> `r < r_end - 1`:
each fails the edge test (the last one the batch-shape and host-path tests too)."""
import ctypes as C
import os

import numpy as np
import pytest

import liq_cases
import parity_bounds as pb
import rates_cases as rc
from conftest import REPO

pytestmark = pytest.mark.gpu
MECH_ID = {"gas": 0, "aer": 1, "tot": 2}


@pytest.fixture(scope="module")
def chem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mistra_amd import chem as c
    c.init(0)
    return c


def _device_rconst(chem, mech, env, extra_rows=0, base=7000.0):
    """mistra_chem_update_rconst_device on a device copy of env [ncell, nenv] into a caller-owned output of ncell + extra_rows rows filled with
    liq_cases.poison's values (made on the device: the big batches put nothing on the host) -> (output tensor, poison tensor)"""
    import torch
    dev = torch.device("cuda", 0)
    nreact = chem.DIMS[mech][2]
    ncell = env.shape[0]
    poison = (-(base + 0.5 * torch.arange((ncell + extra_rows) * nreact, dtype=torch.float64, device=dev))).view(ncell + extra_rows, nreact)
    out = poison.clone() if extra_rows else poison
    e = env if isinstance(env, torch.Tensor) else torch.tensor(np.ascontiguousarray(env), device=dev)
    assert e.is_contiguous() and e.shape[1] == chem.lib().mistra_chem_rates_env_size(MECH_ID[mech])
    rc_ = chem.lib().mistra_chem_update_rconst_device(MECH_ID[mech], ncell, e.data_ptr(), out.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc_ == 0, chem.lib().mistra_chem_last_error()
    torch.cuda.synchronize()
    return out, (poison[ncell:] if extra_rows else None)


@pytest.mark.parametrize("mech", rc.MECHS)
def test_edge_cases_against_the_compiled_reference(chem, mech):
    fx = rc.fixture(mech)
    env, want = fx["env"], fx["rconst"]
    ncell = env.shape[0]
    out, behind = _device_rconst(chem, mech, env, extra_rows=1)
    got = out.cpu().numpy()
    poison = liq_cases.poison((ncell + 1, want.shape[1]), 7000.0)
    assert np.array_equal(behind.cpu().numpy()[0], poison[ncell])
    assert np.array_equal(got[ncell], poison[ncell]), "the row behind the last cell was written"
    got = got[:ncell]
    assert not (got == poison[:ncell]).any(), "%d entries were not written" % int((got == poison[:ncell]).sum())
    names = rc.cases(mech)["names"]
    for i in range(ncell):
        assert np.array_equal(np.isnan(got[i]), np.isnan(want[i])), "%s, case %r: NaN in other places than the reference" % (mech, names[i])
        assert np.array_equal(got[i] == 0.0, want[i] == 0.0), "%s, case %r: zeros in other places: reactions %s" % (
            mech, names[i], np.nonzero((got[i] == 0.0) != (want[i] == 0.0))[0][:8].tolist())
        assert np.array_equal(np.isinf(got[i]), np.isinf(want[i])), "%s, case %r" % (mech, names[i])
    plain, libfree, lib = rc.program_kinds(mech)
    exact = plain | libfree
    for i in range(ncell):
        assert rc.same_bits(got[i][exact], want[i][exact]), "%s, case %r: library-free reactions %s differ" % (
            mech, names[i], np.nonzero(exact)[0][~((got[i][exact] == want[i][exact]) | np.isnan(want[i][exact]))][:8].tolist())
    g, w = got[:, lib], want[:, lib]
    fin = np.isfinite(w) & (w != 0.0)
    assert np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)])
    rel = np.abs(g[fin] - w[fin]) / np.abs(w[fin])
    worst = np.nonzero(fin)[0][np.argmax(rel)]
    print("%s: %d edge cases; %d library-free entries bit for bit; %d entries through exp / pow / log10: %.1f %% bit-identical, max rel diff %.2e (case %r), bound %.1e"
          % (mech, ncell, int(exact.sum()) * ncell, int(fin.sum()), 100.0 * float((g[fin] == w[fin]).mean()), rel.max(), names[worst], pb.RATES_EDGES_RTOL[mech]))
    assert rel.max() <= pb.RATES_EDGES_RTOL[mech]


def test_batch_sizes_reach_every_launch_shape():
    for mech in rc.MECHS:
        nreact = {"gas": 331, "aer": 979, "tot": 1627}[mech]
        cap = (nreact + 15) // 16
        gys = {n: rc.launch_gy(n, nreact) for n in rc.BATCH_NCELL}
        assert gys[148] == cap and gys[1] == cap, gys                     # a column's worth of cells: the capped split
        assert gys[131073] == 1, gys
        assert any(1 < g < cap for g in gys.values()), (mech, gys)       # and a split in between
    assert {1, 63, 64, 65, 129, 148, 6401, 131073} <= set(rc.BATCH_NCELL)


@pytest.mark.parametrize("mech", rc.MECHS)
def test_a_cells_row_does_not_depend_on_the_batch(chem, mech):
    """48 seeded rows + the edge rows, tiled on the device to every size of rates_cases.BATCH_NCELL: each cell's row is bit-identical (NaN included: the
    comparison is on the bit patterns, on the device) to the same env row evaluated in a batch of 48."""
    import torch
    dev = torch.device("cuda", 0)
    rows = np.concatenate([np.load(os.path.join(REPO, "tests", "golden", "rates_%s.npz" % mech))["env"][:48], rc.fixture(mech)["env"]])
    nb = rows.shape[0]
    assert nb > 48 and np.isnan(rows).any()
    rows_d = torch.tensor(rows, device=dev)
    ref = []
    for i in range(0, nb, 48):      # batches of exactly 48 (the last one is filled up from the front)
        idx = torch.arange(i, i + 48, device=dev) % nb
        out, _ = _device_rconst(chem, mech, rows_d[idx].contiguous())
        ref.append(out[: min(48, nb - i)])
    ref = torch.cat(ref).contiguous().view(torch.int64)
    nreact = ref.shape[1]
    for ncell in rc.BATCH_NCELL:
        env = rows_d[torch.arange(ncell, device=dev) % nb].contiguous()
        out, behind = _device_rconst(chem, mech, env, extra_rows=1, base=9000.0)
        del env
        assert torch.equal(out[ncell:], behind), "ncell = %d: the row behind the last cell was written" % ncell
        bits = out.view(torch.int64)
        full = ncell // nb
        if full:
            assert bool((bits[: full * nb].view(full, nb, nreact) == ref[None]).all()), "%s, ncell = %d (gy = %d)" % (mech, ncell, rc.launch_gy(ncell, nreact))
        assert torch.equal(bits[full * nb:ncell], ref[: ncell - full * nb]), "%s, ncell = %d (gy = %d)" % (mech, ncell, rc.launch_gy(ncell, nreact))
        del out, bits
    # ... and the batch of 48 is what the reference comparison above saw: the edge rows evaluated alone
    alone, _ = _device_rconst(chem, mech, rows_d[48:].contiguous())
    assert torch.equal(alone.view(torch.int64), ref[48:])


@pytest.mark.parametrize("mech", rc.MECHS)
@pytest.mark.parametrize("ncell", [1, 255, 256, 257, 1000])
def test_rates_env_from_c_fills_the_concentration_slots_only(chem, mech, ncell):
    """index-coded VAR / FIX: entry i of cell k is k + (i + 1) / 1024 (VAR) or -(k + (i + 1) / 1024) (FIX), exact in a double"""
    import re
    import torch
    dev = torch.device("cuda", 0)
    nvar, nfix = chem.DIMS[mech][:2]
    names = rc.env_info(mech)[0]
    cell = np.arange(ncell, dtype=np.float64)[:, None]
    var = cell + (np.arange(nvar) + 1.0)[None, :] / 1024.0
    fix = -(cell + (np.arange(nfix) + 1.0)[None, :] / 1024.0)
    poison = liq_cases.poison((ncell + 1, len(names)), 5000.0) * 1024.0      # (no multiple of 1/1024 between two cells' codes collides with it: it is below -5e6)
    env = torch.tensor(poison, device=dev)
    g = np.load(os.path.join(REPO, "tests", "golden", "drive_%s.npz" % mech))      # (the hand-over entries want the model's species maps set; this one reads none)
    chem.set_species_maps(mech, g["gas_m2k"], g["gas_k2m"], g["rad_m2k"], g["rad_k2m"])
    chem.rates_env_from_c(mech, torch.tensor(var, device=dev), torch.tensor(fix, device=dev), env)
    torch.cuda.synchronize()
    got = env.cpu().numpy()
    want = poison.copy()
    c = np.concatenate([var, fix], axis=1)
    filled = 0
    for i, nm in enumerate(names):
        m = re.match(r"(c|fix)\((\d+)\)$", nm)
        if m:
            want[:ncell, i] = c[:, int(m.group(2)) - 1] if m.group(1) == "c" else fix[:, int(m.group(2)) - 1]
            filled += 1
    assert filled >= 6
    assert np.array_equal(got, want), "slots %s" % sorted({names[j] for j in np.nonzero(got != want)[1]})[:8]


@pytest.mark.parametrize("mech", rc.MECHS)
def test_host_buffer_path_gives_the_device_buffer_paths_bits(chem, mech):
    env = rc.fixture(mech)["env"]
    out, _ = _device_rconst(chem, mech, env)
    host = chem.update_rconst(mech, np.array(env))
    assert host.shape == tuple(out.shape)
    assert np.array_equal(host.view(np.int64), out.cpu().numpy().view(np.int64))
