"""The user mechanism slots without a GPU: the derivation tool (mistra_amd/mechderive.py, tools/derive_mech.py), the two demo tables, the oracle and
the schedule emulator on them, the generated traits and the size-class rule, the C ABI's answers that need no device, and the bounds the GPU tests
(tests/test_gpu_user_mech.py) use."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import user_mech_bounds as ub
import user_mech_cases as uc
from conftest import REPO, load_golden
from test_schedule import emu, test_programs_match_oracle as programs_match_oracle      # noqa: F401  (the fixture and the checks of the shipped tables)

MECH_DIR = os.path.join(REPO, "mistra_amd", "mech")
DEMO_NAMES = tuple(uc.DEMOS)


def _raw(name, ext=".mech"):
    with open(os.path.join(MECH_DIR, name + ext), "rb") as f:
        return f.read()


@pytest.fixture(scope="module", autouse=True)
def demo_tables():
    uc.ensure_tables()


@pytest.fixture(scope="module")
def demo_oracles():
    from oracle.oracle import Oracle
    return {n: Oracle(n) for n in DEMO_NAMES}


@pytest.mark.parametrize("mech", ["gas", "aer", "tot"])
def test_identity_derivation_reproduces_the_shipped_tables(mech, tmp_path):
    """Nothing dropped: the filtered lists are the source's and the symbolic fill-in of the structural pattern is LU_CROW / LU_ICOL — byte for byte,
    through the module and through the command line."""
    import subprocess
    import sys
    from mistra_amd import mechderive, mechtab
    tab, maps = mechderive.derive(mechtab.load(mech))
    assert mechderive.table_bytes(tab) == _raw(mech)
    assert maps["kept_reactions"] == list(range(tab["nreact"])) and maps["kept_species"] == list(range(tab["nvar"]))
    out = tmp_path / (mech + "_id.mech")
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "derive_mech.py"), os.path.join(MECH_DIR, mech + ".mech"), str(out)], check=True,
                   stdout=subprocess.DEVNULL)
    assert out.read_bytes() == _raw(mech) and (tmp_path / (mech + "_id.json")).exists()


@pytest.mark.parametrize("name", DEMO_NAMES)
def test_demo_tables_regenerate_from_their_rule(name):
    from mistra_amd import mechderive, mechtab
    source, removed = uc.DEMOS[name]
    import hashlib
    tab, maps, species, drop = uc.derive_demo(name)
    # the derivation, the table on disk (derived, not committed) and the committed index map against the digests pinned in tests/user_mech_cases.py:
    # nothing here is compared with what the same run has just written
    sha = lambda raw: hashlib.sha256(raw).hexdigest()
    assert sha(mechderive.table_bytes(tab)) == uc.SHA256[name + ".mech"], "the derivation of %s no longer gives the pinned table" % name
    assert sha(mechderive.maps_text(maps).encode()) == uc.SHA256[name + ".json"]
    assert sha(_raw(name)) == uc.SHA256[name + ".mech"], "mistra_amd/mech/%s.mech is not the pinned table" % name
    assert sha(_raw(name, ".json")) == uc.SHA256[name + ".json"], "the committed mistra_amd/mech/%s.json is not the pinned index map" % name
    assert tab["nnz"] == uc.NNZ[name]
    assert len(_raw(name)) <= len(_raw(source))
    src, t = mechtab.load(source), mechtab.load(name)
    assert (t.nvar, t.nfix, t.nreact) == uc.SIZES[name] and len(species) == uc.NSPECIES
    assert len(drop) == {"demo_g": 20, "demo_a": 26}[name] and src.nreact - len(drop) == t.nreact
    part = mechderive.species_reactions(src)
    left = [s for s in range(src.nvar) if part[s] and not (part[s] - set(drop))]
    assert len(left) == 16 and sorted(left) == sorted(species)
    assert t.nnz <= src.nnz
    if removed:       # demo_g: the 16 are gone, and nothing of them is left in a surviving list
        assert sorted(set(range(src.nvar)) - set(maps["kept_species"])) == sorted(left) and t.nvar == 86
        for s in left:
            assert not (part[s] - set(drop))
        assert t.a_fac.max() < t.nvar + t.nfix + t.nconst and t.b_fac.max() < t.nvar + t.nfix + t.nconst
    else:             # demo_a: 257 species, the 16 rows are a bare diagonal with an empty sum
        assert t.nvar == 257 and t.nnz < src.nnz
        bare = [k for k in range(t.nvar) if t.crow[k + 1] - t.crow[k] == 1]
        assert sorted(bare) == sorted(left)
        for k in bare:
            assert t.icol[t.crow[k]] == k and t.jv_ptr[t.crow[k] + 1] == t.jv_ptr[t.crow[k]] and t.vd_ptr[k + 1] == t.vd_ptr[k]
    # the LU pattern is closed under fill-in with the diagonal in every row, columns ascending
    for k in range(t.nvar):
        row = t.icol[t.crow[k]:t.crow[k + 1]]
        assert np.all(np.diff(row) > 0) and t.icol[t.diag[k]] == k


def _shared_slots(name):
    """slots of the demo table's LU pattern and the source's slots of the same (row, column)"""
    from mistra_amd import mechderive, mechtab
    t, src = mechtab.load(name), mechtab.load(uc.DEMOS[name][0])
    sp = mechderive.load_maps(name)["kept_species"]
    where = {}
    for k in range(src.nvar):
        for p in range(src.crow[k], src.crow[k + 1]):
            where[(k, int(src.icol[p]))] = p
    mine, theirs = [], []
    for k in range(t.nvar):
        for p in range(t.crow[k], t.crow[k + 1]):
            q = where.get((sp[k], sp[int(t.icol[p])]))
            if q is not None:
                mine.append(p)
                theirs.append(q)
    assert len(mine) == t.nnz, "the demo pattern is part of the source's"
    return np.array(mine), np.array(theirs)


@pytest.mark.parametrize("name", DEMO_NAMES)
def test_oracle_on_the_demo_table_equals_the_full_mechanism_at_zeroed_rates(name, demo_oracles, oracles):
    """The dropped reactions' terms of the full run are exact zeros (0 * V * V summed in place), so on the kept species and the shared Jacobian slots
    Fun and Jac_SP agree bit for bit for both tables.  demo_a keeps every species — NVAR, and with it the error norm, is the source's — so there the
    whole 10 s run agrees too: VAR, IERR, the eight counters, exit time and last step size.  (demo_g's error norm divides by another NVAR: whole runs
    of it are not held against gas.)"""
    from mistra_amd import mechderive
    source = uc.DEMOS[name][0]
    g = load_golden(source)
    o, full = demo_oracles[name], oracles[source]
    V, F, K = uc.cut_inputs(name, g, uc.CELLS)
    Kz = uc.zeroed_rates(name, g, uc.CELLS)
    sp = np.array(mechderive.load_maps(name)["kept_species"])
    mine, theirs = _shared_slots(name)
    for i, c in enumerate(uc.CELLS):
        assert np.array_equal(o.fun(V[i], F[i], K[i]), full.fun(g["var_in"][c], g["fix"][c], Kz[i])[sp])
        assert np.array_equal(o.jac_sp(V[i], F[i], K[i])[mine], full.jac_sp(g["var_in"][c], g["fix"][c], Kz[i])[theirs])
        if name == "demo_a":
            got, want = o.integrate(V[i], F[i], K[i]), full.integrate(g["var_in"][c], g["fix"][c], Kz[i])
            assert got[1] == want[1] == 1 and np.array_equal(got[2], want[2])
            assert np.array_equal(got[0], want[0][sp]) and got[3] == want[3] and got[4] == want[4]
            # ... and the zeroed constants do not change how the captured cell runs: the counters are the full mechanism's
            assert np.array_equal(want[2], full.integrate(g["var_in"][c], g["fix"][c], g["rconst"][c])[2])


@pytest.mark.parametrize("nt", [64, 256])
@pytest.mark.parametrize("name", DEMO_NAMES)
def test_schedule_emulator_on_the_demo_tables(emu, name, nt, demo_oracles):      # noqa: F811
    """tests/test_schedule.py::test_programs_match_oracle, its checks as they stand, on the demo tables at both size classes' workgroup sizes"""
    V, F, K = uc.cut_inputs(name, load_golden(uc.DEMOS[name][0]), uc.CELLS)
    programs_match_oracle(emu, name, nt, {name: {"var_in": V, "fix": F, "rconst": K}}, demo_oracles)


def _patched_header(name, nvar, path):
    raw = bytearray(_raw(name))
    raw[8:12] = struct.pack("<i", nvar)
    with open(path, "wb") as f:
        f.write(raw)
    return str(path)


def test_generated_traits_and_the_size_class_rule(emu, tmp_path):      # noqa: F811
    import re
    from mistra_amd import build as B
    from mistra_amd import mechtab
    gen = B.build_traits_gen()
    for slot, name in enumerate(DEMO_NAMES):
        t = mechtab.load(name)
        tr = B.user_traits(os.path.join(MECH_DIR, name + ".mech"), slot, str(tmp_path / ("t%d.hpp" % slot)), gen)
        njnz = int(np.sum(np.diff(t.jv_ptr) > 0))
        assert (tr["NVAR"], tr["NFIX"], tr["NREACT"], tr["NNZ"], tr["NB"], tr["NCONST"], tr["NJNZ"]) == (t.nvar, t.nfix, t.nreact, t.nnz, t.nb, t.nconst, njnz)
        assert tr["NAME"] == name and tr["DENSE_ND"] == 0 and tr["DENSE_KB"] == 0
        # the size class follows from NVAR alone
        nt = 64 if t.nvar <= 128 else 256
        assert tr["NT"] == nt and tr["RING_LOW"] == (nt == 64) and tr["WAVES_PER_SIMD"] == ("MISTRA_GAS_WPS" if nt == 64 else "MISTRA_AER_WPS")
        # what the schedule compiler reports at that workgroup size (the emulator runs the same compiler)
        h = emu.emu_create(os.path.join(MECH_DIR, name + ".mech").encode(), nt)
        text = emu.emu_describe(h).decode()
        assert emu.emu_tail_h(h) == t.nvar - 64 * tr["TAIL_REGS"]
        temps = int(re.search(r"(\d+) partial-sum cells", text).group(1))
        assert tr["Temps"] == temps and tr["MAX_TEMPS"] == (temps + 2 + 1) // 2 * 2
        assert emu.emu_dense_nd(h) == 0
        # the cell's LDS block: inside a CU, and twice where the rate constants went into it
        assert tr["LdsTotal"] * 8 <= 160 * 1024 and (not tr["RCT_LDS"] or (nt == 256 and tr["LdsTotal"] * 8 * 2 <= 160 * 1024))
        if os.path.exists(os.path.join(B.OBJDIR, "user_traits_%d.hpp" % slot)) and B.user_mech_tables() == B.USER_DEFAULT:
            assert open(os.path.join(B.OBJDIR, "user_traits_%d.hpp" % slot)).read() == open(tmp_path / ("t%d.hpp" % slot)).read()
    assert tr["SCALE_PASS"] is True and tr["TAIL_REGS"] == 2 and tr["RCT_LDS"] is True      # demo_a runs like aer
    for nvar, text in ((513, "NVAR = 513: no size class"), (63, "NVAR = 63: no size class")):
        with pytest.raises(RuntimeError, match=text):
            B.user_traits(_patched_header("demo_a", nvar, tmp_path / "crafted.mech"), 1, str(tmp_path / "crafted.hpp"), gen)
    with pytest.raises(RuntimeError, match="is taken"):
        B.user_traits(os.path.join(MECH_DIR, "gas.mech"), 0, str(tmp_path / "gas.hpp"), gen)


def test_c_abi_without_a_device():
    from mistra_amd import chem
    from mistra_amd.build import build_lib
    build_lib()
    L = chem.lib()
    assert L.mistra_chem_user_mechs() == 2 and chem.user_mechs() == list(DEMO_NAMES)
    for i, name in enumerate(DEMO_NAMES):
        mid = 3 + i
        assert L.mistra_chem_mech_name(mid) == name.encode()
        v = [C.c_int32() for _ in range(4)]
        assert L.mistra_chem_dims(mid, *[C.byref(x) for x in v]) == 0
        from mistra_amd import mechtab
        t = mechtab.load(name)
        assert tuple(x.value for x in v) == (t.nvar, t.nfix, t.nreact, t.nnz) == chem.DIMS[name]
        assert chem._mech_id("user%d" % i) == chem._mech_id(name) == chem._mech_id(mid) == (mid, name)
        # Rosenbrock_x's decode needs no device
        r = chem.check_options(name, rtol=1.0e-5)
        assert r.ierr == 1 and r.hstart == 1.0e-3 and r.max_steps == 100000
        assert chem.check_options("user%d" % i, rpar=[-1.0]).ierr == -3
        assert chem.check_options(mid, atol=np.zeros(t.nvar), ipar=[0, 0, 0, 2]).ierr == -5
        with pytest.raises(chem.MistraChemError, match="Ros3"):
            chem.check_options(name, ipar=[0, 1, 0, 4])
        assert chem.get_options(name) is None
        # one entry of every family a user slot does not have: the slot's text, whatever the other arguments, and without a device
        slot_text = ("user mechanism slot %d \\(%s\\) has no " % (i, name))
        ipar, rpar, tol = np.zeros(20, np.int32), np.zeros(20), np.ones(t.nvar) * 1e-3
        ipar[3] = 4
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        P = lambda a: a.ctypes.data_as(ip if a.dtype == np.int32 else dp)
        calls = {
            "rates": lambda: L.mistra_chem_update_rconst(mid, 1, None, None),
            "pack": lambda: L.mistra_chem_pack_device(mid, 0, None, None, None, None, None, None, None, None),
            "drive": lambda: L.mistra_chem_drive_end(mid),
            "liq_parm": lambda: L.mistra_chem_henry_device(mid, 1, None, None, None),
            "integrate_common": lambda: L.mistra_chem_integrate_common(mid, None, None, None),
            "step reuse": lambda: L.mistra_chem_set_step_reuse(mid, 1),
            "trace": lambda: L.mistra_chem_rosenbrock_trace_ex(mid, 1, None, None, None, 0.0, 10.0, P(tol), P(tol), P(rpar), P(ipar), None, None, None, None, 0, None, None,
                                                               None, None),
            "other methods": lambda: L.mistra_chem_rosenbrock_ex(mid, 1, None, None, None, 0.0, 10.0, P(tol), P(tol), P(rpar), P(ipar), None, None, None, None),
            "env": lambda: L.mistra_chem_integrate_env_ex(mid, 1, None, None, None, 0.0, 10.0, None, None, None, None),
        }
        import re
        for family, call in calls.items():
            assert call() != 0, family
            assert re.search(slot_text, L.mistra_chem_last_error().decode()), (family, L.mistra_chem_last_error())
        assert L.mistra_chem_get_step_reuse(mid) == 0
    assert L.mistra_chem_mech_name(5) is None and L.mistra_chem_dims(5, None, None, None, None) != 0
    assert b"unknown mechanism" in L.mistra_chem_last_error()
    assert L.mistra_chem_set_step_reuse(5, 1) != 0 and b"unknown mechanism" in L.mistra_chem_last_error()
    with pytest.raises(chem.MistraChemError, match="unknown mechanism"):
        chem._mech_id(5)
    with pytest.raises(chem.MistraChemError, match="unknown mechanism"):
        chem._mech_id("demo_x")


@pytest.mark.parametrize("run", ub.RUNS)
@pytest.mark.parametrize("name", DEMO_NAMES)
def test_bounds_of_the_gpu_tests_follow_the_oracles_own_spread(name, run):
    """Every constant of tests/user_mech_bounds.py is 10x .. 100x what the oracle's variants 1, 2 and 4 move by on the test cells (or the floor), and no
    variant changes IERR or a counter there (measure asserts it)."""
    import parity_bounds as pb
    s_var, s_th = ub.measure(name, run)
    print("%s %s: oracle's spread VAR %.3e, exit time / step size %.3e" % (name, run, s_var, s_th))
    pb.check_constant("VAR_RTOL[%s, %s]" % (name, run), ub.VAR_RTOL[(name, run)], s_var, floor=pb.PARITY_FLOOR)
    if run != "hstart":
        pb.check_constant("TH_RTOL[%s, %s]" % (name, run), ub.TH_RTOL[(name, run)], s_th, floor=pb.PARITY_FLOOR)
    ierr = ub.oracle_run(name, run)[1]
    assert (ierr == 1).all()
