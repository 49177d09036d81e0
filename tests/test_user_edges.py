"""The tables at the edges of the user slots' size classes without a GPU (tests/user_edge_cases.py): the rule and its pinned digests, the traits the
generator derives, the schedule emulator against the oracle at each table's workgroup size, and the bounds the GPU tests
(tests/test_gpu_user_edges.py) use."""
import hashlib
import os
import re

import numpy as np
import pytest

import user_edge_bounds as eb
import user_edge_cases as ec
from conftest import load_golden
from test_schedule import emu, test_programs_match_oracle as programs_match_oracle      # noqa: F401  (the fixture and the checks of the shipped tables)


@pytest.fixture(scope="module", autouse=True)
def edge_tables():
    ec.ensure_tables()


def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


@pytest.mark.parametrize("name", ec.NAMES)
def test_edge_tables_regenerate_from_their_rule(name):
    """The derivation and the files in the edge directory against the pinned digests and sizes; the species the rule names are gone, and the directory
    serves as a mechanism directory (gas, aer and tot lie beside the tables, byte for byte)."""
    from mistra_amd import mechderive, mechtab
    source, nspecies = ec.EDGES[name]
    tab, maps = mechderive.derive_edge(name)
    assert _sha(mechderive.table_bytes(tab)) == ec.SHA256[name + ".mech"], "the derivation of %s no longer gives the pinned table" % name
    assert _sha(mechderive.maps_text(maps).encode()) == ec.SHA256[name + ".json"]
    for ext in (".mech", ".json"):
        with open(ec.path(name, ext), "rb") as f:
            assert _sha(f.read()) == ec.SHA256[name + ext], "%s is not the pinned file" % ec.path(name, ext)
    t, src = ec.tables(name), mechtab.load(source)
    assert (t.nvar, t.nfix, t.nreact, t.nnz) == ec.SIZES[name] and maps["source"] == source
    for mech in ("gas", "aer", "tot"):
        with open(ec.path(mech), "rb") as f, open(os.path.join(mechtab.MECH_DIR, mech + ".mech"), "rb") as g:
            assert f.read() == g.read()
    if nspecies is None:      # tot's bytes under another name, identity maps
        with open(os.path.join(mechtab.MECH_DIR, source + ".mech"), "rb") as f:
            assert _sha(f.read()) == ec.SHA256[name + ".mech"]
        assert maps["kept_species"] == list(range(src.nvar)) and maps["kept_reactions"] == list(range(src.nreact))
    else:
        species, drop = mechderive.fewest_reactions_rule(src, nspecies)
        part = mechderive.species_reactions(src)
        left = [s for s in range(src.nvar) if not (part[s] - set(drop))]      # (those the rule names, and whatever had no reaction before or loses its last one)
        assert len(species) == nspecies and set(species) <= set(left)
        assert sorted(set(range(src.nvar)) - set(maps["kept_species"])) == left and t.nvar == src.nvar - len(left)
        assert t.nreact == src.nreact - len(drop)
        assert t.a_fac.max() < t.nvar + t.nfix + t.nconst and t.b_fac.max() < t.nvar + t.nfix + t.nconst
    for k in range(t.nvar):      # the LU pattern: columns ascending, the diagonal in every row
        row = t.icol[t.crow[k]:t.crow[k + 1]]
        assert np.all(np.diff(row) > 0) and t.icol[t.diag[k]] == k
    assert re.fullmatch(r"\w+", name) and name not in ("gas", "aer", "tot", "user0", "user1")      # a legal slot name


def test_generated_traits_at_the_size_classes_edges(emu, tmp_path):      # noqa: F811
    """The traits of the issue's table, Temps and MAX_TEMPS as tests/test_user_mech.py::test_generated_traits_and_the_size_class_rule relates them,
    emu_tail_h == NVAR - 64 * TAIL_REGS (0 for edge_g64: no head rows) and the cell's LDS block inside a CU.  A one-wave table WITH the scaling pass
    (edge_a128) is accepted: scale_run's low placement works through the ring two slots at a time and stays below the ring's registers."""
    from mistra_amd import build as B
    gen = B.build_traits_gen()
    for twin, names in ec.TWINS.items():
        for slot, name in enumerate(names):
            t, want = ec.tables(name), ec.TRAITS[name]
            tr = B.user_traits(ec.path(name), slot, str(tmp_path / ("%s_%d.hpp" % (twin, slot))), gen)
            njnz = int(np.sum(np.diff(t.jv_ptr) > 0))
            assert (tr["NVAR"], tr["NFIX"], tr["NREACT"], tr["NNZ"], tr["NB"], tr["NCONST"], tr["NJNZ"]) == (t.nvar, t.nfix, t.nreact, t.nnz, t.nb, t.nconst, njnz)
            assert tr["NAME"] == name and tr["DENSE_ND"] == 0 and tr["DENSE_KB"] == 0
            for k, v in want.items():
                assert tr[k] == v, (name, k, tr[k], v)
            nt = 64 if t.nvar <= 128 else 256
            assert tr["NT"] == nt and tr["RING_LOW"] == (nt == 64) and tr["WAVES_PER_SIMD"] == ("MISTRA_GAS_WPS" if nt == 64 else "MISTRA_AER_WPS")
            h = emu.emu_create(ec.path(name).encode(), nt)
            assert h, "schedule compiler failed"
            assert emu.emu_tail_h(h) == t.nvar - 64 * tr["TAIL_REGS"]
            temps = int(re.search(r"(\d+) partial-sum cells", emu.emu_describe(h).decode()).group(1))
            assert tr["Temps"] == temps and tr["MAX_TEMPS"] == (temps + 2 + 1) // 2 * 2
            assert emu.emu_dense_nd(h) == 0
            assert tr["LdsTotal"] * 8 <= 160 * 1024 and (not tr["RCT_LDS"] or (nt == 256 and tr["LdsTotal"] * 8 * 2 <= 160 * 1024))
            built = os.path.join(B.edge_twin_dir(twin), "user_traits_%d.hpp" % slot)
            if os.path.exists(built):      # what the twin was built from
                assert open(built).read() == open(tmp_path / ("%s_%d.hpp" % (twin, slot))).read()
    # edge_g64 has no head rows.  Its head sweeps are programs without an update, and such a program is ONE round of null rows, never none: the
    # kernel's executor counts rounds down at each round's end and has no test at entry (with none it ran off the end of its table on the GPU)
    h = emu.emu_create(ec.path("edge_g64").encode(), 64)
    assert emu.emu_tail_h(h) == 0
    assert "head fwd 1 rounds / 1 rows critical, head bwd 1 rounds / 1 rows critical, 0 partial-sum cells" in emu.emu_describe(h).decode()


@pytest.mark.parametrize("name", ec.NAMES)
def test_schedule_emulator_on_the_edge_tables(emu, name):      # noqa: F811
    """tests/test_schedule.py::test_programs_match_oracle, its checks as they stand, on each edge table at its size class's workgroup size (the table's
    path without extension stands in for the mechanism's name: user_edge_cases.stem)"""
    V, F, K = ec.cut_inputs(name, load_golden(ec.EDGES[name][0]))
    key = ec.stem(name)
    programs_match_oracle(emu, key, ec.TRAITS[name]["NT"], {key: {"var_in": V, "fix": F, "rconst": K}}, {key: ec.oracle(name)})


@pytest.mark.parametrize("run", eb.RUNS)
@pytest.mark.parametrize("name", ec.NAMES)
def test_bounds_of_the_gpu_tests_follow_the_oracles_own_spread(name, run):
    """Every constant of tests/user_edge_bounds.py is 10x .. 100x what the oracle's variants 1, 2 and 4 move by on the test cells (or the floor), and no
    variant changes IERR or a counter there (measure asserts it)."""
    import parity_bounds as pb
    s_var, s_th = eb.measure(name, run)
    print("%s %s: oracle's spread VAR %.3e, exit time / step size %.3e" % (name, run, s_var, s_th))
    pb.check_constant("VAR_RTOL[%s, %s]" % (name, run), eb.VAR_RTOL[(name, run)], s_var, floor=pb.PARITY_FLOOR)
    pb.check_constant("TH_RTOL[%s, %s]" % (name, run), eb.TH_RTOL[(name, run)], s_th, floor=pb.PARITY_FLOOR)
    ierr = eb.oracle_run(name, run)[1]
    assert (ierr == 1).all()
