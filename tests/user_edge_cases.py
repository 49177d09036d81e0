"""The tables at the edges of the user slots' size classes: the rule they are cut by, their pinned sizes, digests and traits, and the
captured cells cut to them.  The rule itself lives in mistra_amd/mechderive.py (EDGE_TABLES, derive_edge, ensure_edge_tables), which the build calls too
(mistra_amd/build.py: build_edge_twins):

  edge_g64    fewest_reactions_rule(gas, 37), species removed   NVAR 64:  H = NVAR - 64 = 0, no head rows, the tail chain is the whole solve
  edge_a128   fewest_reactions_rule(aer, 129), species removed  NVAR 128: the largest one-wave table, and a one-wave table WITH the scaling pass
  edge_a129   fewest_reactions_rule(aer, 128), species removed  NVAR 129: the smallest four-wave table, the upper two waves own at most one species
  edge_t417   tot's own bytes under another name                NVAR 417: the largest table there is, at 256 threads without the dense tail block

Nothing of them is committed: tables, maps and copies of gas.mech, aer.mech and tot.mech are written into mistra_amd/build/edge_mech/ (ignored by git),
which then serves as a mechanism directory.  tests/test_user_edges.py holds the derivation and the files on disk to the digests pinned here.
"""
import os

import numpy as np

from conftest import REPO

EDGES = {"edge_g64": ("gas", 37), "edge_a128": ("aer", 129), "edge_a129": ("aer", 128), "edge_t417": ("tot", None)}      # name: (source, species of the rule)
NAMES = tuple(EDGES)
EDGE_DIR = os.path.join(REPO, "mistra_amd", "build", "edge_mech")
TWINS = {"edge0": ("edge_g64", "edge_a129"), "edge1": ("edge_a128", "edge_t417")}      # the twin libraries and the tables in their slots 0 and 1

SIZES = {"edge_g64": (64, 3, 258, 839), "edge_a128": (128, 5, 546, 4172), "edge_a129": (129, 5, 552, 4211), "edge_t417": (417, 7, 1627, 13503)}   # NVAR NFIX NREACT NNZ
# what user_traits_gen derives from them
TRAITS = {"edge_g64": dict(NT=64, TAIL_REGS=1, MAX_TEMPS=2, SCALE_PASS=False, RCT_LDS=False, LdsTotal=1530),
          "edge_a128": dict(NT=64, TAIL_REGS=1, MAX_TEMPS=190, SCALE_PASS=True, RCT_LDS=False, LdsTotal=5342),
          "edge_a129": dict(NT=256, TAIL_REGS=1, MAX_TEMPS=194, SCALE_PASS=False, RCT_LDS=True, LdsTotal=6006),
          "edge_t417": dict(NT=256, TAIL_REGS=2, MAX_TEMPS=618, SCALE_PASS=True, RCT_LDS=False, LdsTotal=17112)}
# SHA-256 of the tables and their maps, taken when they were first derived and their sizes and traits checked against the figures above
SHA256 = {
    "edge_g64.mech": "2d04c4f011ea5f07ce13864ae5da1360275750915356e0fee06a81f4cf179e8c",
    "edge_g64.json": "132b164c8cd4753982fd7d71c2cac5402100f7a87576e069bb9a1fd02e3258e8",
    "edge_a128.mech": "1716da44ac76eccbfa2edfa52f2c05c1dbd8e26dcc9733159badd759d47b9c04",
    "edge_a128.json": "0abc0c8f499ae4e14863322b9b47bac5cdeb245f235e6f139ee59ea975b58751",
    "edge_a129.mech": "516d342ef323bc2558a1127c95e4c8f83c6826df53db59f1cef01e1d70fe248e",
    "edge_a129.json": "47b8b456a6be2f57ae520ee99d208c8c85eabd5b1e23201f5d7730aa7ee57c0b",
    "edge_t417.mech": "52511ca6a952b2bb520776b1745a6b97dc52d31dda0c6d98403a5414843e4427",      # (tot.mech's)
    "edge_t417.json": "352770c554fb0bf228773906ad29a32c3f3d3579b398a78578438003bdd4661d",
}

CELLS = (0, 16, 31)      # of tests/golden/integrate_<source>.npz, for every table and run: the oracle leaves them with IERR = 1, and none of its variants
#                          1, 2 and 4 moves a counter on them (tests/test_user_edges.py asserts it)


def ensure_tables():
    """The edge directory exists and holds what the rule derives (ignored files only are written)"""
    from mistra_amd import mechderive
    assert mechderive.EDGE_TABLES == EDGES and os.path.realpath(mechderive.EDGE_DIR) == os.path.realpath(EDGE_DIR), \
        "the package and the tests state different rules"
    mechderive.ensure_edge_tables()


def path(name, ext=".mech"):
    return os.path.join(EDGE_DIR, name + ext)


def stem(name):
    """The table's path without its extension.  Handed as the mechanism's NAME to the helpers that look a table up as <mechanism directory>/<name>.mech
    (tests/test_schedule.py, mistra_amd.mechtab.load): an absolute path survives the join, so they read the edge directory as they stand."""
    return os.path.join(EDGE_DIR, name)


def tables(name):
    from mistra_amd import mechtab
    return mechtab.load(stem(name))


def oracle(name):
    from oracle.oracle import Oracle
    return Oracle(stem(name))


def maps(name):
    from mistra_amd import mechderive
    return mechderive.load_maps(name, EDGE_DIR)


def cut_inputs(name, g, cells=CELLS):
    """The captured cells of the SOURCE mechanism's golden set `g`, cut to the table through its .json maps -> (VAR, FIX, RCONST); edge_t417's maps
    are the identity: tot's cells as they are"""
    m = maps(name)
    c = list(cells)
    sp, rx = np.array(m["kept_species"]), np.array(m["kept_reactions"])
    return (np.ascontiguousarray(g["var_in"][c][:, sp]), np.ascontiguousarray(g["fix"][c]), np.ascontiguousarray(g["rconst"][c][:, rx]))


def batch(name, g, n):
    """n cells for a launch: CELLS repeated in turn"""
    V, F, K = cut_inputs(name, g)
    idx = [i % len(CELLS) for i in range(n)]
    return np.ascontiguousarray(V[idx]), np.ascontiguousarray(F[idx]), np.ascontiguousarray(K[idx])
