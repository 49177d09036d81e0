"""The two demo mechanisms of the user slots (mistra_amd/mech/demo_g.mech, demo_a.mech): the rule they are cut by, and the captured cells cut to them.

One rule for both (mistra_amd/mechderive.py: fewest_reactions_rule):
  * take the 16 variable species that take part in the fewest reactions, as a factor of the rate product or as a term of their Vdot sum; ties go to
    the lower index; species that take part in no reaction are skipped;
  * drop every reaction any of the 16 takes part in.
demo_g: cut from gas, the species left without a reaction REMOVED  -> NVAR 86, NREACT 311 (20 of 331 reactions dropped, 16 species removed)
demo_a: cut from aer, the species KEPT                             -> NVAR 257, NREACT 953 (26 of 979 dropped, 16 rows left as a bare diagonal)

The tables are binary, so only their index maps (demo_g.json, demo_a.json) are committed; SHA256 below pins all four files.  mistra_amd/mechderive.py
holds the same rule (DEMO_TABLES, ensure_demo_tables) and writes the two .mech files beside gas.mech and aer.mech where they are missing or stale —
the build does that before it compiles the slots, and ensure_tables() here does it for a test that runs without a build.  Neither writes a committed
file.  tests/test_user_mech.py holds the derivation, the files on disk and the committed maps to the pinned digests: a changed derivation, a changed
source table or a stale map fails there instead of healing itself.
"""
import os

import numpy as np

NSPECIES = 16
DEMOS = {"demo_g": ("gas", True), "demo_a": ("aer", False)}      # name: (source, remove the species left without a reaction)
SIZES = {"demo_g": (86, 3, 311), "demo_a": (257, 5, 953)}        # NVAR, NFIX, NREACT

# SHA-256 of the four files, taken when the tables were first derived and their sizes, drop counts and LU patterns checked against the issue's figures
SHA256 = {
    "demo_g.mech": "eca69b6001ae9fc4fbef3cc5951f40c7d0361f911071b9a1226fef550bb81a1f",
    "demo_g.json": "6fadf492281f4b0f88a152402cc6c01b64700b37102cb946e73e36e827540d18",
    "demo_a.mech": "d4e1ce707cb193858cc351a85ff9ebe075deb86fe3cf48be11dd2107cfead83f",
    "demo_a.json": "72107513ad4cf287ff7e114e7bb95c1d9185c07514a0f173d23c6452faf1a162",
}
NNZ = {"demo_g": 1043, "demo_a": 6539}      # LU_NONZERO of the derived patterns (gas 1110, aer 6579)


def ensure_tables():
    """The two .mech files exist and are what the rule derives (untracked files only are written)."""
    from mistra_amd import mechderive
    assert mechderive.DEMO_TABLES == DEMOS and mechderive.DEMO_SPECIES == NSPECIES, "the package and the tests state different rules"
    mechderive.ensure_demo_tables()


CELLS = (0, 16, 31)      # of tests/golden/integrate_<source>.npz: the oracle leaves them with IERR = 1 and the full run's counters when the dropped
#                          rate constants are zero


def derive_demo(name):
    """-> (tables dict, maps dict, species of the rule, dropped reactions), regenerated from the source table"""
    from mistra_amd import mechderive, mechtab
    source, remove = DEMOS[name]
    t = mechtab.load(source)
    species, drop = mechderive.fewest_reactions_rule(t, NSPECIES)
    tab, maps = mechderive.derive(t, drop, remove)
    return tab, maps, species, drop


def cut_inputs(name, g, cells=None):
    """The captured cells of the SOURCE mechanism's golden set `g`, cut to the demo table through its .json maps -> (VAR, FIX, RCONST)"""
    from mistra_amd import mechderive
    maps = mechderive.load_maps(name)
    c = list(range(g["var_in"].shape[0])) if cells is None else list(cells)
    sp, rx = np.array(maps["kept_species"]), np.array(maps["kept_reactions"])
    return (np.ascontiguousarray(g["var_in"][c][:, sp]), np.ascontiguousarray(g["fix"][c]), np.ascontiguousarray(g["rconst"][c][:, rx]))


def zeroed_rates(name, g, cells):
    """RCONST of the source mechanism with the dropped reactions' rate constants set to 0"""
    from mistra_amd import mechderive
    maps = mechderive.load_maps(name)
    k = np.zeros_like(g["rconst"][list(cells)])
    rx = np.array(maps["kept_reactions"])
    k[:, rx] = g["rconst"][list(cells)][:, rx]
    return k


def batch(name, g, n):
    """n cells for a launch: CELLS repeated in turn"""
    V, F, K = cut_inputs(name, g, CELLS)
    idx = [i % len(CELLS) for i in range(n)]
    return np.ascontiguousarray(V[idx]), np.ascontiguousarray(F[idx]), np.ascontiguousarray(K[idx])
