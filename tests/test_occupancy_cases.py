"""tests/occupancy_cases.py without a GPU: the interleaving, the fill counts, that the conditions the filled launches are held to are ones the compiled
reference's records meet, and that the GPU module walks exactly the kernels the launch table holds."""
import os

import numpy as np
import pytest

import occupancy_cases as OC
import ros_methods_py as RM
from mistra_amd import build as B


def test_copy_i_is_cell_i_mod_3():
    """no two neighbours are the same cell, every cell fills a third of the batch, and fill() / fill_legs() put the rows where pattern() says"""
    for mech in OC.MECHS:
        n = OC.FILL[mech]
        p = OC.pattern(n)
        assert p.tolist() == [i % 3 for i in range(n)] and (p[1:] != p[:-1]).all()
        assert [abs(int((p == c).sum()) - n / 3) < 1 for c in range(3)] == [True] * 3
    rows = np.arange(3 * 4, dtype=np.float64).reshape(3, 4)
    got = OC.fill(rows, 8)
    assert got.flags.c_contiguous and got.tolist() == [rows[i % 3].tolist() for i in range(8)]
    legs = np.stack([rows, rows + 100.0])
    got = OC.fill_legs(legs, 7)
    assert got.flags.c_contiguous and got.shape == (2, 7, 4) and all(got[k, i].tolist() == legs[k, i % 3].tolist() for k in range(2) for i in range(7))


def test_fill_is_twice_the_resident_capacity_of_an_mi355x():
    assert OC.FILL == {m: 2 * OC.PER_CU[m] * OC.MI355X_CUS for m in OC.MECHS}
    # the figures PER_CU is taken from (mistra_amd/csrc/ros3_kernel.hpp)
    hpp = open(os.path.join(OC.CSRC, "ros3_kernel.hpp")).read()
    for text in ("#define MISTRA_GAS_NT 64", "#define MISTRA_AER_NT 256", "#define MISTRA_TOT_NT 512", "#define MISTRA_GAS_WPS 3", "#define MISTRA_AER_WPS 2",
                 "#define MISTRA_TOT_WPS 2", "LDS (16.0 KB per cell) admits 10 one-wave cells per CU"):
        assert text in hpp, text
    simds, waves = 4, {"aer": (256 // 64, 2), "tot": (512 // 64, 2)}
    assert OC.PER_CU == {"gas": 10, **{m: simds * wps // per_cell for m, (per_cell, wps) in waves.items()}}


@pytest.mark.parametrize("mech", OC.MECHS)
def test_the_reference_ends_every_cell_with_ierr_1(mech):
    """m1 .. m5 on the three cells: IERR 1 in the compiled reference's record (Ros3: the captured INTEGRATE_x calls, which have statistics and no IERR —
    every one of them made its steps), so "every copy ends with IERR 1" asks nothing the reference does not do"""
    V, F, K = OC.cells(mech)
    assert V.shape == (3, RM.NVAR[mech]) and F.shape[0] == K.shape[0] == 3
    for m in OC.METHODS:
        ierr, stats = OC.reference_record(mech, m)
        assert stats.shape == (3, 8) and (stats[:, 3] >= 1).all() and (stats[:, 2] >= stats[:, 3]).all(), (m, stats)
        if m == OC.ROS3:
            assert ierr is None
        else:
            assert ierr.tolist() == [1, 1, 1], (m, ierr)


def test_the_cells_retire_at_different_times():
    """accepted steps (IPAR(14)) of the three cells under Ros3: not all equal for aer and tot.  gas cannot be helped: EVERY cell of integrate_gas.npz makes
    the same number of steps, so there is none to put in another's place; its copies differ in step count under Ros2 alone (occupancy_cases: docstring)"""
    nacc = {mech: {m: OC.reference_record(mech, m)[1][:, 3].tolist() for m in OC.METHODS} for mech in OC.MECHS}
    for mech in ("aer", "tot"):
        for m in OC.METHODS:
            assert len(set(nacc[mech][m])) > 1, (mech, m, nacc[mech][m])
    every = np.load(os.path.join(OC.GOLDEN, "integrate_gas.npz"))["stats"][:, 3]
    assert len(set(nacc["gas"][OC.ROS3])) == 1 and len(set(every.tolist())) == 1, "gas has cells that differ in steps now: put the one with the most in (occupancy_cases.cells)"
    assert len(set(nacc["gas"][1])) > 1


def test_the_walk_is_the_launch_table():
    """the (VARIANT, method) pairs the GPU module is parametrised over are the non-null slots of capi.cpp's table — read off its description and,
    independently, off build.py's units and what ros_unit_kernel.hip instantiates in each — plus the product unit's options kernel of Ros3; no pair
    twice.  A kernel added to the table without an entry in occupancy_cases.ENTRIES fails here."""
    table = OC.table_slots()
    assert len(table) == len(set(table)) == 32
    for mech in (0, 1, 2):
        assert OC.unit_slots(mech) == table, mech
    assert {v for v, _ in table} == set(range(3, 12)) and OC.PRODUCT_SLOT not in table
    assert {u.variant for u in B.VARIANT_UNITS} < {v for v, _ in table}
    assert OC.walk_pairs() == sorted(table + [OC.PRODUCT_SLOT])
    ids = [OC.walk_id(mech, *w) for mech in OC.MECHS for w in OC.WALK]
    assert len(set(ids)) == len(ids) == 3 * 33
