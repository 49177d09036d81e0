"""TEST INFRASTRUCTURE — the cases of tests/test_gpu_occupancy.py: every integrator kernel on a FULL device, copies of known cells side by side, each copy
held to the same entry's answer for its cell launched alone, byte for byte.

Cells.  Per mechanism the three cells ros_methods_py.cells_of names (0, n/2, n-1 of tests/golden/integrate_<mech>.npz), the ones whose results the compiled
reference left in tests/golden/ros_methods_<mech>.npz (Ros2, Ros4, Rodas3, Rodas4; Ros3 at these options is INTEGRATE_x itself, and its record is the
`stats` of integrate_<mech>.npz).  Copy i of a filled batch is cell i % 3: neighbours in the grid are never the same cell, so workgroups that share a CU,
or follow each other onto one, are at different steps — where the cells take different numbers of steps.  aer and tot do (Ros3: 81 / 53 / 98 and
130 / 95 / 115 accepted steps).  gas does NOT under Ros3, Ros4, Rodas3 and Rodas4: all 32 cells of integrate_gas.npz make 7 accepted steps, so there is no
cell "with the most steps" to put in another's place (what tests/test_gpu_dense_finish.py does for tot) and the three cells stay as they are; only
Ros2 separates them (8 / 7 / 7).  gas copies therefore retire nearly in lockstep; what the fill still gives gas is ten workgroups per CU, nine of them
at an LDS base above 0, and a second round of workgroups starting while the first is running.

Fill counts.  FILL is twice the device's resident capacity, PER_CU cells per CU on the 256 CUs of an MI355X, so that a second round of workgroups is
dispatched onto CUs whose neighbours are in mid-step.  PER_CU from mistra_amd/csrc/ros3_kernel.hpp:
    gas 10   one wave per cell (MISTRA_GAS_NT 64); MISTRA_GAS_WPS: "LDS (16.0 KB per cell) admits 10 one-wave cells per CU" of the 160 KiB
    aer  2   MISTRA_AER_NT 256 = four waves per cell at MISTRA_AER_WPS 2 waves per SIMD: 8 wave slots on the CU's 4 SIMDs, "still two cells per CU"
    tot  1   MISTRA_TOT_NT 512 = eight waves per cell at MISTRA_TOT_WPS 2: the 8 wave slots are one cell's
The GPU module reads the CU count off the device and fails where FILL is less than twice its capacity.

The walk.  ENTRIES names, per entry of the library, the kernel VARIANT it launches (capi.cpp: launch) and the methods it is run with; WALK lists the
(entry, VARIANT, method) triples the GPU module is parametrised over.  tests/test_occupancy_cases.py holds the pairs to the launch table's non-null
slots, which table_slots() reads off capi.cpp's description of the table and unit_slots() off build.py's VARIANT_UNITS and the kernels each unit of
ros_unit_kernel.hip holds — plus PRODUCT_SLOT, the options kernel of Ros3, which the table leaves to the product unit."""
import os
import re

import numpy as np

import ros_methods_py as RM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CSRC = os.path.join(REPO, "mistra_amd", "csrc")
MECHS = RM.MECHS
MECH_ID = {"gas": 0, "aer": 1, "tot": 2}
METHODS = (1, 2, 3, 4, 5)
ROS3, RODAS4 = 2, 5
NCELL = 3

FILL = {"gas": 5120, "aer": 1024, "tot": 512}
PER_CU = {"gas": 10, "aer": 2, "tot": 1}
MI355X_CUS = 256

# entry -> (kernel VARIANT, the methods it is run with)
ENTRIES = {
    "plain": (3, METHODS),             # rosenbrock(); Ros3: the product unit's options kernel (PRODUCT_SLOT), and rosenbrock_cells beside it
    "trace": (4, (ROS3,)),             # rosenbrock_trace(), cap 256
    "series": (5, METHODS),            # rosenbrock_series(), four legs; Ros3 with carry_h too; Ros3 and Rodas4 also as rosenbrock_series_rates()
    "flux": (6, METHODS),              # rosenbrock_flux()
    "dense": (7, METHODS),             # rosenbrock_dense(), ros_dense_py.LINEAR8
    "ops": (8, (ROS3,)),               # ops(): Fun, Jac_SP, one shifted solve with the fun_rhs row
    "replay": (9, (ROS3,)),            # rosenbrock_replay(): the accepted steps of cell 0's trace, shared and as rows per cell
    "linrates": (10, METHODS),         # rosenbrock_series_linrates(), the night/day node blocks
    "series_flux": (11, METHODS),      # rosenbrock_series_flux()
}
WALK = [(entry, variant, method) for entry, (variant, methods) in ENTRIES.items() for method in methods]
PRODUCT_SLOT = (3, ROS3)


def walk_pairs():
    """the (VARIANT, method) pairs of WALK, as a sorted list (a pair walked twice shows twice)"""
    return sorted((v, m) for _, v, m in WALK)


def walk_id(mech, entry, variant, method):
    return "%s-v%d-%s-%s" % (mech, variant, entry, RM.METHOD_NAMES[method])


def table_slots():
    """The non-null slots of the launch table as capi.cpp describes it: the VARIANTs unit_table() adds, the methods of its integer sequence, and
    add_unit()'s condition evaluated for each pair -> sorted [(VARIANT, method)]"""
    src = open(os.path.join(CSRC, "capi.cpp")).read()
    body = src[src.index("constexpr UnitTable unit_table("):]
    body = body[:body.index("return t;")]
    variants = sorted({int(v) for v in re.findall(r"add_unit<MT, NT, (\d+), METHOD \+ 1>", body)})
    nmeth = int(re.search(r"unit_table<MT, NT>\(std::make_integer_sequence<int, (\d+)>", src).group(1))
    cond = re.search(r"constexpr void add_unit\(UnitTable& t\) \{\s*if constexpr \((.*)\) t\.fn\[VARIANT\]\[METHOD\] = ", src).group(1)
    kros3 = int(re.search(r"kRos3 = (\d+)", open(os.path.join(CSRC, "ros_methods.hpp")).read()).group(1))
    expr = cond.replace("||", " or ").replace("&&", " and ").replace("kRos3", str(kros3))
    assert re.fullmatch(r"[\sA-Za-z0-9()!=]*", expr), expr
    return sorted((v, m) for v in variants for m in range(1, nmeth + 1) if eval(expr, {"__builtins__": {}}, {"VARIANT": v, "METHOD": m}))


def unit_slots(mech=0):
    """The kernels the units of one mechanism hold: build.py's VARIANT_UNITS, and per unit the further VARIANTs that ros_unit_kernel.hip instantiates under
    its `#if MISTRA_UNIT_VARIANT == ..` blocks, each with the unit's method -> sorted [(VARIANT, method)]"""
    from mistra_amd import build as B
    src = open(os.path.join(CSRC, B.UNIT_SOURCE)).read()
    hosted = {}      # VARIANT of the unit -> the VARIANTs it holds besides
    for cond, block in re.findall(r"^#if ((?:MISTRA_UNIT_VARIANT == \d+(?: \|\| )?)+)$(.*?)^#endif", src, re.M | re.S):
        held = [int(v) for v in re.findall(r"launch_ros_unit<UnitMT, kUnitNT, (\d+), MISTRA_UNIT_METHOD>\(const KernelArgs", block)]
        for host in re.findall(r"== (\d+)", cond):
            hosted.setdefault(int(host), []).extend(held)
    units = [u for u in B.VARIANT_UNITS if u.mech == mech]
    return sorted([(u.variant, u.method) for u in units] + [(v, u.method) for u in units for v in hosted.get(u.variant, ())])


def pattern(n):
    """the cell each of n copies holds: copy i is cell i % 3"""
    return np.arange(n) % NCELL


def fill(rows, n):
    """rows [3, ...] (or [k, 3, ...] with axis = 1) -> the n interleaved copies"""
    return np.ascontiguousarray(rows[pattern(n)])


def fill_legs(blocks, n):
    """blocks [k, 3, .] (per leg or per node) -> [k, n, .]"""
    return np.ascontiguousarray(blocks[:, pattern(n)])


def cells(mech):
    """-> (VAR [3, NVAR], FIX [3, NFIX], RCONST [3, NREACT]) of the three cells"""
    g = np.load(os.path.join(GOLDEN, "integrate_%s.npz" % mech))
    c = list(RM.cells_of(g["var_in"].shape[0]))
    return tuple(np.ascontiguousarray(g[k][c]) for k in ("var_in", "fix", "rconst"))


def reference_record(mech, method):
    """(IERR [3] or None, IPAR(11:18) [3, 8]) the compiled reference left for the three cells under method_set(mech, "m<method>"): the record of
    ros_methods_<mech>.npz; Ros3, which that file does not hold, is INTEGRATE_x: the statistics of integrate_<mech>.npz (a captured call has no IERR)"""
    if method == ROS3:
        g = np.load(os.path.join(GOLDEN, "integrate_%s.npz" % mech))
        return None, g["stats"][list(RM.cells_of(g["var_in"].shape[0]))]
    z = np.load(os.path.join(GOLDEN, "ros_methods_%s.npz" % mech))
    assert z["cells"].tolist() == list(RM.cells_of(np.load(os.path.join(GOLDEN, "integrate_%s.npz" % mech))["var_in"].shape[0]))
    return z["m%d_ierr" % method], z["m%d_ipar" % method]


def differing(odd, what, mech, ncopy):
    """the text of a failure: odd = indices of the copies that differ"""
    odd = np.asarray(odd)
    per_cell = [int((odd % NCELL == c).sum()) for c in range(NCELL)]
    return ("%s, %s: %d of %d copies differ from their cell launched alone, first: copy %d, a copy of cell %d (differing copies per cell %s)"
            % (mech, what, len(odd), ncopy, int(odd[0]), int(odd[0]) % NCELL, per_cell))
