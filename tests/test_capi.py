"""The C-ABI library: loads on a machine without a GPU, exports every symbol include/mistra_chem.h declares, and
refuses to compute without a device (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def lib():
    from mistra_amd.build import build_lib
    build_lib()
    from mistra_amd import chem
    return chem.lib()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(REPO, "include", "mistra_chem.h")).read()
    names = set(re.findall(r"\b(mistra_chem_\w+)\s*\(", hdr))
    assert {"mistra_chem_init", "mistra_chem_integrate", "mistra_chem_integrate_device", "mistra_chem_integrate_common",
            "mistra_chem_finalize", "mistra_chem_dims", "mistra_chem_last_error", "mistra_chem_describe"} <= names
    for n in names:
        assert hasattr(lib, n), "symbol %s declared in the header is not exported" % n


def test_dims(lib):
    from mistra_amd.chem import DIMS
    for mech, name in enumerate(("gas", "aer", "tot")):
        v = [C.c_int32() for _ in range(4)]
        assert lib.mistra_chem_dims(mech, *[C.byref(x) for x in v]) == 0
        assert tuple(x.value for x in v) == DIMS[name]
    assert lib.mistra_chem_dims(7, None, None, None, None) != 0


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mistra_amd import chem
    assert lib.mistra_chem_init(0) != 0
    assert b"no HIP device" in lib.mistra_chem_last_error()
    with pytest.raises(chem.MistraChemError):
        chem.integrate("gas", np.zeros((1, 102)), np.zeros((1, 3)), np.zeros((1, 331)))
    # (the Fortran-facing entry points bring the library up themselves; without a device that fails loudly too)
    rc = lib.mistra_chem_integrate_ex(0, 1, None, None, None, 0.0, 10.0, None, None, None, None)
    assert rc != 0 and b"no HIP device" in lib.mistra_chem_last_error()
    # compute entry point without init: error, not a silent result
    out = np.zeros(102)
    dp = C.POINTER(C.c_double)
    rc = lib.mistra_chem_integrate(0, 1, out.ctypes.data_as(dp), out.ctypes.data_as(dp), out.ctypes.data_as(dp), 0.0, 10.0,
                                   out.ctypes.data_as(dp), None, None)
    assert rc != 0


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under mistra_amd/ may reference it."""
    for root, _, files in os.walk(os.path.join(REPO, "mistra_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                text = open(os.path.join(root, f), errors="replace").read()
                assert "oracle." not in text and "oracle/" not in text and "kpp_ros3" not in text and "libmistra_ref" not in text, f


def test_lookahead_ring_registers_are_out_of_the_compilers_reach():
    """ros3_kernel.hip streams its tables through a ring of fixed VGPRs (v192..v247, or four blocks from v64 up for the mechanisms run at three or
    four waves per SIMD) inside two non-inlined device functions; that is only sound while the compiler's own values in those
    functions stay below the ring (build.py scans the
    generated gfx950 assembly).  Cross-compiles, no GPU needed."""
    from mistra_amd.build import ring_register_report
    rep = ring_register_report()          # raises if a function's own registers reach its ring
    dev = {k: v for k, v in rep.items() if "gsum_run" in k or "tail_solve" in k or "scale_run" in k}      # (three gsum_run, five tail_solve, two scale_run)
    assert len(dev) >= 9, rep
    low = {k: v for k, v in dev.items() if "Lb1E" in k}
    assert low and max(low.values()) < 64, low      # (ring_register_report has raised already if not)


def test_ring_register_table_matches_the_generated_gather_sum_stream():
    """The look-ahead ring's sixteen slots are stated once in ros3_kernel.hip (MISTRA_RING_LO<K> / MISTRA_RING_HI<K>) and once in
    tools/gen_gsum_asm.py (SLOTS), whose generated stream loads and clobbers the same registers: the two tables agree."""
    import re
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_gsum_asm
    finally:
        sys.path.pop(0)
    text = open(os.path.join(REPO, "mistra_amd", "csrc", "ros3_kernel.hip")).read()
    table = {(m.group(1), int(m.group(2))): [int(r) for r in m.group(3).split(",")]
             for m in re.finditer(r"^#define MISTRA_RING_(LO|HI)(\d) ([\d, ]+)$", text, re.M)}
    assert len(table) == 16, sorted(table)
    for half, name in (("LO", "LOW"), ("HI", "HIGH")):
        for k, first in enumerate(gen_gsum_asm.SLOTS[name]):
            assert table[(half, k)] == [first, first + 1, first + 2, first + 3], (half, k)


@pytest.mark.parametrize("tool", ["gen_vm_asm.py", "gen_gsum_asm.py", "gen_rates_shim.py"])
def test_generated_sources_are_up_to_date(tool):
    """mistra_amd/csrc/vm_exec_asm.inc, gsum_exec_asm.inc and shim/mistra_kpp_rates.f90 are generator output kept in the tree: what is committed is what
    the generator writes today."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", tool), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _read_tables(path, count):
    """`count` tables of the 'KRAT' v2 format back to back (a .rates file holds one, a .stcoeff file four) -> [(header, consts, offs, words, fslot)]"""
    raw = open(path, "rb").read()
    off, out = 0, []
    for _ in range(count):
        h = np.frombuffer(raw, np.int32, 8, off).copy()
        off += 32
        parts = []
        for dt, n in ((np.float64, h[4]), (np.int32, h[2] + 1), (np.int32, h[5]), (np.int32, h[6])):
            parts.append(np.frombuffer(raw, dt, int(n), off).copy())
            off += int(n) * np.dtype(dt).itemsize
        out.append((h, *parts))
    assert off == len(raw)
    return out


def _write_tables(path, tables):
    with open(path, "wb") as f:
        for h, consts, offs, words, fslot in tables:
            h = h.copy()
            h[4], h[5] = len(consts), len(words)
            for a, dt in ((h, np.int32), (consts, np.float64), (offs, np.int32), (words, np.int32), (fslot, np.int32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())


def _with_first_program(table, pushes):
    """the table with its first program replaced by `pushes` literals summed up: that program needs `pushes` operand-stack entries"""
    h, consts, offs, words, fslot = table
    prog = np.array([0] * pushes + [2] * (pushes - 1), np.int32)      # word = opcode | operand << 8: literal 0, pushes times; then +
    old = offs[1] - offs[0]
    return (h, consts, np.concatenate([offs[:1], offs[1:] + (len(prog) - old)]), np.concatenate([prog, words[old:]]), fslot)


@pytest.mark.parametrize("kind", ["rates", "stcoeff"])
def test_loader_refuses_a_table_deeper_than_the_evaluators_stack(lib, tmp_path, kind):
    """The device evaluator keeps its operand stack in a fixed column of kRatesStackDepth = 12 doubles per thread (mistra_amd/csrc/rates.hpp); a program
    that pushes a thirteenth would write into the next column.  The library's own loaders (RatesTable::load, StcoeffTable::load, reached without a
    device through mistra_chem_table_stack_depth) take a crafted table whose first program needs 12 entries and refuse one that needs 13."""
    lib.mistra_chem_table_stack_depth.argtypes = [C.c_char_p, C.c_int]
    mech, count = ("gas", 1) if kind == "rates" else ("aer", 4)
    shipped = os.path.join(REPO, "mistra_amd", "mech", "%s.%s" % (mech, kind))
    tables = _read_tables(shipped, count)
    assert lib.mistra_chem_table_stack_depth(shipped.encode(), count == 4) == (7 if kind == "rates" else 8)
    for which in range(count):
        for pushes, accepted in ((12, True), (13, False)):
            path = str(tmp_path / ("%d_%d.%s" % (which, pushes, kind)))
            _write_tables(path, [_with_first_program(t, pushes) if i == which else t for i, t in enumerate(tables)])
            got = lib.mistra_chem_table_stack_depth(path.encode(), count == 4)
            if accepted:
                assert got == 12, lib.mistra_chem_last_error()
            else:
                assert got == -1
                msg = lib.mistra_chem_last_error().decode()
                assert "needs 13 operand-stack entries" in msg and "holds 12" in msg and path in msg
    # a program that pops from an empty stack, or leaves two results, is no program
    h, consts, offs, words, fslot = tables[0]
    for bad in (np.array([2], np.int32), np.array([0, 0], np.int32)):
        old = offs[1] - offs[0]
        t = (h, consts, np.concatenate([offs[:1], offs[1:] + (len(bad) - old)]), np.concatenate([bad, words[old:]]), fslot)
        path = str(tmp_path / ("bad." + kind))
        _write_tables(path, [t] + tables[1:])
        assert lib.mistra_chem_table_stack_depth(path.encode(), count == 4) == -1
