"""The tail chain's address tables (mistra_amd/csrc/schedule.hpp: TailSolve::fwd_addr / bwd_addr): one table per register and
direction, the words of the host-side 16-bit tables (two Ghimj cells per word, the form the emulator reads) as LDS
byte addresses, 8 * cell, in the same group / lane / column layout — slack and absent operands on the 0.0 cell.  The tail
chain of ros3_kernel.hip (tail_solve) gathers through them straight from its look-ahead ring."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "mistra_amd", "csrc")
NT = {"gas": 64, "aer": 256, "tot": 512}      # threads per cell of the product kernels (ros3_kernel.hpp)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler here")
    lib = str(tmp_path_factory.mktemp("probe") / "libtail_probe.so")
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-o", lib, os.path.join(REPO, "tests", "probe", "tail_tables.cpp"),
                    os.path.join(CSRC, "schedule.cpp"), os.path.join(CSRC, "mech_tables.cpp")], check=True)
    p = C.CDLL(lib)
    p.tail_probe_create.restype = C.c_void_p
    p.tail_probe_create.argtypes = [C.c_char_p, C.c_int]
    p.tail_probe_destroy.argtypes = [C.c_void_p]
    p.tail_probe_regs.argtypes = [C.c_void_p]
    p.tail_probe_zero_cell.argtypes = [C.c_void_p]
    p.tail_probe_table.restype = C.c_long
    p.tail_probe_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    return p


def table(p, h, which):
    n = p.tail_probe_table(h, which, None, 0)
    out = np.zeros(n, np.uint32)
    p.tail_probe_table(h, which, out.ctypes.data, n)
    return out


@pytest.mark.parametrize("mech", ["gas", "aer", "tot"])
def test_address_words_are_the_cells_times_eight(probe, mech):
    h = probe.tail_probe_create(os.path.join(REPO, "mistra_amd", "mech", mech + ".mech").encode(), NT[mech])
    assert h, "schedule compiler failed"
    try:
        regs, zero = probe.tail_probe_regs(h), probe.tail_probe_zero_cell(h)
        assert regs in (1, 2)
        m = 64 * regs
        for d, name in enumerate(("fwd", "bwd")):
            cells = table(probe, h, d)
            assert cells.size == (m // 4 + 16) * 256          # + VM_LOOKAHEAD_ROWS groups of slack
            for r in range(2):
                addr = table(probe, h, 2 + 2 * d + r)
                if r >= regs:
                    assert addr.size == 0, "%s_addr[%d] built for a one-register tail" % (name, r)
                    continue
                want = ((cells >> np.uint32(16 * r)) & np.uint32(0xFFFF)).astype(np.uint64) * 8
                assert addr.size == cells.size
                assert np.array_equal(addr.astype(np.uint64), want), "%s_addr[%d]" % (name, r)
                slack = addr[(m // 4) * 256:]
                assert np.all(slack == 8 * zero), "slack rows of %s_addr[%d] off the 0.0 cell" % (name, r)
                # the chain's operands: every word is some Ghimj cell or the 0.0 cell, and the register's strictly-lower (fwd) /
                # strictly-upper (bwd) entries are there
                assert np.all(addr % 8 == 0) and np.all(addr // 8 <= zero)
                assert np.count_nonzero(addr != 8 * zero) > 0
    finally:
        probe.tail_probe_destroy(h)
