"""Host restatement of the gather-sum programs (schedule.hpp: GsumProgram, GsumChain), shared by tests/test_gsum_chain.py and
tests/test_gpu_gsum_chain.py: the tables come through mistra_chem_gsum_program (no device needed), the arithmetic is numpy float64 with one
rounding per operation — a regular row as acc = acc + c * M[a], a chain step as A = A + p."""
import ctypes
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_VDOT, JVS, LEAN_VDOT, PASSES = 0, 1, 2, 3
INFO = ("nt", "nw", "nq", "words", "on", "npass", "pole_rows_full", "pole_rows_lean", "pole_cycles_full", "pole_cycles_lean", "zero", "trash", "src", "xs")


def load_lib(path=None):
    lib = ctypes.CDLL(path or os.environ.get("MISTRA_CHEM_LIB") or os.path.join(REPO, "mistra_amd", "lib", "libmistra_chem.so"))
    lib.mistra_chem_gsum_program.restype = ctypes.c_int
    lib.mistra_chem_last_error.restype = ctypes.c_char_p
    return lib


def program(lib, mech, which):
    """-> dict: the INFO fields, wave_base, rows, mask, chained, pass_wave, recs[rows total][64][8] (uint32)"""
    os.environ.setdefault("MISTRA_MECH_DIR", os.path.join(REPO, "mistra_amd", "mech"))
    info = (ctypes.c_int64 * 14)()
    null = ctypes.c_void_p(0)
    if lib.mistra_chem_gsum_program(mech, which, info, null, null, null, null, null, null, ctypes.c_int64(0)) != 0:
        raise RuntimeError(lib.mistra_chem_last_error().decode())
    P = dict(zip(INFO, [int(v) for v in info]))
    nw, npass = P["nw"], P["npass"]
    wave_base = np.zeros(nw, np.uint32)
    rows = np.zeros(nw, np.int32)
    mask = np.zeros(nw, np.uint64)
    chained = np.full(max(1, 4 * npass), -1, np.int32)
    pass_wave = np.zeros(max(1, npass), np.int32)
    recs = np.zeros(P["words"], np.uint32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    if lib.mistra_chem_gsum_program(mech, which, info, ptr(wave_base), ptr(rows), ptr(mask), ptr(chained), ptr(pass_wave), ptr(recs),
                                    ctypes.c_int64(recs.size)) != 0:
        raise RuntimeError(lib.mistra_chem_last_error().decode())
    P.update(wave_base=wave_base, rows=rows, mask=mask, chained=chained[:4 * npass], pass_wave=pass_wave[:npass], recs=recs.reshape(-1, 64, 8))
    return P


def run_rows(P, M, out_addr, out_stride):
    """The regular executor on LDS image M (float64, indexed by byte address / 8; modified in place): every wave's rows in order, lane l of
    wave w flushing to out_addr[w*64+l], then every out_stride[w*64+l] bytes.  -> number of stores per cell index (dict)"""
    stores = {}
    with np.errstate(all="ignore"):
        for w in range(P["nw"]):
            acc = np.full(64, -0.0)
            out = out_addr[w * 64:(w + 1) * 64].astype(np.int64).copy()
            for r in range(int(P["rows"][w])):
                rec = P["recs"][int(P["wave_base"][w]) + r]
                addr = rec[:, :4].astype(np.int64)
                coef = rec[:, 4:].copy().view(np.float32).astype(np.float64)
                flush = addr[0, 0] & 1
                assert ((addr[:, 0] & 1) == flush).all(), "the flush mark is the row's, in every lane"
                addr[:, 0] &= ~7
                for k in range(4):
                    acc = acc + coef[:, k] * M[addr[:, k] // 8]
                if flush:
                    for l in range(64):
                        M[out[l] // 8] = acc[l]
                        stores[int(out[l] // 8)] = stores.get(int(out[l] // 8), 0) + 1
                    out += out_stride[w * 64:(w + 1) * 64]
                    acc = np.full(64, -0.0)
    return stores


def run_passes(P, M):
    """The chain passes on LDS image M: per pass and 16-lane row, A = -0.0, then A = A + p[16 g + i] for g < G, i < 16, stored to the
    cell the pass names.  -> number of stores per cell index (dict)"""
    stores = {}
    with np.errstate(all="ignore"):
        for w in range(P["nw"]):
            assert P["rows"][w] % 4 == 0
            for p in range(int(P["rows"][w]) // 2):
                r0 = P["recs"][int(P["wave_base"][w]) + 2 * p]
                r1 = P["recs"][int(P["wave_base"][w]) + 2 * p + 1]
                G = int(r0[0, 0] & 7)
                assert ((r0[:, 0] & 7) == G).all(), "the group count is the pass's, in every lane"
                if G == 0:
                    continue
                addr = np.concatenate([r0[:, :4], r1[:, :4]], axis=1).astype(np.int64)
                coef = np.concatenate([r0[:, 4:], r1[:, 4:]], axis=1).copy().view(np.float32).astype(np.float64)
                addr[:, 0] &= ~7
                prod = coef[:, :7] * M[addr[:, :7] // 8]
                for R in range(4):
                    A = np.float64(-0.0)
                    for g in range(G):
                        for i in range(16):
                            A = A + prod[16 * R + i, g]
                    cells = addr[16 * R:16 * R + 16, 7] // 8
                    assert (cells == cells[0]).all(), "one output cell per 16-lane row"
                    M[cells[0]] = A
                    stores[int(cells[0])] = stores.get(int(cells[0]), 0) + 1
    return stores
