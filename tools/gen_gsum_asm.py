#!/usr/bin/env python3
"""Writes mistra_amd/csrc/gsum_exec_asm.inc: the gfx950 instruction stream of the gather-sum machine (ros3_kernel.hip: gsum_run), one
variant per placement of the look-ahead ring, as C string literals.

    python tools/gen_gsum_asm.py          (the output is committed; tests/test_capi.py checks that it is up to date)

The machine, per table row (schedule.hpp: four LDS byte addresses — the first one carries the flush mark in bit 0 — and four float
coefficients per lane):
    acc = acc + (double)c0 * M[a0];  ... c1, c2, c3 likewise, left to right, one rounding per operation;
    a marked row completes the lane's current output:  M[out] = acc;  out += stride;  acc = -0.0
Why assembly: a wave that walks a long sum alone (four species of tot have 108 terms, 27 rows, where the average wave has 3) is bound
by instruction ISSUE — one instruction per 4-7 cycles whatever it is — and the compiler's version of a row was ~39 instructions: the
table words copied out of the ring (8 moves), then masked, converted and used.  Here the consumers read the ring registers themselves
and the loads take scalar bases (fixed; the lane's offset moves on by 8 KiB per group of four rows): 25 instructions per row.  Software pipeline as in the LDS VM executor: the gathers of row r+1 are
issued before the additions of row r (two operand sets, A and B); only the additions are serial along a sum.  Same terms, same order,
same three operations per term: bit-identical sums.

Ring: 8 slots of 4 registers in caller-saved blocks (ros3_kernel.hip: vm_ring_load), row r of a group of four in slots 2r (addresses)
and 2r+1 (coefficients); a row is refilled with the row four further on as soon as its words have been consumed.
Wait counts: table loads return in order, 8 in flight when a row is taken: vmcnt(6) = its two have landed.  LDS returns in order; when
set P is summed the only younger operations in flight are the 4 gathers of the other set (and possibly the store of a flush in
between, which lgkmcnt(4) then waits for as well).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "mistra_amd", "csrc", "gsum_exec_asm.inc")

# the kernel's copy of these blocks: the MISTRA_RING_LO<K> / MISTRA_RING_HI<K> table of ros3_kernel.hip (tests/test_capi.py compares them)
SLOTS = {"LOW": [64, 68, 80, 84, 96, 100, 112, 116], "HIGH": [192, 196, 208, 212, 224, 228, 240, 244]}


def variant(name, fill=True, barrier=False, chain=False):
    """fill: the stream fills its own ring (else it enters on a ring that the stream in front of it filled: its first four rows
    are in flight, issued in the order a fill issues them, so the counted waits below hold as they stand).
    barrier: the workgroup barrier in front of the stream sits behind the fill — table loads do not depend on LDS, the gathers do.
    chain: in the last ring turn the refills fetch the NEXT stream's first four rows (%[nb0], %[nb1]: its base less the distance
    %[voff] has moved on by then, 8 KiB per group of four rows) where they would fetch slack rows, and the stream returns with
    those loads in flight."""
    slot = SLOTS[name]
    L = []
    emit = L.append

    def load_row(r):            # rows 0, 1 of a group through %[b0] (immediates < 4096), rows 2, 3 through %[b1] = b0 + 4096
        base, off = ("%[b0]", r * 2048) if r < 2 else ("%[b1]", (r - 2) * 2048)
        a, c = slot[2 * r], slot[2 * r + 1]
        emit("global_load_dwordx4 v[%d:%d], %%[voff], %s offset:%d" % (a, a + 3, base, off))
        emit("global_load_dwordx4 v[%d:%d], %%[voff], %s offset:%d" % (c, c + 3, base, off + 16))

    def fetch(r, s):            # take row r's words: mark, gathers, coefficients into set s; then refill its slots
        a, c = slot[2 * r], slot[2 * r + 1]
        emit("s_waitcnt vmcnt(6)")
        emit("v_and_b32 %%[ad], -8, v%d" % a)
        emit("ds_read_b64 %%[x%s0], %%[ad]" % s)
        for k in (1, 2, 3):
            emit("ds_read_b64 %%[x%s%d], v%d" % (s, k, a + k))
        emit("v_readfirstlane_b32 %%[fl%s], v%d" % (s, a))
        for k in range(4):
            emit("v_cvt_f64_f32 %%[c%s%d], v%d" % (s, k, c + k))
        load_row(r)

    def summ(s, tag):
        emit("s_waitcnt lgkmcnt(4)")
        for k in range(4):
            emit("v_mul_f64 %%[c%s%d], %%[c%s%d], %%[x%s%d]" % (s, k, s, k, s, k))
            emit("v_add_f64 %%[acc], %%[acc], %%[c%s%d]" % (s, k))
        emit("s_bitcmp1_b32 %%[fl%s], 0" % s)
        emit("s_cbranch_scc0 Lgs_nf%s_%%=" % tag)
        emit("ds_write_b64 %[out], %[acc]")
        emit("v_add_u32 %[out], %[out], %[stride]")
        emit("v_mov_b64 %[acc], %[mzero]")
        emit("Lgs_nf%s_%%=:" % tag)

    def to_next():              # from here on the refills fetch the next stream (scalar registers written by scalar instructions: no wait states)
        emit("s_mov_b64 %[b0], %[nb0]")
        emit("s_mov_b64 %[b1], %[nb1]")

    if fill:
        emit("s_waitcnt vmcnt(0)")          # nothing of the caller's may sit between the counted loads
        emit("s_nop 4")                     # (the bases may have been written by v_readfirstlane just before: 5 wait states before a memory instruction reads them)
        for r in range(4):
            load_row(r)
    if barrier:
        emit("s_waitcnt lgkmcnt(0)")        # the caller's LDS stores are done (lds_barrier's release), then the barrier itself
        emit("s_barrier")
    if chain:
        emit("s_cmp_lt_i32 %[n], 1")
        emit("s_cbranch_scc1 Lgs_none_%=")
        emit("v_add_u32 %[voff], 0x2000, %[voff]")
        emit("s_cmp_lt_i32 %[n], 5")        # one group only: its refills are the last turn's
        emit("s_cbranch_scc0 Lgs_go_%=")
        to_next()
        emit("Lgs_go_%=:")
    else:
        emit("v_add_u32 %[voff], 0x2000, %[voff]")      # the next group of four rows
        emit("s_cmp_lt_i32 %[n], 1")
        emit("s_cbranch_scc1 Lgs_exit_%=")
    fetch(0, "A")
    emit("Lgs_loop_%=:")
    fetch(1, "B"); summ("A", "0")
    fetch(2, "A"); summ("B", "1")
    fetch(3, "B"); summ("A", "2")
    emit("v_add_u32 %[voff], 0x2000, %[voff]")
    emit("s_sub_i32 %[n], %[n], 4")
    if chain:
        emit("s_cmp_lt_i32 %[n], 5")        # (the main line carries the same three scalar instructions as without a next stream)
        emit("s_cbranch_scc1 Lgs_few_%=")
    else:
        emit("s_cmp_lt_i32 %[n], 1")
        emit("s_cbranch_scc1 Lgs_last_%=")
    fetch(0, "A"); summ("B", "3")
    emit("s_branch Lgs_loop_%=")
    if chain:
        emit("Lgs_few_%=:")
        emit("s_cmp_lt_i32 %[n], 1")
        emit("s_cbranch_scc1 Lgs_last_%=")
        to_next()                           # one group left: the last ring turn begins with this refill
        fetch(0, "A"); summ("B", "5")
        emit("s_branch Lgs_loop_%=")
    emit("Lgs_last_%=:")
    emit("s_waitcnt lgkmcnt(0)")
    summ("B", "4")
    if chain:
        emit("s_branch Lgs_exit_%=")
        emit("Lgs_none_%=:")                # a wave without rows: its own fill was for nothing, the next stream's takes its place
        emit("s_waitcnt vmcnt(0)")
        to_next()
        for r in range(4):
            load_row(r)
        emit("Lgs_exit_%=:")
        emit("s_waitcnt lgkmcnt(0)")        # stores done; the next stream's first four rows stay in flight
    else:
        emit("Lgs_exit_%=:")
        emit("s_waitcnt vmcnt(0) lgkmcnt(0)")      # the look-ahead loads have landed before the ring registers are reused; stores done
    clob = ", ".join('"v%d"' % (b + k) for b in slot for k in range(4))
    return L, clob


def pass_variant(name, barrier):
    """The chain passes of a wave (schedule.hpp: GsumChain; ros3_kernel.hip: gsum_pass_run): a stream of whole ring turns, two passes of
    two rows each per turn, no look-ahead beyond the turn (a wave has one or two passes).  Per pass: seven gathers and products as a
    regular row forms them — slots 0-3 from the first row into set A, 4-6 from the second into set B, the products left in the
    coefficient registers —, then the running sum takes them in term order, group by group: sixteen `acc = fma(p[lane i], 1.0, acc)`
    with the product broadcast over its 16-lane row.  The DPP operand is a product written at least two instructions earlier, the
    dependency runs through the destination only.  The group count G sits in the three low bits of the pass's first address word
    (tested between the groups, wave-uniform; 0 = an empty pass), the output's address in the last address word of its second row.
    n >= 4 on entry."""
    slot = SLOTS[name]
    L = []
    emit = L.append

    def load_turn():
        for r in range(4):
            base, off = ("%[b0]", r * 2048) if r < 2 else ("%[b1]", (r - 2) * 2048)
            a, c = slot[2 * r], slot[2 * r + 1]
            emit("global_load_dwordx4 v[%d:%d], %%[voff], %s offset:%d" % (a, a + 3, base, off))
            emit("global_load_dwordx4 v[%d:%d], %%[voff], %s offset:%d" % (c, c + 3, base, off + 16))

    def one_pass(ra, rb, tag):
        a, c = slot[2 * ra], slot[2 * ra + 1]
        b, d = slot[2 * rb], slot[2 * rb + 1]
        prod = ["%%[cA%d]" % k for k in range(4)] + ["%%[cB%d]" % k for k in range(3)]
        emit("v_readfirstlane_b32 %%[flA], v%d" % a)
        emit("v_and_b32 %%[ad], -8, v%d" % a)
        emit("ds_read_b64 %[xA0], %[ad]")
        for k in (1, 2, 3):
            emit("ds_read_b64 %%[xA%d], v%d" % (k, a + k))
        for k in range(3):
            emit("ds_read_b64 %%[xB%d], v%d" % (k, b + k))
        for k in range(4):
            emit("v_cvt_f64_f32 %%[cA%d], v%d" % (k, c + k))
        for k in range(3):
            emit("v_cvt_f64_f32 %%[cB%d], v%d" % (k, d + k))
        emit("v_mov_b64 %[acc], %[mzero]")
        emit("s_and_b32 %[flA], %[flA], 7")
        emit("s_cmp_eq_u32 %[flA], 0")
        emit("s_cbranch_scc1 Lgp_skip%s_%%=" % tag)
        emit("s_waitcnt lgkmcnt(0)")
        for k in range(4):
            emit("v_mul_f64 %%[cA%d], %%[cA%d], %%[xA%d]" % (k, k, k))
        for k in range(3):
            emit("v_mul_f64 %%[cB%d], %%[cB%d], %%[xB%d]" % (k, k, k))
        for g in range(7):
            if g:
                emit("s_cmp_lt_u32 %%[flA], %d" % (g + 1))
                emit("s_cbranch_scc1 Lgp_st%s_%%=" % tag)
            for i in range(16):
                emit("v_fmac_f64_dpp %%[acc], %s, %%[one] row_newbcast:%d row_mask:0xf bank_mask:0xf" % (prod[g], i))
        emit("Lgp_st%s_%%=:" % tag)
        emit("ds_write_b64 v%d, %%[acc]" % (b + 3))
        emit("Lgp_skip%s_%%=:" % tag)

    emit("s_waitcnt vmcnt(0)")
    emit("s_nop 4")
    load_turn()
    if barrier:
        emit("s_waitcnt lgkmcnt(0)")
        emit("s_barrier")
    emit("Lgp_loop_%=:")
    emit("v_add_u32 %[voff], 0x2000, %[voff]")
    emit("s_waitcnt vmcnt(0)")
    one_pass(0, 1, "0")
    one_pass(2, 3, "1")
    emit("s_waitcnt lgkmcnt(0)")            # the turn's gathers and stores have read their ring registers
    emit("s_sub_i32 %[n], %[n], 4")
    emit("s_cmp_lt_i32 %[n], 1")
    emit("s_cbranch_scc1 Lgp_exit_%=")
    load_turn()
    emit("s_branch Lgp_loop_%=")
    emit("Lgp_exit_%=:")
    return L


# the streams ros3_kernel.hip runs: suffix -> (fill, barrier, chain)
FORMS = [("", (True, False, False)),                 # gsum_run: fill, run, drain
         ("_BAR", (True, True, False)),              # gsum_run_bar: fill, workgroup barrier, run, drain
         ("_CHAIN", (True, False, True)),            # gsum_run_pair, first program: fill, run, leave the second program's first rows in flight
         ("_BAR_CHAIN", (True, True, True)),         #   ... with the workgroup barrier behind the fill
         ("_PRIMED", (False, False, False))]         # gsum_run_pair, second program: run on the ring as filled, drain


def render():
    out = ["// GENERATED by tools/gen_gsum_asm.py — do not edit.  Instruction stream of the gather-sum machine (ros3_kernel.hip: gsum_run).", ""]
    for name in ("LOW", "HIGH"):
        for suffix, form in FORMS:
            if name == "LOW" and suffix:      # the low placement (gas) runs the plain form only
                continue
            lines, clob = variant(name, *form)
            out.append("#define MISTRA_GSUM_ASM_%s%s \\" % (name, suffix))
            for i, ln in enumerate(lines):
                sep = "\\n" if ln.endswith(":") else "\\n\\t"
                last = i == len(lines) - 1
                out.append('  "%s%s"%s' % (ln, "" if last else sep, "" if last else " \\"))
            out.append("")
        for suffix, barrier in (("_PASS", False), ("_PASS_BAR", True)) if name == "HIGH" else ():
            lines = pass_variant(name, barrier)
            out.append("#define MISTRA_GSUM_ASM_%s%s \\" % (name, suffix))
            for i, ln in enumerate(lines):
                sep = "\\n" if ln.endswith(":") else "\\n\\t"
                last = i == len(lines) - 1
                out.append('  "%s%s"%s' % (ln, "" if last else sep, "" if last else " \\"))
            out.append("")
        out.append("#define MISTRA_GSUM_CLOBBER_%s %s" % (name, clob))
        out.append("")
    return "\n".join(out)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text else 1)
    open(OUT, "w").write(text)
    print("wrote", os.path.normpath(OUT), "(%d lines)" % text.count("\n"))
