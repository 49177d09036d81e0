// One workgroup integrates one grid cell: the whole Ros3 Rosenbrock step loop of the reference
// (INTEGRATE_x -> Rosenbrock_x -> RosenbrockIntegrator_x, gas.f:710-1337 | aer.f:1408-2035 | tot.f:2812-3439)
// runs inside the kernel with the cell's state on chip:
//
//   LDS        M  = [ Ghimj (LU_NONZERO) | XS (NVAR) ]   matrix being factorised / solve vector   (LDS VM memory)
//              X  = [ V (NVAR) | F (NFIX) | consts ]     extended species vector read by Fun/Jac products
//              AB = A(NREACT) or B(NB)                   rate products, then Jacobian products
//   registers  one species per lane-slot: Y, Ynew, Fcn0, Fcn, K1..K3 (thread t owns species q*NT+t);
//              RCONST of the reactions the thread owns; the structurally non-zero entries of Jac0
//   HBM        read VAR, FIX, RCONST once (coalesced, cell-major), write VAR once; schedule words stream from L2
//
// gfx950 only.  Built with -ffp-contract=off: every multiply and add/subtract rounds once, as in the reference
// built without FMA contraction.  MFMA (v_mfma_f64_16x16x4_f64) is used in ONE place: the last 64x64 block of the tot
// mechanism's LU, which fill-in makes completely dense (dense_lu below); everything else is sparse gather arithmetic.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kernel_args.hpp"
#include "ros3_kernel.hpp"
#include "ros_methods.hpp"
#include "wave_ops.hpp"

namespace mistra {

namespace {

constexpr uint16_t kPosDiag = 0x8000, kPosNone = 0xFFFF;
constexpr int kRingSlots = 8;  // 16-byte table loads in flight per lane (schedule.cpp appends 2x that many rows of slack)

// ---- table-stream start-up: every table-driven executor call opened with a whole table round trip in which its
// waves did nothing else.  The sites below move the ring fill in front of what the call waited for anyway, or take it over from
// the stream in front; each has a compile-time switch (on in the product build; tools/build_variant.sh NAME -DMISTRA_STREAM_...=0
// builds the library without one, for same-box A/B runs).  No table, record, operation or order of operations differs.
// The low ring placement (gas) keeps the executors it had.  (Tried and taken out again: the tail chain's ring filled ahead)
#ifndef MISTRA_STREAM_GSUM_BARRIER      // Fun / Jac sums: ring fill in front of the barrier behind the products (gsum_run_bar)
#define MISTRA_STREAM_GSUM_BARRIER 1
#endif
#ifndef MISTRA_STREAM_GSUM_CHAIN        // fun_jac: the JVS program enters on rows the Vdot program fetched in its last ring turn (gsum_run_pair)
#define MISTRA_STREAM_GSUM_CHAIN 1
#endif
#ifndef MISTRA_STREAM_SWEEP_BARRIER     // head sweeps of the solves: ring fill in front of the barrier they follow (vm_run<.., true>)
#define MISTRA_STREAM_SWEEP_BARRIER 1
#endif
#ifndef MISTRA_STREAM_SCALE_TRIM        // scale_run: the last ring turn issues no refills (they fetched rows nobody reads, drained on the spot)
#define MISTRA_STREAM_SCALE_TRIM 1
#endif

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // plain vector types load from any address space
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <class T>
using gptr = const T __attribute__((address_space(1)))*;
template <class T>
using gptr_mut = T __attribute__((address_space(1)))*;
template <class T>
__device__ __forceinline__ gptr<T> G_(const T* p) { return (gptr<T>)p; }
template <class T>
__device__ __forceinline__ gptr_mut<T> GM_(T* p) { return (gptr_mut<T>)p; }

// LDS accesses by 32-bit LDS address.  A `double*` that crosses a (non-inlined) function boundary is a generic pointer:
// every access through it pays a generic->LDS conversion with a null check (4 VALU + a scalar load per operand).
typedef __attribute__((address_space(3))) double lds_f64;
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
__device__ __forceinline__ double lds_ld(uint32_t addr) { return *(const lds_f64*)(uintptr_t)addr; }
__device__ __forceinline__ void lds_st(uint32_t addr, double v) { *(lds_f64*)(uintptr_t)addr = v; }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() would also drain vmcnt, i.e. wait for the
// schedule-table prefetches that are deliberately kept in flight across rounds.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Ros3_x (gas.f:1596-1626)
constexpr double kRosA1 = 1.0;
constexpr double kRosC1 = -0.10156171083877702091975600115545e+01;
constexpr double kRosC2 = 0.40759956452537699824805835358067e+01;
constexpr double kRosC3 = 0.92076794298330791242156818474003e+01;
constexpr double kRosM1 = 0.1e+01;
constexpr double kRosM2 = 0.61697947043828245592553615689730e+01;
constexpr double kRosM3 = -0.42772256543218573326238373806514e+00;
constexpr double kRosE1 = 0.5e+00;
constexpr double kRosE2 = -0.29079558716805469821718236208017e+01;
constexpr double kRosE3 = 0.22354069897811569627360909276199e+00;
constexpr double kRosGamma1 = 0.43586652150845899941601945119356e+00;
[[maybe_unused]] constexpr double kRosGamma2 = 0.24291996454816804366592249683314e+00;
[[maybe_unused]] constexpr double kRosGamma3 = 0.21851380027664058511513169485832e+01;
constexpr double kRosElo = 3.0;

// Err**(1/ros_ELO) of the step-size controller (gas.f:1303).  Not inlined: the library routine's two dozen polynomial
// coefficients were hoisted out of the step loop as live registers, and the 128-register kernel spilled them to scratch and
// read them back every step (most of its HBM-side traffic).  The 256-register kernel keeps the inlined form (0.7 % faster there).
__device__ __attribute__((noinline)) double err_root(double err) { return pow(err, 1.0 / kRosElo); }
// the method kernels' (ros_ELO = 2 and 4: Ros2, Ros4, Rodas4), likewise
[[maybe_unused]] __device__ __attribute__((noinline)) double err_root_elo(double err, double inv_elo) { return pow(err, inv_elo); }

// A value every lane of the wave holds identically (time, step size: sums reduced in a fixed order, the same in all lanes),
// moved to scalar registers: the register-starved kernels spilled these to scratch at the head of the step loop.
__device__ __forceinline__ double wave_uniform(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
  return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}

// A constant formed in scalar registers where it is used: hoisted out of the step loop, 0.1 became a vector-register pair the
// register-starved kernels kept in scratch and re-read three times per step.
__device__ __forceinline__ double scalar_const(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
  asm volatile("" : "+s"(lo), "+s"(hi));
  return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}

// Sum over the wave, the same value in every lane: six pairing steps in which both partners add the same two numbers (so all lanes
// agree bit for bit).  Inside a lane row the partner's value comes by DPP (quad swaps, half-row mirror, row mirror: ~10 cycles a step),
// across lane rows by v_permlane16/32_swap; __shfl_xor went through ds_bpermute, an LDS round trip per step (six of them: ~800 cycles of
// every step's error norm).
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_partner<0xB1>(v);       // quad_perm [1,0,3,2]
  v += dpp_partner<0x4E>(v);       // quad_perm [2,3,0,1]
  v += dpp_partner<0x141>(v);      // row_half_mirror: quads 0 <-> 1, 2 <-> 3
  v += dpp_partner<0x140>(v);      // row_mirror: lanes 0-7 <-> 8-15
  {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    // permlane16_swap(a, b) from a = b: a = [r0 r0 r2 r2], b = [r1 r1 r3 r3] (lane rows): their sum pairs rows 0+1 and 2+3 in every lane
    const auto l = __builtin_amdgcn_permlane16_swap((uint32_t)u, (uint32_t)u, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap((uint32_t)(u >> 32), (uint32_t)(u >> 32), false, false);
    v = __builtin_bit_cast(double, (uint64_t)l[0] | ((uint64_t)h[0] << 32)) + __builtin_bit_cast(double, (uint64_t)l[1] | ((uint64_t)h[1] << 32));
  }
  {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    // permlane32_swap(a, b) from a = b: a = [lower lower], b = [upper upper]
    const auto l = __builtin_amdgcn_permlane32_swap((uint32_t)u, (uint32_t)u, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap((uint32_t)(u >> 32), (uint32_t)(u >> 32), false, false);
    v = __builtin_bit_cast(double, (uint64_t)l[0] | ((uint64_t)h[0] << 32)) + __builtin_bit_cast(double, (uint64_t)l[1] | ((uint64_t)h[1] << 32));
  }
  return v;
}

__device__ __forceinline__ double fmin_f(double a, double b) { return (a < b || b != b) ? a : b; }   // Fortran MIN
__device__ __forceinline__ double fmax_f(double a, double b) { return (a > b || b != b) ? a : b; }   // Fortran MAX

// ---- table look-ahead ring of the tail chain and the gather-sum machine: eight 16-byte loads in flight per lane.
// hipcc's own s_waitcnt placement falls back to vmcnt(0) around branches and barriers, which would serialise every
// table row behind a full memory round trip, so the loads are issued from asm and counted by hand.  A compiler-visible
// VGPR destination would be unsafe (the compiler may copy an asm output before the data lands, cdna_hip_programming.md
// §5.7 item 1).  The ring therefore lives in fixed registers named only by the statements built from the table below; a consume
// statement waits and copies out (or gathers through the words) in ONE asm (§5.7 form i).  Loads are in flight only inside the
// non-inlined functions that use the ring (gsum_run, tail_solve, scale_run: each drains it before returning), and those functions' own values sit below the ring (they need
// < 64 registers; mistra_amd/build.py checks the generated ISA before it links), so nothing of the compiler's can be hit by a landing
// load; the callers see the blocks as ordinary call-clobbered registers.  Two placements (LOW):
//   false  v192-199, v208-215, v224-231, v240-247: four caller-saved blocks at the top of the file, nothing to save — for
//          kernels that run two waves per SIMD and have 256 registers (tot: one cell fills a CU's LDS anyway);
//   true   v64-71, v80-87, v96-103, v112-119: four caller-saved blocks again, for the kernel that runs more than two waves per
//          SIMD (gas; aer too while it was held to 128 registers); the functions' own values stay below v64 (the build checks it).  (Until round 2 this ring was v96-127: two of those blocks are callee-saved, every call
//          of gsum_run / tail_solve stored and reloaded 16 registers per lane — most of the aer kernel's HBM-side traffic.)
// Loads return in issue order, hence "at most PENDING outstanding" means the oldest one — the slot about to be
// consumed — has landed.  (An earlier version kept the ring in AGPRs: any AGPR use halves the compiler's VGPR budget
// on gfx950, which cost the kernel ~100 spilled registers.)
//
// The ring's sixteen slots of four registers, stated ONCE: slot K of the low (v64..) and of the high (v192..) placement.  (The
// generated streams name the same blocks: tools/gen_gsum_asm.py: SLOTS; tests/test_capi.py holds the two together.)
#define MISTRA_RING_LO0 64, 65, 66, 67
#define MISTRA_RING_LO1 68, 69, 70, 71
#define MISTRA_RING_LO2 80, 81, 82, 83
#define MISTRA_RING_LO3 84, 85, 86, 87
#define MISTRA_RING_LO4 96, 97, 98, 99
#define MISTRA_RING_LO5 100, 101, 102, 103
#define MISTRA_RING_LO6 112, 113, 114, 115
#define MISTRA_RING_LO7 116, 117, 118, 119
#define MISTRA_RING_HI0 192, 193, 194, 195
#define MISTRA_RING_HI1 196, 197, 198, 199
#define MISTRA_RING_HI2 208, 209, 210, 211
#define MISTRA_RING_HI3 212, 213, 214, 215
#define MISTRA_RING_HI4 224, 225, 226, 227
#define MISTRA_RING_HI5 228, 229, 230, 231
#define MISTRA_RING_HI6 240, 241, 242, 243
#define MISTRA_RING_HI7 244, 245, 246, 247
#define MISTRA_APPLY(M, ...) M(__VA_ARGS__)
// M(the four registers of slot K in placement LOW): K and LOW are the template parameters of the function it stands in
#define MISTRA_ON_RING_SLOT(M)                                                                                                 \
  static_assert(K >= 0 && K < kRingSlots, "ring slot");                                                                        \
  if constexpr (LOW) {                                                                                                         \
    if constexpr (K == 0) MISTRA_APPLY(M, MISTRA_RING_LO0);                                                                    \
    else if constexpr (K == 1) MISTRA_APPLY(M, MISTRA_RING_LO1);                                                               \
    else if constexpr (K == 2) MISTRA_APPLY(M, MISTRA_RING_LO2);                                                               \
    else if constexpr (K == 3) MISTRA_APPLY(M, MISTRA_RING_LO3);                                                               \
    else if constexpr (K == 4) MISTRA_APPLY(M, MISTRA_RING_LO4);                                                               \
    else if constexpr (K == 5) MISTRA_APPLY(M, MISTRA_RING_LO5);                                                               \
    else if constexpr (K == 6) MISTRA_APPLY(M, MISTRA_RING_LO6);                                                               \
    else MISTRA_APPLY(M, MISTRA_RING_LO7);                                                                                     \
  } else {                                                                                                                     \
    if constexpr (K == 0) MISTRA_APPLY(M, MISTRA_RING_HI0);                                                                    \
    else if constexpr (K == 1) MISTRA_APPLY(M, MISTRA_RING_HI1);                                                               \
    else if constexpr (K == 2) MISTRA_APPLY(M, MISTRA_RING_HI2);                                                               \
    else if constexpr (K == 3) MISTRA_APPLY(M, MISTRA_RING_HI3);                                                               \
    else if constexpr (K == 4) MISTRA_APPLY(M, MISTRA_RING_HI4);                                                               \
    else if constexpr (K == 5) MISTRA_APPLY(M, MISTRA_RING_HI5);                                                               \
    else if constexpr (K == 6) MISTRA_APPLY(M, MISTRA_RING_HI6);                                                               \
    else MISTRA_APPLY(M, MISTRA_RING_HI7);                                                                                     \
  }
// M(args, the sixteen registers of ring half H — slots 4H .. 4H + 3 — in table column order)
#define MISTRA_ON_RING_HALF(M, ...)                                                                                            \
  if constexpr (LOW && H == 0) MISTRA_APPLY(M, __VA_ARGS__, MISTRA_RING_LO0, MISTRA_RING_LO1, MISTRA_RING_LO2, MISTRA_RING_LO3); \
  else if constexpr (LOW) MISTRA_APPLY(M, __VA_ARGS__, MISTRA_RING_LO4, MISTRA_RING_LO5, MISTRA_RING_LO6, MISTRA_RING_LO7);    \
  else if constexpr (H == 0) MISTRA_APPLY(M, __VA_ARGS__, MISTRA_RING_HI0, MISTRA_RING_HI1, MISTRA_RING_HI2, MISTRA_RING_HI3); \
  else MISTRA_APPLY(M, __VA_ARGS__, MISTRA_RING_HI4, MISTRA_RING_HI5, MISTRA_RING_HI6, MISTRA_RING_HI7);

template <bool LOW, int K, int BYTE_OFFSET = 0>
__device__ __forceinline__ void vm_ring_load(gptr<u32x4> p) {
#define MISTRA_RING_LOAD(R0, R1, R2, R3)                                                                              \
  asm volatile("global_load_dwordx4 v[" #R0 ":" #R3 "], %0, off offset:%1" : : "v"(p), "n"(BYTE_OFFSET)             \
               : "memory", "v" #R0, "v" #R1, "v" #R2, "v" #R3)
  MISTRA_ON_RING_SLOT(MISTRA_RING_LOAD)
#undef MISTRA_RING_LOAD
}

// A table's base in scalar registers: the tail chain loads its rows through a scalar base and the lane's 32-bit byte offset in ONE
// vector register (vm_ring_load_at).  (With per-lane 64-bit pointers the compiler kept one 64-bit row offset per load in scalar
// registers — enough of them to reach the callee-saved ones, whose save area cost the tail chain a scratch store and reload per
// call: aer's last per-step HBM traffic.)
__device__ __forceinline__ uint64_t ring_base(const void* p) {
  const uint64_t u = (uint64_t)(uintptr_t)p;
  uint32_t lo, hi;
  // (a scalar register written by a vector instruction may not feed a memory instruction's address for 5 wait states, and the
  // compiler's hazard pass does not look inside the asm statements that issue the loads: the wait is spelled out here)
  asm volatile("v_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3\n\ts_nop 4" : "=s"(lo), "=s"(hi) : "v"((uint32_t)u), "v"((uint32_t)(u >> 32)));
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// The same load from such a base: the row's base handed over as it stands (a compile-time offset from a table's start: two scalar
// additions), IMM in the instruction's immediate offset (13 bits signed on gfx950)
template <bool LOW, int K, int IMM>
__device__ __forceinline__ void vm_ring_load_at(uint64_t sbase, uint32_t voff) {
  static_assert(IMM >= 0 && IMM < 4096, "13-bit signed immediate offset");
#define MISTRA_RING_LOAD_AT(R0, R1, R2, R3)                                                                                   \
  asm volatile("global_load_dwordx4 v[" #R0 ":" #R3 "], %0, %1 offset:%2" : : "v"(voff), "s"(sbase), "n"(IMM)                \
               : "memory", "v" #R0, "v" #R1, "v" #R2, "v" #R3)
  MISTRA_ON_RING_SLOT(MISTRA_RING_LOAD_AT)
#undef MISTRA_RING_LOAD_AT
}

template <bool LOW, int K, int PENDING = 7>
__device__ __forceinline__ u32x4 vm_ring_take() {
  uint32_t x, y, z, w;
#define MISTRA_RING_TAKE(R0, R1, R2, R3)                                                                              \
  asm volatile("s_waitcnt vmcnt(%4)\n\tv_mov_b32 %0, v" #R0 "\n\tv_mov_b32 %1, v" #R1                                   \
               "\n\tv_mov_b32 %2, v" #R2 "\n\tv_mov_b32 %3, v" #R3                                                    \
               : "=v"(x), "=v"(y), "=v"(z), "=v"(w) : "n"(PENDING) : "memory")
  MISTRA_ON_RING_SLOT(MISTRA_RING_TAKE)
#undef MISTRA_RING_TAKE
  return u32x4{x, y, z, w};
}
#undef MISTRA_ON_RING_SLOT
static_assert(kRingSlots == 8, "the ring table above has 8 slots per placement");

// ---- the LDS VM executor (schedule.hpp), hand-scheduled: one asm statement holds the whole program loop; its instruction
// stream is generated (tools/gen_vm_asm.py -> vm_exec_asm.inc, where the pipeline and the wait counts are explained).
//   * records land straight in VGPRs: a ring of four 8-register slots in caller-saved blocks (v48-55, v64-71, v80-87, v96-103), named only inside this statement, so no compiler copy can get between a load
//     and its counted wait (cdna_hip_programming.md §5.7); a slot is refilled (row + 4) behind its record's store;
//   * d0, d2..d7 of a record are LDS byte addresses as they stand (M starts at LDS address 0, checked at kernel entry);
//     every mark sits on d1: one v_readfirstlane per record, one scalar test for "any mark" on the main line;
//   * round 3: the six operand gathers of record S+1 are issued at the head of record S (two operand register sets), so a
//     lone wave no longer waits out an LDS round trip per record: measured ~250 cycles per record row before, the record's
//     own instruction issue now.  The arithmetic and its order are unchanged (bit-identical results);
//   * marked rows (aux operand: scale by a pivot reciprocal, or publish one; end of round; null rows) run out of line.
// A continuation record reloads its target: its lane's previous record stored it, and LDS is in-order within a wave.
// The IEEE reciprocal is the sequence hipcc emits for 1.0/x (v_div_scale, v_rcp, two Newton steps, v_div_fmas, v_div_fixup).
#include "vm_exec_asm.inc"

// UPR: updates per record — 2: (a, r, u) triples, the LU program; 3: (a, u) pairs, the triangular sweeps (schedule.hpp)
// BARRIER: the call stands in place of lds_barrier() + vm_run(): the barrier sits between the ring fill and the first counted wait
// (table loads do not depend on LDS, the first record's gathers stay behind the barrier)
template <int NT, int SLOTS, int UPR = 2, bool BARRIER = false>
__device__ __attribute__((noinline)) void vm_run(const VmDev P, uint32_t row0, int lane) {
  static_assert(SLOTS == 4 && (UPR == 2 || UPR == 3), "ring depth and executor variants vm_exec_asm.inc is generated for");
  static_assert(!BARRIER || UPR == 3, "the barrier form is generated for the sweep programs");
  const uint64_t recs = reinterpret_cast<uint64_t>(P.recs);      // the same in every lane: move it to SGPRs
  const uint64_t base = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)recs) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(recs >> 32)) << 32);
  // row0: the wave's first record row (P.wave_base[wave]; the kernel fetched it when it started — read here it was a memory round
  // trip in front of the first table load, on every call)
  uint32_t va = row0 * 2048u + (uint32_t)lane * 16u;     // this lane's first record (planar rows: lo plane, hi plane + 1024), bytes
  uint32_t vb = va + 4096u;                                                          // rows +2, +3
  int rounds = __builtin_amdgcn_readfirstlane(P.nrounds);
  double acc, a1A, r1A, u1A, a2A, r2A, u2A, a1B, r1B, u1B, a2B, r2B, u2B, sc;
  uint32_t tg, ax, t, flA, flB, tmp;
  uint64_t sv, sm;
#define MISTRA_VM_OPERANDS                                                                                                                             \
  [acc] "=&v"(acc), [a1A] "=&v"(a1A), [r1A] "=&v"(r1A), [u1A] "=&v"(u1A), [a2A] "=&v"(a2A), [r2A] "=&v"(r2A), [u2A] "=&v"(u2A), [a1B] "=&v"(a1B),      \
      [r1B] "=&v"(r1B), [u1B] "=&v"(u1B), [a2B] "=&v"(a2B), [r2B] "=&v"(r2B), [u2B] "=&v"(u2B), [sc] "=&v"(sc), [tg] "=&v"(tg), [ax] "=&v"(ax),          \
      [t] "=&v"(t), [flA] "=&s"(flA), [flB] "=&s"(flB), [tmp] "=&s"(tmp), [sv] "=&s"(sv), [sm] "=&s"(sm), [rounds] "+s"(rounds), [va] "+v"(va),         \
      [vb] "+v"(vb)
  if constexpr (BARRIER) {
    asm volatile(MISTRA_VM_ASM_N4_SWEEP_BAR : MISTRA_VM_OPERANDS : [base] "s"(base) : "memory", "vcc", "scc", MISTRA_VM_CLOBBER_N4);
  } else if constexpr (UPR == 3) {
    asm volatile(MISTRA_VM_ASM_N4_SWEEP : MISTRA_VM_OPERANDS : [base] "s"(base) : "memory", "vcc", "scc", MISTRA_VM_CLOBBER_N4);
  } else {
    asm volatile(MISTRA_VM_ASM_N4 : MISTRA_VM_OPERANDS : [base] "s"(base) : "memory", "vcc", "scc", MISTRA_VM_CLOBBER_N4);
  }
#undef MISTRA_VM_OPERANDS
}

// ---- tail chain of the triangular solves (schedule.hpp: TailSolve), run by ONE wave: lane l holds rows h+l and h+64+l of the
//      solution in registers (x[0], x[1]); lane row r (16 lanes) of register q = 16x16 block row 4q + r of the tail triangle.
//      Matrix entries are gathered from LDS through per-column index tables streamed through the look-ahead ring (one 16-byte
//      slot = 4 columns, a 16-column block = 4 slots; the backward tables follow the forward ones through the same ring, so the
//      stream is primed once per solve).  Per block column J (forward; backward runs the blocks and the columns the other way):
//        1. the block's own 16 unknowns, in their lane row: x(i) -= L(i,j) x(j), j ascending — the pivot value reaches the other
//           lanes of its lane row inside the multiply-add itself (DPP row_newbcast on v_fmac_f64: measured 10 cycles per dependent
//           step with one wait state, 14 with the two the ISA manual asks for; the v_readlane -> SGPR -> VALU round trip that all
//           columns but the dense block's forward ones took until round 3 costs ~57);
//        2. the 16 finished values go to all four lane rows (gfx950 v_permlane16_swap / v_permlane32_swap);
//        3. the rows below take their 16 terms, j ascending, again by DPP: the lane rows below in the same register, and every
//           lane row of the other register.
//      Every row still receives its terms in ascending (backward: descending) column order with the operands and the fused
//      multiply-add of the column-by-column chain the emulator states (tests/emu/schedule_emu.cpp): the results are bit-identical.
//      Operands that are not in the pattern (and every diagonal) point at the 0.0 cell.
template <int ROW>
__device__ __forceinline__ double lane_row_to_all(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
  // permlane16_swap(a, b): a.row1 <-> b.row0, a.row3 <-> b.row2.   From a = b = v: a = [v0 v0 v2 v2], b = [v1 v1 v3 v3]
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const uint32_t a = l16[ROW & 1], b = h16[ROW & 1];
  // permlane32_swap(a, b): a.upper32 <-> b.lower32.   From a = b: a = [lower lower], b = [upper upper]
  const auto l32 = __builtin_amdgcn_permlane32_swap(a, a, false, false);
  const auto h32 = __builtin_amdgcn_permlane32_swap(b, b, false, false);
  return __builtin_bit_cast(double, (uint64_t)l32[(ROW >> 1) & 1] | ((uint64_t)h32[(ROW >> 1) & 1] << 32));
}
// The phases are ONE asm statement each: between separate statements the compiler adds wait states of its own.  Step j of the
// diagonal block needs no lane selection: every operand that is not a strictly-lower (forward) / strictly-upper (backward) entry of
// the block points at the 0.0 cell, so the lanes i <= j (i >= j) of the lane row add an exact zero, as the column-by-column chain
// of the emulator does; row_mask confines the writes to the block's lane row.  The DPP read of the value the previous step wrote
// needs two wait states, the hardware does not interlock it (tools/ubench/dpp.hip: 10 cycles per dependent step with one, wrong
// with none).
#define MISTRA_TAIL_COPS                                                                                                          \
  [c0] "v"(c[0]), [c1] "v"(c[1]), [c2] "v"(c[2]), [c3] "v"(c[3]), [c4] "v"(c[4]), [c5] "v"(c[5]), [c6] "v"(c[6]), [c7] "v"(c[7]),     \
      [c8] "v"(c[8]), [c9] "v"(c[9]), [c10] "v"(c[10]), [c11] "v"(c[11]), [c12] "v"(c[12]), [c13] "v"(c[13]), [c14] "v"(c[14]), [c15] "v"(c[15])
#define MISTRA_DIAG_STEP(J, RM) "s_nop 1\n\tv_fmac_f64_dpp %[x], -%[x], %[c" #J "] row_newbcast:" #J " row_mask:" RM " bank_mask:0xf\n\t"
#define MISTRA_DIAG_FWD(RM)                                                                                                     \
  asm volatile(MISTRA_DIAG_STEP(0, RM) MISTRA_DIAG_STEP(1, RM) MISTRA_DIAG_STEP(2, RM) MISTRA_DIAG_STEP(3, RM) MISTRA_DIAG_STEP(4, RM)   \
               MISTRA_DIAG_STEP(5, RM) MISTRA_DIAG_STEP(6, RM) MISTRA_DIAG_STEP(7, RM) MISTRA_DIAG_STEP(8, RM) MISTRA_DIAG_STEP(9, RM)   \
               MISTRA_DIAG_STEP(10, RM) MISTRA_DIAG_STEP(11, RM) MISTRA_DIAG_STEP(12, RM) MISTRA_DIAG_STEP(13, RM) MISTRA_DIAG_STEP(14, RM) \
               "s_nop 0"                                                                                                        \
               : [x] "+v"(x) : MISTRA_TAIL_COPS)
#define MISTRA_DIAG_BWD(RM)                                                                                                     \
  asm volatile(MISTRA_DIAG_STEP(15, RM) MISTRA_DIAG_STEP(14, RM) MISTRA_DIAG_STEP(13, RM) MISTRA_DIAG_STEP(12, RM) MISTRA_DIAG_STEP(11, RM) \
               MISTRA_DIAG_STEP(10, RM) MISTRA_DIAG_STEP(9, RM) MISTRA_DIAG_STEP(8, RM) MISTRA_DIAG_STEP(7, RM) MISTRA_DIAG_STEP(6, RM)     \
               MISTRA_DIAG_STEP(5, RM) MISTRA_DIAG_STEP(4, RM) MISTRA_DIAG_STEP(3, RM) MISTRA_DIAG_STEP(2, RM) MISTRA_DIAG_STEP(1, RM)      \
               "s_nop 0"                                                                                                        \
               : [x] "+v"(x) : MISTRA_TAIL_COPS)
#define MISTRA_UPD_STEP(J, ROWMASK) "v_fmac_f64_dpp %[x], -%[xb], %[c" #J "] row_newbcast:" #J " row_mask:" ROWMASK " bank_mask:0xf\n\t"
#define MISTRA_UPDATE_FWD(ROWMASK)                                                                                             \
  asm volatile("s_nop 1\n\t"                                                                                                   \
               MISTRA_UPD_STEP(0, ROWMASK) MISTRA_UPD_STEP(1, ROWMASK) MISTRA_UPD_STEP(2, ROWMASK) MISTRA_UPD_STEP(3, ROWMASK)   \
               MISTRA_UPD_STEP(4, ROWMASK) MISTRA_UPD_STEP(5, ROWMASK) MISTRA_UPD_STEP(6, ROWMASK) MISTRA_UPD_STEP(7, ROWMASK)   \
               MISTRA_UPD_STEP(8, ROWMASK) MISTRA_UPD_STEP(9, ROWMASK) MISTRA_UPD_STEP(10, ROWMASK) MISTRA_UPD_STEP(11, ROWMASK) \
               MISTRA_UPD_STEP(12, ROWMASK) MISTRA_UPD_STEP(13, ROWMASK) MISTRA_UPD_STEP(14, ROWMASK)                            \
               "v_fmac_f64_dpp %[x], -%[xb], %[c15] row_newbcast:15 row_mask:" ROWMASK " bank_mask:0xf"                         \
               : [x] "+v"(x) : [xb] "v"(xb), MISTRA_TAIL_COPS)
#define MISTRA_UPDATE_BWD(ROWMASK)                                                                                             \
  asm volatile("s_nop 1\n\t"                                                                                                   \
               MISTRA_UPD_STEP(15, ROWMASK) MISTRA_UPD_STEP(14, ROWMASK) MISTRA_UPD_STEP(13, ROWMASK) MISTRA_UPD_STEP(12, ROWMASK) \
               MISTRA_UPD_STEP(11, ROWMASK) MISTRA_UPD_STEP(10, ROWMASK) MISTRA_UPD_STEP(9, ROWMASK) MISTRA_UPD_STEP(8, ROWMASK)   \
               MISTRA_UPD_STEP(7, ROWMASK) MISTRA_UPD_STEP(6, ROWMASK) MISTRA_UPD_STEP(5, ROWMASK) MISTRA_UPD_STEP(4, ROWMASK)     \
               MISTRA_UPD_STEP(3, ROWMASK) MISTRA_UPD_STEP(2, ROWMASK) MISTRA_UPD_STEP(1, ROWMASK)                                 \
               "v_fmac_f64_dpp %[x], -%[xb], %[c0] row_newbcast:0 row_mask:" ROWMASK " bank_mask:0xf"                           \
               : [x] "+v"(x) : [xb] "v"(xb), MISTRA_TAIL_COPS)

// step 1 of a block column for the lane row ROW of x
template <int ROW, bool BACKWARD>
__device__ __forceinline__ void tail_diag(double& x, const double (&c)[16]) {
  if constexpr (!BACKWARD) {
    if constexpr (ROW == 0) MISTRA_DIAG_FWD("0x1");
    else if constexpr (ROW == 1) MISTRA_DIAG_FWD("0x2");
    else if constexpr (ROW == 2) MISTRA_DIAG_FWD("0x4");
    else MISTRA_DIAG_FWD("0x8");
  } else {
    if constexpr (ROW == 0) MISTRA_DIAG_BWD("0x1");
    else if constexpr (ROW == 1) MISTRA_DIAG_BWD("0x2");
    else if constexpr (ROW == 2) MISTRA_DIAG_BWD("0x4");
    else MISTRA_DIAG_BWD("0x8");
  }
}
// step 3: the lane rows selected by MASK (a 4-bit row mask) take the block column's 16 terms from the broadcast values xb
template <int MASK, bool BACKWARD>
__device__ __forceinline__ void tail_update(double& x, const double xb, const double (&c)[16]) {
  static_assert(MASK >= 1 && MASK <= 15, "row mask");
#define MISTRA_UPD_CASE(M, S) else if constexpr (MASK == M) { if constexpr (BACKWARD) MISTRA_UPDATE_BWD(S); else MISTRA_UPDATE_FWD(S); }
  if constexpr (MASK == 15) { if constexpr (BACKWARD) MISTRA_UPDATE_BWD("0xf"); else MISTRA_UPDATE_FWD("0xf"); }
  MISTRA_UPD_CASE(14, "0xe") MISTRA_UPD_CASE(12, "0xc") MISTRA_UPD_CASE(8, "0x8") MISTRA_UPD_CASE(1, "0x1") MISTRA_UPD_CASE(3, "0x3") MISTRA_UPD_CASE(7, "0x7")
  else static_assert(MASK == 15, "row mask not instantiated");
#undef MISTRA_UPD_CASE
}
// The same phases with the gathers of one ring group (the 16 operand addresses of one register's rows in one block, table column
// order, in four ring slots) issued inside them: straight from the ring registers, whose words are LDS byte addresses
// (schedule.hpp: TailSolve::fwd_addr / bwd_addr), into g.  The compiler does not know the ring, nor that the loads are in flight:
// each statement waits for its group's table loads first (vmcnt(4): the group after it is the only one issued since, see
// tail_solve) and for its own gathers last (lgkmcnt(0); cdna_hip_programming.md §5.7), and g are early-clobber outputs.  In the
// diagonal steps the gathers take the wait slots, two per slot (an instruction is a wait state); in the 16-step update of the other
// register two precede each of the first eight steps, the last eight cover the LDS round trip.  (The diagonal steps are the 15 of
// tail_diag: the block's last column has no rows below it in the block, forward, nor its first above, backward; the closing
// s_waitcnt is the wait state tail_diag's trailing s_nop 0 gives.)
#define MISTRA_TAIL_GOPS                                                                                                          \
  [g0] "=&v"(g[0]), [g1] "=&v"(g[1]), [g2] "=&v"(g[2]), [g3] "=&v"(g[3]), [g4] "=&v"(g[4]), [g5] "=&v"(g[5]), [g6] "=&v"(g[6]),           \
      [g7] "=&v"(g[7]), [g8] "=&v"(g[8]), [g9] "=&v"(g[9]), [g10] "=&v"(g[10]), [g11] "=&v"(g[11]), [g12] "=&v"(g[12]),                   \
      [g13] "=&v"(g[13]), [g14] "=&v"(g[14]), [g15] "=&v"(g[15])
#define MISTRA_G2(A, RA, B, RB) "ds_read_b64 %[g" #A "], v" #RA "\n\tds_read_b64 %[g" #B "], v" #RB "\n\t"
#define MISTRA_G16(r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)                                        \
  MISTRA_G2(0, r0, 1, r1) MISTRA_G2(2, r2, 3, r3) MISTRA_G2(4, r4, 5, r5) MISTRA_G2(6, r6, 7, r7) MISTRA_G2(8, r8, 9, r9)       \
      MISTRA_G2(10, r10, 11, r11) MISTRA_G2(12, r12, 13, r13) MISTRA_G2(14, r14, 15, r15)
#define MISTRA_DSTEP(J, RM) "v_fmac_f64_dpp %[x], -%[x], %[c" #J "] row_newbcast:" #J " row_mask:" RM " bank_mask:0xf\n\t"
#define MISTRA_NSTEP(J, RM) "s_nop 1\n\t" MISTRA_DSTEP(J, RM)
#define MISTRA_DIAG_G_FWD(RM, r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)                               \
  asm volatile("s_waitcnt vmcnt(4)\n\t"                                                                                       \
               MISTRA_G2(0, r0, 1, r1) MISTRA_DSTEP(0, RM) MISTRA_G2(2, r2, 3, r3) MISTRA_DSTEP(1, RM)                        \
               MISTRA_G2(4, r4, 5, r5) MISTRA_DSTEP(2, RM) MISTRA_G2(6, r6, 7, r7) MISTRA_DSTEP(3, RM)                        \
               MISTRA_G2(8, r8, 9, r9) MISTRA_DSTEP(4, RM) MISTRA_G2(10, r10, 11, r11) MISTRA_DSTEP(5, RM)                    \
               MISTRA_G2(12, r12, 13, r13) MISTRA_DSTEP(6, RM) MISTRA_G2(14, r14, 15, r15) MISTRA_DSTEP(7, RM)                \
               MISTRA_NSTEP(8, RM) MISTRA_NSTEP(9, RM) MISTRA_NSTEP(10, RM) MISTRA_NSTEP(11, RM) MISTRA_NSTEP(12, RM)         \
               MISTRA_NSTEP(13, RM) MISTRA_NSTEP(14, RM) "s_waitcnt lgkmcnt(0)"              \
               : [x] "+v"(x), MISTRA_TAIL_GOPS : MISTRA_TAIL_COPS : "memory")
#define MISTRA_DIAG_G_BWD(RM, r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)                               \
  asm volatile("s_waitcnt vmcnt(4)\n\t"                                                                                       \
               MISTRA_G2(0, r0, 1, r1) MISTRA_DSTEP(15, RM) MISTRA_G2(2, r2, 3, r3) MISTRA_DSTEP(14, RM)                      \
               MISTRA_G2(4, r4, 5, r5) MISTRA_DSTEP(13, RM) MISTRA_G2(6, r6, 7, r7) MISTRA_DSTEP(12, RM)                      \
               MISTRA_G2(8, r8, 9, r9) MISTRA_DSTEP(11, RM) MISTRA_G2(10, r10, 11, r11) MISTRA_DSTEP(10, RM)                  \
               MISTRA_G2(12, r12, 13, r13) MISTRA_DSTEP(9, RM) MISTRA_G2(14, r14, 15, r15) MISTRA_DSTEP(8, RM)                \
               MISTRA_NSTEP(7, RM) MISTRA_NSTEP(6, RM) MISTRA_NSTEP(5, RM) MISTRA_NSTEP(4, RM) MISTRA_NSTEP(3, RM)            \
               MISTRA_NSTEP(2, RM) MISTRA_NSTEP(1, RM) "s_waitcnt lgkmcnt(0)"                 \
               : [x] "+v"(x), MISTRA_TAIL_GOPS : MISTRA_TAIL_COPS : "memory")
#define MISTRA_USTEP(J) "v_fmac_f64_dpp %[x], -%[xb], %[c" #J "] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define MISTRA_UPDATE_G_FWD(UNUSED, r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)                                 \
  asm volatile("s_waitcnt vmcnt(4)\n\t"                                                                                       \
               MISTRA_G2(0, r0, 1, r1) MISTRA_USTEP(0) MISTRA_G2(2, r2, 3, r3) MISTRA_USTEP(1)                                \
               MISTRA_G2(4, r4, 5, r5) MISTRA_USTEP(2) MISTRA_G2(6, r6, 7, r7) MISTRA_USTEP(3)                                \
               MISTRA_G2(8, r8, 9, r9) MISTRA_USTEP(4) MISTRA_G2(10, r10, 11, r11) MISTRA_USTEP(5)                            \
               MISTRA_G2(12, r12, 13, r13) MISTRA_USTEP(6) MISTRA_G2(14, r14, 15, r15) MISTRA_USTEP(7)                        \
               MISTRA_USTEP(8) MISTRA_USTEP(9) MISTRA_USTEP(10) MISTRA_USTEP(11) MISTRA_USTEP(12) MISTRA_USTEP(13)            \
               MISTRA_USTEP(14) MISTRA_USTEP(15) "s_waitcnt lgkmcnt(0)"                                                       \
               : [x] "+v"(x), MISTRA_TAIL_GOPS : [xb] "v"(xb), MISTRA_TAIL_COPS : "memory")
#define MISTRA_UPDATE_G_BWD(UNUSED, r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)                                 \
  asm volatile("s_waitcnt vmcnt(4)\n\t"                                                                                       \
               MISTRA_G2(0, r0, 1, r1) MISTRA_USTEP(15) MISTRA_G2(2, r2, 3, r3) MISTRA_USTEP(14)                              \
               MISTRA_G2(4, r4, 5, r5) MISTRA_USTEP(13) MISTRA_G2(6, r6, 7, r7) MISTRA_USTEP(12)                              \
               MISTRA_G2(8, r8, 9, r9) MISTRA_USTEP(11) MISTRA_G2(10, r10, 11, r11) MISTRA_USTEP(10)                          \
               MISTRA_G2(12, r12, 13, r13) MISTRA_USTEP(9) MISTRA_G2(14, r14, 15, r15) MISTRA_USTEP(8)                        \
               MISTRA_USTEP(7) MISTRA_USTEP(6) MISTRA_USTEP(5) MISTRA_USTEP(4) MISTRA_USTEP(3) MISTRA_USTEP(2)                \
               MISTRA_USTEP(1) MISTRA_USTEP(0) "s_waitcnt lgkmcnt(0)"                                                         \
               : [x] "+v"(x), MISTRA_TAIL_GOPS : [xb] "v"(xb), MISTRA_TAIL_COPS : "memory")
#define MISTRA_GATHER_ONLY(UNUSED, r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)                                  \
  asm volatile("s_waitcnt vmcnt(4)\n\t" MISTRA_G16(r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15)       \
               "s_waitcnt lgkmcnt(0)" : MISTRA_TAIL_GOPS : : "memory")

// step 1 with the gathers of ring half H
template <bool LOW, int H, int ROW, bool BACKWARD>
__device__ __forceinline__ void tail_diag_gather(double& x, const double (&c)[16], double (&g)[16]) {
  if constexpr (!BACKWARD) {
    if constexpr (ROW == 0) { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_FWD, "0x1") }
    else if constexpr (ROW == 1) { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_FWD, "0x2") }
    else if constexpr (ROW == 2) { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_FWD, "0x4") }
    else { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_FWD, "0x8") }
  } else {
    if constexpr (ROW == 0) { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_BWD, "0x1") }
    else if constexpr (ROW == 1) { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_BWD, "0x2") }
    else if constexpr (ROW == 2) { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_BWD, "0x4") }
    else { MISTRA_ON_RING_HALF(MISTRA_DIAG_G_BWD, "0x8") }
  }
}
// step 3 for all four lane rows of the other register, with the gathers of ring half H
template <bool LOW, int H, bool BACKWARD>
__device__ __forceinline__ void tail_update_gather(double& x, const double xb, const double (&c)[16], double (&g)[16]) {
  if constexpr (BACKWARD) { MISTRA_ON_RING_HALF(MISTRA_UPDATE_G_BWD, 0) }
  else { MISTRA_ON_RING_HALF(MISTRA_UPDATE_G_FWD, 0) }
}
// the gathers of ring half H alone (a block with nothing left to host them)
template <bool LOW, int H>
__device__ __forceinline__ void tail_gather(double (&g)[16]) {
  MISTRA_ON_RING_HALF(MISTRA_GATHER_ONLY, 0)
}
#undef MISTRA_TAIL_GOPS
#undef MISTRA_ON_RING_HALF
#undef MISTRA_APPLY
#undef MISTRA_G2
#undef MISTRA_G16
#undef MISTRA_DSTEP
#undef MISTRA_NSTEP
#undef MISTRA_DIAG_G_FWD
#undef MISTRA_DIAG_G_BWD
#undef MISTRA_USTEP
#undef MISTRA_UPDATE_G_FWD
#undef MISTRA_UPDATE_G_BWD
#undef MISTRA_GATHER_ONLY
#undef MISTRA_DIAG_STEP
#undef MISTRA_DIAG_FWD
#undef MISTRA_DIAG_BWD
#undef MISTRA_UPD_STEP
#undef MISTRA_UPDATE_FWD
#undef MISTRA_UPDATE_BWD
#undef MISTRA_TAIL_COPS

// The block stream of one solve (forward blocks from FWD_BLOCK0 on, then every block backward) and the groups it reads from the
// look-ahead ring: per block its own register's 16 operand addresses and, where the other register takes part, that register's
// 16 — one group of four ring slots each, in the order the chain gathers them (own(0); other(0), own(1); ...).  Group g lands in
// ring half g & 1; once it is gathered its half is refilled with group g + 2, so every gathering statement waits for vmcnt(4).
template <int R, int FWD_BLOCK0>
struct TailStream {
  static constexpr int NB = 4 * R;               // 16-column blocks of the tail triangle
  static constexpr int NF = NB - FWD_BLOCK0;     // ... of them in the forward chain
  static constexpr int NS = NF + NB;             // blocks of the whole solve, forward then backward
  static constexpr bool bw(int s) { return s >= NF; }
  static constexpr int col_block(int s) { return bw(s) ? NB - 1 - (s - NF) : FWD_BLOCK0 + s; }
  static constexpr bool last(int s) { return bw(s) ? s == NS - 1 : FWD_BLOCK0 + s == NB - 1; }
  static constexpr int reg(int s) { return col_block(s) / 4; }
  static constexpr int other(int s) { return bw(s) ? 0 : R - 1; }     // the other register's rows lie wholly below (forward) / above (backward) the block
  static constexpr bool has_other(int s) { return !last(s) && R == 2 && reg(s) != other(s); }
  static constexpr int own_group(int s) {
    int g = 0;
    for (int i = 0; i < s && i < NS; i++) g += has_other(i) ? 2 : 1;
    return g;
  }
  static constexpr int NG = own_group(NS);
  static constexpr int group_block(int g) {
    int s = 0;
    while (s + 1 < NS && own_group(s + 1) <= g) s++;
    return s;
  }
  static constexpr int group_reg(int g) { return g == own_group(group_block(g)) ? reg(group_block(g)) : other(group_block(g)); }
};

// One block column, in two halves so that the operand gathers of block b + 1 are in flight while block b computes (a lone wave
// would otherwise sit out an LDS round trip in front of every block: measured, the chain then took as long as the column-by-column
// one).  c: the block's own operands in chain order (step j: table column j forward, 15 - j backward), gathered by the previous
// block.  Where the other register takes part, its operands are gathered in the wait slots of the diagonal steps, and the next
// block's own ones inside the other register's 16-step update.  Elsewhere the next block's own operands take the diagonal steps'
// wait slots — except in the low ring placement, whose functions stay below v64 and cannot hold two operand sets at once: there
// they are gathered on their own once the block's last use of c is issued (an exposed LDS round trip per block).
// load(g): refills the ring half of group g - 2, just gathered, with group g.
template <class TS, int S, bool LOW, int R, class LOAD>
__device__ __forceinline__ void tail_block(double (&xr)[R], double (&c)[16], LOAD&& load) {
  constexpr int J = TS::col_block(S), REG = J / 4, ROW = J % 4, OTHER = TS::other(S);
  constexpr bool BACKWARD = TS::bw(S), LAST = TS::last(S), HAS_OTHER = TS::has_other(S), NEXT = S + 1 < TS::NS;
  constexpr int GO = TS::own_group(S) + 1, GN = TS::own_group(S + 1);     // groups: the other register's operands, the next block's own
  constexpr bool DIAG_NEXT = !HAS_OTHER && NEXT && !LOW;                   // the next block's own operands gathered in the diagonal steps
  double x = xr[REG];
  double g[16], d[16];
  if constexpr (HAS_OTHER) {
    tail_diag_gather<LOW, GO & 1, ROW, BACKWARD>(x, c, g);               // 1. (and the other register's operands)
    load(std::integral_constant<int, GO + 2>());
#pragma unroll
    for (int j = 0; j < 16; j++) d[j] = g[BACKWARD ? 15 - j : j];
  } else if constexpr (DIAG_NEXT) {
    tail_diag_gather<LOW, GN & 1, ROW, BACKWARD>(x, c, g);               // 1. (and the next block's operands)
    load(std::integral_constant<int, GN + 2>());
  } else {
    tail_diag<ROW, BACKWARD>(x, c);                                      // 1.
  }
  if constexpr (!LAST) {
    const double xb = lane_row_to_all<ROW>(x);                           // 2.
    constexpr int same = BACKWARD ? (1 << ROW) - 1 : (0xF << (ROW + 1)) & 0xF;      // 3. lane rows above / below in the same register
    if constexpr (same != 0) tail_update<same, BACKWARD>(x, xb, c);
    xr[REG] = x;
    if constexpr (HAS_OTHER) {
      double y = xr[OTHER];
      tail_update_gather<LOW, GN & 1, BACKWARD>(y, xb, d, g);          // 3. for the other register (and the next block's operands)
      xr[OTHER] = y;
      load(std::integral_constant<int, GN + 2>());
    } else if constexpr (!DIAG_NEXT) {
      tail_gather<LOW, GN & 1>(g);
      load(std::integral_constant<int, GN + 2>());
    }
  } else {
    xr[REG] = x;
    if constexpr (NEXT && !DIAG_NEXT) {
      tail_gather<LOW, GN & 1>(g);
      load(std::integral_constant<int, GN + 2>());
    }
  }
  if constexpr (NEXT) {
#pragma unroll
    for (int j = 0; j < 16; j++) c[j] = g[TS::bw(S + 1) ? 15 - j : j];
  }
}

// FWD_BLOCK0: first 16-column block of the forward chain.  0: the whole forward chain; 4R: none (the vector has been
// forward-swept already — stage 1, inside the LU program); 4 of R = 2 with the dense tail block: only the block's own columns,
// whose rows the LU program leaves without exactly those terms (schedule.cpp: lu_entries, dense_h)
template <int R, int FWD_BLOCK0, bool LOW>
__device__ __attribute__((noinline)) void tail_solve(const TailDev T, uint32_t xb, uint32_t rb, int lane) {
  using TS = TailStream<R, FWD_BLOCK0>;
  static_assert(FWD_BLOCK0 >= 0 && FWD_BLOCK0 <= TS::NB && TS::NS <= 16, "first forward block");
  double x[R], rd[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    x[r] = lds_ld(xb + 8 * (r * 64 + lane));
    rd[r] = lds_ld(rb + 8 * (r * 64 + lane));          // R(k) = 1/U(k,k), published by the LU program
  }
  // table rows: one u32x4 per lane and group of 4 columns, 1 KiB per row, 4 rows per block; past the stream's last group: the
  // backward tables' slack rows.  Table bases in scalar registers, the lane's offset in one vector register.
  uint64_t tf[R], tb[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    tf[r] = ring_base(T.fwd_addr[r]);
    tb[r] = ring_base(T.bwd_addr[r]);
  }
  const uint32_t voff = 16u * (uint32_t)lane;
  auto load = [&](auto group) {
    constexpr int G = decltype(group)::value, K0 = 4 * (G & 1);
    uint64_t base;
    if constexpr (G < TS::NG) {
      constexpr int s = TS::group_block(G), r = TS::group_reg(G);
      base = TS::bw(s) ? tb[r] + (uint64_t)(s - TS::NF) * 4096u : tf[r] + (uint64_t)TS::col_block(s) * 4096u;
    } else {
      base = tb[0] + (uint64_t)(TS::NB + G - TS::NG) * 4096u;
    }
    vm_ring_load_at<LOW, K0, 0>(base, voff); vm_ring_load_at<LOW, K0 + 1, 1024>(base, voff);
    vm_ring_load_at<LOW, K0 + 2, 2048>(base, voff); vm_ring_load_at<LOW, K0 + 3, 3072>(base, voff);
  };
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");     // nothing of the caller's may sit between the counted loads
  load(std::integral_constant<int, 0>());
  load(std::integral_constant<int, 1>());
  double c[16];
  {
    double g[16];
    tail_gather<LOW, 0>(g);
    load(std::integral_constant<int, 2>());
#pragma unroll
    for (int j = 0; j < 16; j++) c[j] = g[TS::bw(0) ? 15 - j : j];
  }
  // the blocks; between the forward and the backward half: x = R .* x (the backward half runs on the row-scaled triangle
  // U' = D^-1 U that the factorisation leaves in the tail block — schedule.cpp: lu_entries; dense_lu — so there is no quotient
  // on the serial chain)
#define MISTRA_TAIL_STEP(S)                                                                                               \
  if constexpr ((S) < TS::NS) {                                                                                          \
    if constexpr ((S) == TS::NF) {                                                                                       \
      _Pragma("unroll") for (int r = 0; r < R; r++) x[r] = x[r] * rd[r];                                                 \
    }                                                                                                                    \
    tail_block<TS, (S), LOW>(x, c, load);                                                                                \
  }
  MISTRA_TAIL_STEP(0) MISTRA_TAIL_STEP(1) MISTRA_TAIL_STEP(2) MISTRA_TAIL_STEP(3) MISTRA_TAIL_STEP(4) MISTRA_TAIL_STEP(5) MISTRA_TAIL_STEP(6) MISTRA_TAIL_STEP(7)
  MISTRA_TAIL_STEP(8) MISTRA_TAIL_STEP(9) MISTRA_TAIL_STEP(10) MISTRA_TAIL_STEP(11) MISTRA_TAIL_STEP(12) MISTRA_TAIL_STEP(13) MISTRA_TAIL_STEP(14) MISTRA_TAIL_STEP(15)
#undef MISTRA_TAIL_STEP
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");     // the look-ahead loads past the stream's end have landed
#pragma unroll
  for (int r = 0; r < R; r++) lds_st(xb + 8 * (r * 64 + lane), x[r]);
}

// ---- the gather-sum machine (schedule.hpp): out = c0*M[i0] + c1*M[i1] + ...  left to right, four terms per table row,
//      rows streamed through the look-ahead ring (4 rows in flight).  acc starts at -0.0 and padding terms are
//      (-0.0f)*(0.0 cell), so terms need no flags and the sums are bit-for-bit the flagged ones.  A row whose first
//      address carries GS_ROW_FLUSH completes the lane's current output: it is stored to the lane's next output cell in
//      LDS (out_addr, then every out_stride bytes) — the caller reads its own cells back, no barrier needed.
//      The instruction stream is generated (tools/gen_gsum_asm.py -> gsum_exec_asm.inc: why, and the pipeline, are described there).
#include "gsum_exec_asm.inc"
// the wave's first row of program P (2 KiB per row), in scalar registers
__device__ __forceinline__ uint64_t gsum_base(const GsDev P, uint32_t row0) {
  const uint64_t recs = reinterpret_cast<uint64_t>(P.recs) + (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)row0) * 2048u;
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)recs) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(recs >> 32)) << 32);
}
template <int NT, bool LOW>
__device__ __attribute__((noinline)) void gsum_run(const GsDev P, uint32_t row0, int rows, int lane, uint32_t out_addr, uint32_t out_stride) {
  // row0, rows: P.wave_base[wave] and P.rows[wave], fetched by the kernel when it started (see vm_run)
  int n = __builtin_amdgcn_readfirstlane(rows);
  const uint64_t recs = reinterpret_cast<uint64_t>(P.recs) + (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)row0) * 2048u;      // the wave's first row: 2 KiB per row
  const uint64_t b0 = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)recs) |
                      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(recs >> 32)) << 32);
  const uint64_t b1 = b0 + 4096u;
  uint32_t voff = (uint32_t)lane * 32u;      // two uint4 per lane and row: addresses, coefficients
  double acc = -0.0;
  const double mzero = -0.0;
  double xA0, xA1, xA2, xA3, xB0, xB1, xB2, xB3, cA0, cA1, cA2, cA3, cB0, cB1, cB2, cB3;
  uint32_t ad, flA, flB;
#define MISTRA_GSUM_OPERANDS                                                                                                                   \
  [acc] "+&v"(acc), [ad] "=&v"(ad), [xA0] "=&v"(xA0), [xA1] "=&v"(xA1), [xA2] "=&v"(xA2), [xA3] "=&v"(xA3), [xB0] "=&v"(xB0), [xB1] "=&v"(xB1),    \
      [xB2] "=&v"(xB2), [xB3] "=&v"(xB3), [cA0] "=&v"(cA0), [cA1] "=&v"(cA1), [cA2] "=&v"(cA2), [cA3] "=&v"(cA3), [cB0] "=&v"(cB0),               \
      [cB1] "=&v"(cB1), [cB2] "=&v"(cB2), [cB3] "=&v"(cB3), [flA] "=&s"(flA), [flB] "=&s"(flB), [n] "+s"(n), [voff] "+&v"(voff),               \
      [out] "+&v"(out_addr)                                                                                                                    \
      : [b0] "s"(b0), [b1] "s"(b1), [stride] "v"(out_stride), [mzero] "v"(mzero)
  if constexpr (LOW) asm volatile(MISTRA_GSUM_ASM_LOW : MISTRA_GSUM_OPERANDS : "memory", "scc", MISTRA_GSUM_CLOBBER_LOW);
  else asm volatile(MISTRA_GSUM_ASM_HIGH : MISTRA_GSUM_OPERANDS : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
}
// The same behind a workgroup barrier that the stream runs itself, between its ring fill and its first counted wait: a call that
// follows lds_barrier() directly waited out the barrier and THEN a whole table round trip with nothing to do; the table loads do
// not depend on LDS, only the operand gathers do.  (The call stands in place of lds_barrier() + gsum_run().)
template <int NT, bool LOW>
__device__ __attribute__((noinline)) void gsum_run_bar(const GsDev P, uint32_t row0, int rows, int lane, uint32_t out_addr, uint32_t out_stride) {
  int n = __builtin_amdgcn_readfirstlane(rows);
  const uint64_t b0 = gsum_base(P, row0), b1 = b0 + 4096u;
  uint32_t voff = (uint32_t)lane * 32u;
  double acc = -0.0;
  const double mzero = -0.0;
  double xA0, xA1, xA2, xA3, xB0, xB1, xB2, xB3, cA0, cA1, cA2, cA3, cB0, cB1, cB2, cB3;
  uint32_t ad, flA, flB;
  static_assert(!LOW, "generated for the high placement of the ring only (gsum_exec_asm.inc)");
  asm volatile(MISTRA_GSUM_ASM_HIGH_BAR : MISTRA_GSUM_OPERANDS : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
}
// A wave's chain passes (schedule.hpp: GsumChain; the instruction stream: tools/gen_gsum_asm.py, pass_variant): the long sums four at a
// time, one per 16-lane row, the running sum taking the products in term order by v_fmac_f64_dpp row_newbcast.  Each pass stores its
// sums to the cells its table names.  rows > 0, whole ring turns.  BARRIER (0 | 1): as gsum_run_bar.
template <int NT, int BARRIER, bool LOW>
__device__ __attribute__((noinline)) void gsum_pass_run(const GsDev P, uint32_t row0, int rows, int lane) {
  static_assert(!LOW, "generated for the high placement of the ring only (gsum_exec_asm.inc)");
  int n = __builtin_amdgcn_readfirstlane(rows);
  const uint64_t b0 = gsum_base(P, row0), b1 = b0 + 4096u;
  uint32_t voff = (uint32_t)lane * 32u, out_addr = 0;
  const uint32_t out_stride = 0;
  double acc = -0.0;
  const double mzero = -0.0, one = 1.0;
  double xA0, xA1, xA2, xA3, xB0, xB1, xB2, xB3, cA0, cA1, cA2, cA3, cB0, cB1, cB2, cB3;
  uint32_t ad, flA, flB;
  if constexpr (BARRIER) asm volatile(MISTRA_GSUM_ASM_HIGH_PASS_BAR : MISTRA_GSUM_OPERANDS, [one] "v"(one) : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
  else asm volatile(MISTRA_GSUM_ASM_HIGH_PASS : MISTRA_GSUM_OPERANDS, [one] "v"(one) : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
}
#undef MISTRA_GSUM_OPERANDS
// Two programs back to back (fun_jac: the Vdot sums, then the JVS sums): in its last ring turn the first stream's refills fetch the
// second one's first four rows where they fetched slack rows, it returns without draining them, and the second stream enters on
// the ring as it stands — one table round trip where there were two.  The ring is full between the two statements: they sit in
// ONE non-inlined function, whose own values the build holds below the ring like the other executors'.  BARRIER (0 | 1): as
// gsum_run_bar.  (An int: the ring's placement is the one bool among these functions' template arguments, the build's register check and
// tests/test_capi.py read it off the symbol.)
template <int NT, int BARRIER, bool LOW>
__device__ __attribute__((noinline)) void gsum_run_pair(const GsDev P, uint32_t row0, int rows, uint32_t out_addr, uint32_t out_stride,
                                                        const GsDev Q, uint32_t qrow0, int qrows, uint32_t qout_addr, uint32_t qout_stride, int lane) {
  static_assert(!LOW, "generated for the high placement of the ring only (gsum_exec_asm.inc)");
  int n = __builtin_amdgcn_readfirstlane(rows), m = __builtin_amdgcn_readfirstlane(qrows);
  const uint64_t q0 = gsum_base(Q, qrow0);
  uint64_t b0 = gsum_base(P, row0), b1 = b0 + 4096u;
  // the lane offset has moved on by 8 KiB per group of four rows when the last turn's refills are issued: 2 KiB per row
  const uint64_t nb0 = q0 - (uint64_t)(uint32_t)n * 2048u, nb1 = nb0 + 4096u;
  uint32_t voff = (uint32_t)lane * 32u;
  double acc = -0.0;
  const double mzero = -0.0;
  double xA0, xA1, xA2, xA3, xB0, xB1, xB2, xB3, cA0, cA1, cA2, cA3, cB0, cB1, cB2, cB3;
  uint32_t ad, flA, flB;
#define MISTRA_GSUM_OUTPUTS(N, OUT)                                                                                                            \
  [acc] "+&v"(acc), [ad] "=&v"(ad), [xA0] "=&v"(xA0), [xA1] "=&v"(xA1), [xA2] "=&v"(xA2), [xA3] "=&v"(xA3), [xB0] "=&v"(xB0), [xB1] "=&v"(xB1),    \
      [xB2] "=&v"(xB2), [xB3] "=&v"(xB3), [cA0] "=&v"(cA0), [cA1] "=&v"(cA1), [cA2] "=&v"(cA2), [cA3] "=&v"(cA3), [cB0] "=&v"(cB0),               \
      [cB1] "=&v"(cB1), [cB2] "=&v"(cB2), [cB3] "=&v"(cB3), [flA] "=&s"(flA), [flB] "=&s"(flB), [n] "+s"(N), [voff] "+&v"(voff), [out] "+&v"(OUT)
#define MISTRA_GSUM_FIRST MISTRA_GSUM_OUTPUTS(n, out_addr), [b0] "+&s"(b0), [b1] "+&s"(b1) : [nb0] "s"(nb0), [nb1] "s"(nb1), [stride] "v"(out_stride), [mzero] "v"(mzero)
  if constexpr (BARRIER) asm volatile(MISTRA_GSUM_ASM_HIGH_BAR_CHAIN : MISTRA_GSUM_FIRST : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
  else asm volatile(MISTRA_GSUM_ASM_HIGH_CHAIN : MISTRA_GSUM_FIRST : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
  // the second program, its first four rows in flight
  const uint64_t q1 = q0 + 4096u;
  voff = (uint32_t)lane * 32u;
  acc = -0.0;
#define MISTRA_GSUM_SECOND MISTRA_GSUM_OUTPUTS(m, qout_addr) : [b0] "s"(q0), [b1] "s"(q1), [stride] "v"(qout_stride), [mzero] "v"(mzero)
  asm volatile(MISTRA_GSUM_ASM_HIGH_PRIMED : MISTRA_GSUM_SECOND : "memory", "scc", MISTRA_GSUM_CLOBBER_HIGH);
#undef MISTRA_GSUM_OUTPUTS
#undef MISTRA_GSUM_FIRST
#undef MISTRA_GSUM_SECOND
}

// ---- the factorisation's last act (schedule.hpp: ScaleProgram): M[tgt] *= M[aux] for two cells per 16-byte slot,
//      slots streamed through the look-ahead ring.  All cells are distinct: no ordering among lanes.
template <int NT, bool LOW>
__device__ __attribute__((noinline)) void scale_run(const ScaleDev P, int wave, int lane) {
  const int n = __builtin_amdgcn_readfirstlane(P.nslots);
  gptr<u32x4> rp = G_(reinterpret_cast<const u32x4*>(P.recs)) + ((size_t)wave * (size_t)P.wave_slots * 64 + lane);
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");     // nothing of the caller's may sit between the counted loads
  vm_ring_load<LOW, 0>(rp);       vm_ring_load<LOW, 1>(rp + 64);  vm_ring_load<LOW, 2>(rp + 128); vm_ring_load<LOW, 3>(rp + 192);
  vm_ring_load<LOW, 4>(rp + 256); vm_ring_load<LOW, 5>(rp + 320); vm_ring_load<LOW, 6>(rp + 384); vm_ring_load<LOW, 7>(rp + 448);
  rp += kRingSlots * 64;
  // TRIM: the last ring turn issues no refills — nobody reads those rows, and the drain below waited a whole table round trip for
  // them, issued an iteration earlier.  Without refills behind it, slot K is the oldest of 8 - K loads in flight.
  constexpr bool TRIM = MISTRA_STREAM_SCALE_TRIM && !LOW;
  const int n_refilled = TRIM ? n - kRingSlots : n;
    // four slots at a time: sixteen gathers in flight, then the eight products (a lone gather-multiply-store chain per
    // slot would expose the LDS latency sixteen times over)
#define MISTRA_SCALE_GROUP(K, REFILL)                                                \
    {                                                                                \
      const u32x4 a0 = vm_ring_take<LOW, K, REFILL ? 7 : 7 - K>();     if constexpr (REFILL) vm_ring_load<LOW, K>(rp + K * 64);         \
      const u32x4 a1 = vm_ring_take<LOW, K + 1, REFILL ? 7 : 6 - K>(); if constexpr (REFILL) vm_ring_load<LOW, K + 1>(rp + (K + 1) * 64); \
      const u32x4 a2 = vm_ring_take<LOW, K + 2, REFILL ? 7 : 5 - K>(); if constexpr (REFILL) vm_ring_load<LOW, K + 2>(rp + (K + 2) * 64); \
      const u32x4 a3 = vm_ring_take<LOW, K + 3, REFILL ? 7 : 4 - K>(); if constexpr (REFILL) vm_ring_load<LOW, K + 3>(rp + (K + 3) * 64); \
      const double v0 = lds_ld(a0.x), f0 = lds_ld(a0.y), v1 = lds_ld(a0.z), f1 = lds_ld(a0.w); \
      const double v2 = lds_ld(a1.x), f2 = lds_ld(a1.y), v3 = lds_ld(a1.z), f3 = lds_ld(a1.w); \
      const double v4 = lds_ld(a2.x), f4 = lds_ld(a2.y), v5 = lds_ld(a2.z), f5 = lds_ld(a2.w); \
      const double v6 = lds_ld(a3.x), f6 = lds_ld(a3.y), v7 = lds_ld(a3.z), f7 = lds_ld(a3.w); \
      lds_st(a0.x, v0 * f0); lds_st(a0.z, v1 * f1); lds_st(a1.x, v2 * f2); lds_st(a1.z, v3 * f3); \
      lds_st(a2.x, v4 * f4); lds_st(a2.z, v5 * f5); lds_st(a3.x, v6 * f6); lds_st(a3.z, v7 * f7); \
    }
    // the low placement (one wave per cell with a scaling pass: a user slot of 64 .. 128 species) leaves the function's own values the registers
    // below v64: two slots at a time there, eight gathers in flight and four products — half the live values of a group of four (which reached
    // v65).  The cells are distinct and every product is one multiply: the result is the same bits in any grouping.  Every slot is refilled behind
    // its take (TRIM is the high placement's), so slot K is the oldest of the eight loads in flight: vmcnt(7), as in a refilled group of four.
#define MISTRA_SCALE_PAIR(K)                                                         \
    {                                                                                \
      const u32x4 a0 = vm_ring_take<LOW, K, 7>();     vm_ring_load<LOW, K>(rp + K * 64);             \
      const u32x4 a1 = vm_ring_take<LOW, K + 1, 7>(); vm_ring_load<LOW, K + 1>(rp + (K + 1) * 64);   \
      const double v0 = lds_ld(a0.x), f0 = lds_ld(a0.y), v1 = lds_ld(a0.z), f1 = lds_ld(a0.w); \
      const double v2 = lds_ld(a1.x), f2 = lds_ld(a1.y), v3 = lds_ld(a1.z), f3 = lds_ld(a1.w); \
      lds_st(a0.x, v0 * f0); lds_st(a0.z, v1 * f1); lds_st(a1.x, v2 * f2); lds_st(a1.z, v3 * f3); \
    }
  for (int i = 0; i < n_refilled; i += kRingSlots) {
    if constexpr (LOW) {
      MISTRA_SCALE_PAIR(0) MISTRA_SCALE_PAIR(2) MISTRA_SCALE_PAIR(4) MISTRA_SCALE_PAIR(6)
    } else {
      MISTRA_SCALE_GROUP(0, true) MISTRA_SCALE_GROUP(4, true)
    }
    rp += kRingSlots * 64;
  }
#undef MISTRA_SCALE_PAIR
  if constexpr (TRIM) {
    if (n > 0) { MISTRA_SCALE_GROUP(0, false) MISTRA_SCALE_GROUP(4, false) }
  }
#undef MISTRA_SCALE_GROUP
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");     // drain the look-ahead loads before returning
}

// ---- dense tail block (schedule.hpp: DenseTail): the last 64 rows and columns of Ghimj, factorised in registers.
//      Tile (I, J) of the 4x4 grid of 16x16 tiles sits in wave 2I + (J>>1) as accumulator q = J&1 of
//      v_mfma_f64_16x16x4_f64: lane l, element r = row (l>>4) + 4r, column l&15 (cdna_hip_programming.md §3, verified by
//      tools/ubench).  Measured there: 64 cycles per MFMA and wave, the two waves of a SIMD overlapping fully; ~7 cycles per
//      dependent f64 operation, 72 for the IEEE reciprocal, ~30 for a same-wave LDS write -> read (which is why the
//      eliminating wave passes pivot rows lane to lane through LDS: v_readlane into an SGPR and back costs ~60).
#ifdef MISTRA_DIAG_STAMPS      // diagnostic builds only (tools/diag_dense.sh): cycles of wave 0 per section of dense_lu, summed over calls
__device__ unsigned long long g_dense_stamps[24];
#define MISTRA_STAMP(var) const unsigned long long var = clock64();
#define MISTRA_STAMP_ADD(slot, expr) if (threadIdx.x == 0) atomicAdd(&g_dense_stamps[slot], (unsigned long long)(expr));
#else
#define MISTRA_STAMP(var)
#define MISTRA_STAMP_ADD(slot, expr)
#endif
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f64x4 lds_f64x4;
__device__ __forceinline__ f64x4 lds_ld4(uint32_t addr) { return *(const lds_f64x4*)(uintptr_t)addr; }
__device__ __forceinline__ void lds_st4(uint32_t addr, f64x4 v) { *(lds_f64x4*)(uintptr_t)addr = v; }
// the same at an address that is a multiple of 16 only (two 16-byte accesses either way)
typedef __attribute__((address_space(3))) __attribute__((aligned(16))) f64x4 lds_f64x4_a16;
__device__ __forceinline__ f64x4 lds_ld4_a16(uint32_t addr) { return *(const lds_f64x4_a16*)(uintptr_t)addr; }
__device__ __forceinline__ void lds_st4_a16(uint32_t addr, f64x4 v) { *(lds_f64x4_a16*)(uintptr_t)addr = v; }

// Ghimj slot (LDS byte address) of column c of a row's column range, from the row's table entry {first, absent lo, absent hi}
// (schedule.hpp: DenseTail); an absent entry reads as the 0.0 cell `zero`.
__device__ __forceinline__ uint32_t dense_slot(const u32x4 info, const uint32_t c, const uint32_t zero) {
  const uint64_t absent = (uint64_t)info.y | ((uint64_t)info.z << 32);
  const uint32_t idx = info.x + c - (uint32_t)__builtin_popcountll(absent & ((1ull << c) - 1ull));
  return ((absent >> c) & 1ull) ? zero : 8u * idx;
}
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
__device__ __forceinline__ u32x4 lds_ldu4(uint32_t addr) { return *(const lds_u32x4*)(uintptr_t)addr; }

// The finished entries of panel P go from the panel buffers to their Ghimj slots: waves 1 and 3 the L columns (two pivots
// each; wave 1 also the pivots' reciprocals), waves 2 and 5 the (row-scaled) U rows — waves that sit on other SIMDs than
// wave 0.  Runs while wave 0 eliminates inside panel P+1: the buffers of panel P are rewritten by panel P+2, two barriers
// later.
__device__ __forceinline__ bool dense_is_storer(const int wave) { return wave == 1 || wave == 2 || wave == 3 || wave == 5; }
template <class MT, int NT>
__device__ __forceinline__ void dense_store_panel(const int P, const int wave, const int lane) {
  constexpr uint32_t NNZ = MT::NNZ, NVAR = MT::NVAR, H = NVAR - 64, ZERO = 8u * (NNZ + NVAR);
  constexpr uint32_t PB = 8u * (uint32_t)LdsLayout<MT, NT>::PANEL, BC = PB + 8192u, INFO = 8u * (uint32_t)LdsLayout<MT, NT>::DINFO;
  const uint32_t PL = PB + (uint32_t)(P & 1) * 4096u, PU = PL + 2048u;
  const int J0P = 4 * P, khalf = (wave == 3 || wave == 5) ? 2 : 0;
  const f64x4 rcp = lds_ld4(BC + 1024u + 32u * (uint32_t)(P & 1));
  if (wave & 1) {
    if (wave != 5) {
      const f64x4 a = lds_ld4(PL + 32u * lane);
      const u32x4 mine = lds_ldu4(INFO + 16u * lane);
      const double a0 = khalf ? a[2] : a[0], a1 = khalf ? a[3] : a[1];
      const uint32_t at0 = dense_slot(mine, (uint32_t)(J0P + khalf), ZERO), at1 = dense_slot(mine, (uint32_t)(J0P + khalf + 1), ZERO);
      if (lane > J0P + khalf && at0 != ZERO) lds_st(at0, a0);                                               // L(H+lane, H+4P+k)
      if (lane > J0P + khalf + 1 && at1 != ZERO) lds_st(at1, a1);
      if (wave == 1 && lane >= J0P && lane < J0P + 4) {                                                     // R(k) = 1/U(k,k)
        const int k = lane - J0P;
        lds_st(8u * (NNZ + NVAR + 4u + H + (uint32_t)lane), k == 0 ? rcp[0] : k == 1 ? rcp[1] : k == 2 ? rcp[2] : rcp[3]);
      }
      return;
    }
  }
  {
    const f64x4 b = lds_ld4(PU + 32u * lane);
    const double b0 = khalf ? b[2] : b[0], b1 = khalf ? b[3] : b[1], r0 = khalf ? rcp[2] : rcp[0], r1 = khalf ? rcp[3] : rcp[1];
    const uint32_t at0 = dense_slot(lds_ldu4(INFO + 16u * (uint32_t)(J0P + khalf)), (uint32_t)lane, ZERO);
    const uint32_t at1 = dense_slot(lds_ldu4(INFO + 16u * (uint32_t)(J0P + khalf + 1)), (uint32_t)lane, ZERO);
    if (lane >= J0P + khalf && at0 != ZERO) lds_st(at0, lane == J0P + khalf ? b0 : b0 * r0);               // U'(H+4P+k, H+lane), the diagonal unscaled
    if (lane >= J0P + khalf + 1 && at1 != ZERO) lds_st(at1, lane == J0P + khalf + 1 ? b1 : b1 * r1);
  }
}

// One panel of four pivots, 4P .. 4P+3 of the block.
//   1. the owners of block column K = P/4 and block row K put the panel's four columns / rows into LDS: PL[row][4], PU[col][4]
//   2. wave 0 eliminates inside the panel, lane = row for PL and lane = column for PU, pivot by pivot in the order of
//      KppDecomp_x (gas.f:6160-6171), and leaves L, U and the pivots' reciprocals in the panel buffers
//   3. every tile that still has open rows and columns takes the rank-4 update with one MFMA (rows and columns up to the
//      panel's last pivot enter as exact zeros)
// During step 2 of the NEXT panel two otherwise idle waves store the finished L(i,j), U'(j,c) = U(j,c)*R(j), U(j,j), R(j)
// to their Ghimj slots, for the solves (dense_store_panel)
// The two panel buffers alternate, so that step 1 of the next panel can start while slower waves are still in step 3.
// Panels 0 .. 11 run here (pivots 0 .. 47; the last sixteen pivots are dense_finish's), as a loop of copies of the body
// (MISTRA_DENSE_UNROLL below; fully unrolled, sixteen panels were 39 KB of straight-line code executed once per decomposition, and
// instruction fetch, not arithmetic, set its pace); the tile
// registers a panel needs are picked with selects on wave-uniform conditions, which the compiler resolves where P's low bits are
// compile-time constants of the copy.
template <class MT, int NT>
__device__ __forceinline__ void dense_panel(f64x4& T0, f64x4& T1, const int P, const int wave, const int lane
#ifdef MISTRA_DIAG_STAMPS
                                            , unsigned long long (&acc)[5]
#endif
) {
  const int K = P >> 2, S = P & 3, J0P = 4 * P, K2 = (J0P + 4) >> 4;
  constexpr uint32_t PB = 8u * (uint32_t)LdsLayout<MT, NT>::PANEL, BC = PB + 8192u;
  const uint32_t PL = PB + (uint32_t)(P & 1) * 4096u, PU = PL + 2048u;
  const int I = wave >> 1, J0 = 2 * (wave & 1);
  const uint32_t lrow = (uint32_t)(lane >> 4), lcol = (uint32_t)(lane & 15);
  MISTRA_STAMP(ta)
  // (the two tiles are two named values and every choice among their registers is a select on a wave-uniform condition:
  //  an array indexed by K or S would be put in scratch memory, a global-memory round trip per access)
  if (I >= K && (wave & 1) == (K >> 1)) {
    const bool odd = K & 1;
    const double t0 = odd ? T1[0] : T0[0], t1 = odd ? T1[1] : T0[1], t2 = odd ? T1[2] : T0[2], t3 = odd ? T1[3] : T0[3];
    if ((int)(lcol >> 2) == S) {
      const uint32_t at = PL + 8u * ((16u * I + lrow) * 4u + (lcol & 3u));
      lds_st(at, t0); lds_st(at + 128u, t1); lds_st(at + 256u, t2); lds_st(at + 384u, t3);
    }
  }
  if (I == K) {
    if (J0 >= K) lds_st(PU + 8u * ((16u * J0 + lcol) * 4u + lrow), S == 0 ? T0[0] : S == 1 ? T0[1] : S == 2 ? T0[2] : T0[3]);
    if (J0 + 1 >= K) lds_st(PU + 8u * ((16u * (J0 + 1) + lcol) * 4u + lrow), S == 0 ? T1[0] : S == 1 ? T1[1] : S == 2 ? T1[2] : T1[3]);
  }
  lds_barrier();
  MISTRA_STAMP(tb)
  if (wave == 0) {
    // A lone wave issues one instruction every 4-7 cycles whatever it is: this block is kept to the eliminations themselves.
    // The panel's 4x4 diagonal block is read by EVERY lane (uniform addresses: broadcast reads) and factorised redundantly in
    // every lane: the dependent chain  pivot -> reciprocal -> multipliers -> next pivot  then runs in registers, without the
    // LDS round trip per pivot that handing rows from lane to lane would cost (~1000 -> ~500 cycles per panel).  The lanes'
    // own panel entries (lane = row: a, lane = column: b) take the same operations with the same operands: where they
    // coincide with the block's entries the values are bit-identical.
    f64x4 a = lds_ld4(PL + 32u * lane), b = lds_ld4(PU + 32u * lane);
    const f64x4 c0 = lds_ld4(PU + 32u * (uint32_t)J0P), c1 = lds_ld4(PU + 32u * (uint32_t)(J0P + 1));      // column j of the block: rows 0..3
    const f64x4 c2 = lds_ld4(PU + 32u * (uint32_t)(J0P + 2)), c3 = lds_ld4(PU + 32u * (uint32_t)(J0P + 3));
    f64x4 rcp;
    rcp[0] = 1.0 / c0[0];
    const double l10 = c0[1] * rcp[0], l20 = c0[2] * rcp[0], l30 = c0[3] * rcp[0];
    const double u01 = c1[0], u02 = c2[0], u03 = c3[0];
    const double d11 = __builtin_fma(-l10, u01, c1[1]), d12 = __builtin_fma(-l10, u02, c2[1]), d13 = __builtin_fma(-l10, u03, c3[1]);
    double d21 = __builtin_fma(-l20, u01, c1[2]), d22 = __builtin_fma(-l20, u02, c2[2]), d23 = __builtin_fma(-l20, u03, c3[2]);
    double d31 = __builtin_fma(-l30, u01, c1[3]), d32 = __builtin_fma(-l30, u02, c2[3]), d33 = __builtin_fma(-l30, u03, c3[3]);
    rcp[1] = 1.0 / d11;
    const double l21 = d21 * rcp[1], l31 = d31 * rcp[1];
    d22 = __builtin_fma(-l21, d12, d22); d23 = __builtin_fma(-l21, d13, d23);
    d32 = __builtin_fma(-l31, d12, d32); d33 = __builtin_fma(-l31, d13, d33);
    rcp[2] = 1.0 / d22;
    const double l32 = d32 * rcp[2];
    d33 = __builtin_fma(-l32, d23, d33);
    rcp[3] = 1.0 / d33;
    // lane = row: L(i, 4P+k) = (entry - earlier multipliers times the pivot rows' entries) * R(k), columns ascending
    a[0] = a[0] * rcp[0];
    a[1] = __builtin_fma(-a[0], u01, a[1]); a[2] = __builtin_fma(-a[0], u02, a[2]); a[3] = __builtin_fma(-a[0], u03, a[3]);
    a[1] = a[1] * rcp[1];
    a[2] = __builtin_fma(-a[1], d12, a[2]); a[3] = __builtin_fma(-a[1], d13, a[3]);
    a[2] = a[2] * rcp[2];
    a[3] = __builtin_fma(-a[2], d23, a[3]);
    a[3] = a[3] * rcp[3];
    // lane = column: U(4P+k, c) = entry - the row's multipliers times the earlier pivot rows, pivots ascending
    b[1] = __builtin_fma(-l10, b[0], b[1]); b[2] = __builtin_fma(-l20, b[0], b[2]); b[3] = __builtin_fma(-l30, b[0], b[3]);
    b[2] = __builtin_fma(-l21, b[1], b[2]); b[3] = __builtin_fma(-l31, b[1], b[3]);
    b[3] = __builtin_fma(-l32, b[2], b[3]);
    lds_st4(PL + 32u * lane, a);      // L(H+lane, H+4P+k) for lane > 4P+k
    lds_st4(PU + 32u * lane, b);      // U(H+4P+k, H+lane) for lane >= 4P+k
    if (lane == 0) lds_st4(BC + 1024u + 32u * (uint32_t)(P & 1), rcp);
  } else if (dense_is_storer(wave) && P > 0) {
    dense_store_panel<MT, NT>(P - 1, wave, lane);      // while wave 0 eliminates: the previous panel's entries go to their Ghimj slots
  }
  MISTRA_STAMP(tc)
  lds_barrier();
  MISTRA_STAMP(td)
  if (I >= K2) {
    // rows and columns up to the panel's last pivot are finished: their operand is an exact zero, whatever the buffers hold there
    const double aop = (int)(16u * I + lcol) >= J0P + 4 ? -lds_ld(PL + 8u * ((16u * I + lcol) * 4u + lrow)) : 0.0;
    if (J0 >= K2) {
      const double bop = (int)(16u * J0 + lcol) >= J0P + 4 ? lds_ld(PU + 8u * ((16u * J0 + lcol) * 4u + lrow)) : 0.0;
      T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, bop, T0, 0, 0, 0);
    }
    if (J0 + 1 >= K2) {
      const double bop = (int)(16u * (J0 + 1) + lcol) >= J0P + 4 ? lds_ld(PU + 8u * ((16u * (J0 + 1) + lcol) * 4u + lrow)) : 0.0;
      T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, bop, T1, 0, 0, 0);
    }
  }
  MISTRA_STAMP(te)
#ifdef MISTRA_DIAG_STAMPS
  acc[0] += tb - ta; acc[1] += tc - tb; acc[2] += td - tc; acc[3] += te - td; acc[4] += 1;
#endif
}

// ---- the block's last 16 pivots, 48 .. 63: tile (3,3) factorised by its owner, wave 7, alone — no panel, no workgroup barrier.
// As panels these four cost what any panel costs (~1.9 k cycles each: two barriers, two LDS hand-overs) for a matrix that
// sits in one wave's registers.  Here: lane = row (lane & 15; the four 16-lane rows hold the same problem, so that
// row_newbcast serves all of them and the stores can be shared out), the row's 16 columns in registers.  Per pivot j, ascending,
// exactly dense_panel's operations per entry: R = 1/D(j,j); l(i) = D(i,j) * R; D(i,c) = fma(-l(i), D(j,c), D(i,c)) for i, c > j,
// the pivot row's entry reaching its lane row inside the multiply-add (v_fmac_f64_dpp, as the tail chain's).
// Which lanes take a pivot's update is EXEC's business, lanes >= j: a finished row must not take a "neutral" update with l = 0
// (x + (+0.0) turns a stored -0.0 into +0.0), and DPP is not assumed to read a lane that EXEC has switched off — so the pivot's
// own lane j stays on and multiplies with l = -0.0: its update is x + (-x)(-0.0), a zero of x's own sign added to x, which
// leaves every finite x and both zeros bit for bit as they are.  Not an infinite x: inf + (-inf)(-0.0) is NaN, where the panels
// left the pivot row's inf alone.  After such an overflow the stored U'(j,c) of that row differ from the panel form's (NaN for
// inf); a factorisation holding either makes the solves' result non-finite, the error norm with it, and `Err <= 1` rejects the step.
#define MISTRA_FIN_F(J, C) "v_fmac_f64_dpp %[x" #C "], -%[x" #C "], %[l] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define MISTRA_DPP_FROM_15(F, J) F(J, 15)
#define MISTRA_DPP_FROM_14(F, J) F(J, 14) MISTRA_DPP_FROM_15(F, J)
#define MISTRA_DPP_FROM_13(F, J) F(J, 13) MISTRA_DPP_FROM_14(F, J)
#define MISTRA_DPP_FROM_12(F, J) F(J, 12) MISTRA_DPP_FROM_13(F, J)
#define MISTRA_DPP_FROM_11(F, J) F(J, 11) MISTRA_DPP_FROM_12(F, J)
#define MISTRA_DPP_FROM_10(F, J) F(J, 10) MISTRA_DPP_FROM_11(F, J)
#define MISTRA_DPP_FROM_9(F, J) F(J, 9) MISTRA_DPP_FROM_10(F, J)
#define MISTRA_DPP_FROM_8(F, J) F(J, 8) MISTRA_DPP_FROM_9(F, J)
#define MISTRA_DPP_FROM_7(F, J) F(J, 7) MISTRA_DPP_FROM_8(F, J)
#define MISTRA_DPP_FROM_6(F, J) F(J, 6) MISTRA_DPP_FROM_7(F, J)
#define MISTRA_DPP_FROM_5(F, J) F(J, 5) MISTRA_DPP_FROM_6(F, J)
#define MISTRA_DPP_FROM_4(F, J) F(J, 4) MISTRA_DPP_FROM_5(F, J)
#define MISTRA_DPP_FROM_3(F, J) F(J, 3) MISTRA_DPP_FROM_4(F, J)
#define MISTRA_DPP_FROM_2(F, J) F(J, 2) MISTRA_DPP_FROM_3(F, J)
#define MISTRA_DPP_FROM_1(F, J) F(J, 1) MISTRA_DPP_FROM_2(F, J)
#define MISTRA_DPP_FROM_16(F, J)
#define MISTRA_FIN_XS [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [x3] "+v"(x3), [x4] "+v"(x4), [x5] "+v"(x5), [x6] "+v"(x6), [x7] "+v"(x7), \
                      [x8] "+v"(x8), [x9] "+v"(x9), [x10] "+v"(x10), [x11] "+v"(x11), [x12] "+v"(x12), [x13] "+v"(x13), [x14] "+v"(x14), [x15] "+v"(x15)
// pivot J (J1 = J + 1): the diagonal to every lane of its row (the wait states: the register was written two instructions back
// at the latest); the IEEE division in C++, the same one dense_panel compiles to; then the multipliers for the lanes below J — into
// the column's own register, which is where L(i, J) is stored from, and into l — and the update of the columns behind J.
#define MISTRA_FIN_PIVOT(J, J1)                                                                                                       \
  {                                                                                                                                   \
    double dg, l;                                                                                                                     \
    asm volatile("s_nop 1\n\tv_mov_b64_dpp %[dg], %[x] row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : [dg] "=v"(dg) : [x] "v"(x##J));       \
    const double R = 1.0 / dg;                                                                                                        \
    constexpr uint32_t GE = ((0xffffu << J) & 0xffffu) * 0x10001u, GT = ((0xffffu << J1) & 0xffffu) * 0x10001u;                       \
    asm volatile("v_mov_b64 %[l], %[nz]\n\t"                                                                                          \
                 "s_mov_b32 exec_lo, %[gt]\n\ts_mov_b32 exec_hi, %[gt]\n\t"                                                           \
                 "v_mul_f64 %[l], %[x" #J "], %[R]\n\t"                                                                               \
                 "v_mul_f64 %[x" #J "], %[x" #J "], %[R]\n\t"                                                                         \
                 "s_mov_b32 exec_lo, %[ge]\n\ts_mov_b32 exec_hi, %[ge]\n\t"                                                           \
                 MISTRA_DPP_FROM_##J1(MISTRA_FIN_F, J)                                                                                             \
                 "s_mov_b64 exec, -1"                                                                                                 \
                 : [l] "=&v"(l), MISTRA_FIN_XS : [R] "v"(R), [nz] "v"(nz), [gt] "i"((int)GT), [ge] "i"((int)GE));                               \
  }
// A diagonal tile in its owner's accumulator registers T, factorised through the 16 rows of the LDS buffer BUF (144 bytes apart) and left
// there row by row, L below the diagonal and U from it on.  LAST: the block's last tile, (3,3): its entries and reciprocals go to their Ghimj slots
// from here.  Else the tile of a tile step (dense_lu): the waves that solve the step's panels read the rows, and one of them stores them.
template <class MT, int NT, bool LAST>
__device__ __forceinline__ void dense_diag_tile(const f64x4 T, const int lane, const uint32_t BUF) {
  constexpr uint32_t NNZ = MT::NNZ, NVAR = MT::NVAR, H = NVAR - 64, ZERO = 8u * (NNZ + NVAR);
  constexpr uint32_t INFO = 8u * (uint32_t)LdsLayout<MT, NT>::DINFO, RDIAG = 8u * (NNZ + NVAR + 4u);
  constexpr uint32_t STRIDE = 144u;      // rows 16 bytes apart in the banks
  const uint32_t lrow = (uint32_t)(lane >> 4), i = (uint32_t)(lane & 15);
  MISTRA_STAMP(tf0)
  // accumulator layout (lane l, element r = row (l>>4) + 4r, column l&15) -> lane = row: through LDS; one wave, in-order LDS
#pragma unroll
  for (int r = 0; r < 4; r++) lds_st(BUF + STRIDE * (lrow + 4u * r) + 8u * i, T[r]);
  const f64x4 q0 = lds_ld4_a16(BUF + STRIDE * i), q1 = lds_ld4_a16(BUF + STRIDE * i + 32u), q2 = lds_ld4_a16(BUF + STRIDE * i + 64u), q3 = lds_ld4_a16(BUF + STRIDE * i + 96u);
  double x0 = q0[0], x1 = q0[1], x2 = q0[2], x3 = q0[3], x4 = q1[0], x5 = q1[1], x6 = q1[2], x7 = q1[3];
  double x8 = q2[0], x9 = q2[1], x10 = q2[2], x11 = q2[3], x12 = q3[0], x13 = q3[1], x14 = q3[2], x15 = q3[3];
  // the lane's four slots: row 48 + i, columns 48 + 4 lrow .. + 3 (dense_slot for four columns in a row, all in the table's high word)
  uint32_t at[4];
  if constexpr (LAST) {
    const u32x4 info = lds_ldu4(INFO + 16u * (48u + i));
    const uint32_t cb = 16u + 4u * lrow;
    uint32_t idx = info.x + 32u + cb - (uint32_t)__builtin_popcount(info.y) - (uint32_t)__builtin_popcount(info.z & ((1u << cb) - 1u));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t absent = (info.z >> (cb + (uint32_t)k)) & 1u;
      at[k] = absent ? ZERO : 8u * idx;
      idx += 1u - absent;
    }
  }
  const double nz = -0.0;
  MISTRA_FIN_PIVOT(0, 1) MISTRA_FIN_PIVOT(1, 2) MISTRA_FIN_PIVOT(2, 3) MISTRA_FIN_PIVOT(3, 4) MISTRA_FIN_PIVOT(4, 5)
  MISTRA_FIN_PIVOT(5, 6) MISTRA_FIN_PIVOT(6, 7) MISTRA_FIN_PIVOT(7, 8) MISTRA_FIN_PIVOT(8, 9) MISTRA_FIN_PIVOT(9, 10)
  MISTRA_FIN_PIVOT(10, 11) MISTRA_FIN_PIVOT(11, 12) MISTRA_FIN_PIVOT(12, 13) MISTRA_FIN_PIVOT(13, 14) MISTRA_FIN_PIVOT(14, 15)
  MISTRA_STAMP(tf1)
  // rows as they are finished — L(i,c) left of the diagonal, U(i,c) from it on — back through LDS, so that each of the four
  // lanes of a row takes its four columns and the row's own diagonal without sixteen-way selects
  lds_st4_a16(BUF + STRIDE * i, f64x4{x0, x1, x2, x3}); lds_st4_a16(BUF + STRIDE * i + 32u, f64x4{x4, x5, x6, x7});
  lds_st4_a16(BUF + STRIDE * i + 64u, f64x4{x8, x9, x10, x11}); lds_st4_a16(BUF + STRIDE * i + 96u, f64x4{x12, x13, x14, x15});
  if constexpr (LAST) {
    const f64x4 v = lds_ld4_a16(BUF + STRIDE * i + 32u * lrow);
    const double R = 1.0 / lds_ld(BUF + STRIDE * i + 8u * i);      // R(i) = 1/U(i,i): the pivot's own division again, in the row's lanes
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t c = 4u * lrow + (uint32_t)k;
      if (at[k] != ZERO) lds_st(at[k], c > i ? v[k] * R : v[k]);      // U'(i,c) = U(i,c) * R(i); the diagonal and L(i,c) as they are
    }
    if (lrow == 0) lds_st(RDIAG + 8u * (H + 48u + i), R);
  }
  MISTRA_STAMP(tf2)
#ifdef MISTRA_DIAG_STAMPS
  if ((lane & 63) == 0) { atomicAdd(&g_dense_stamps[LAST ? 13 : 16], tf1 - tf0); atomicAdd(&g_dense_stamps[LAST ? 14 : 17], tf2 - tf1); }
#endif
}
// the block's last 16 pivots: called by the kernel (a call from dense_lu would make that function save registers of its own)
template <class MT, int NT>
__device__ __attribute__((noinline)) void dense_finish(const f64x4 T, const int lane) {
  typedef LdsLayout<MT, NT> L;
  // with tile steps in front: the odd diagonal buffer, which the step of block column 1 used last (its storer read it two barriers ago; the storer
  // of block column 2 reads the even one meanwhile).  Else the panel buffers' even half: panel 11 and its storers use the odd one
  constexpr uint32_t BUF = 8u * (uint32_t)(L::DENSE_TILES ? L::TILE_D + L::TILE_CELLS : L::PANEL);
  dense_diag_tile<MT, NT, true>(T, lane, BUF);
}
#undef MISTRA_FIN_PIVOT
#undef MISTRA_FIN_F

// ---- a tile step: the sixteen pivots 16K .. 16K+15 of block column K < 3 in one go (dense_lu; MISTRA_DENSE_TILE_FROM), in place of four panels.
//   1. the owner of tile (K,K) factorises it by itself (dense_diag_tile) and leaves it in the diagonal buffer; meanwhile the owners of the open tiles
//      of block column K put them into the L buffers as rows, those of block row K theirs into the U buffers as columns; barrier
//   2. one wave solves the L panel, lane = row, its four 16-lane rows one tile each: for pivot j ascending  x_j *= R(j),  x_c = fma(-x_j, U(j,c), x_c)
//      for c > j.  A wave on another SIMD solves the U panel, lane = column: for pivot m ascending  b_i = fma(-L(i,m), b_m, b_i)  for i > m.  Both hold
//      row (lane & 15) of the finished diagonal tile in registers, and the other lanes' entry reaches the multiply-add by row_newbcast — every lane
//      is live, so no EXEC handling.  Per entry these are the panels' operations in the panels' order (tests/emu/schedule_emu.cpp).  The results go
//      back over the buffers they came from; barrier
//   3. every open tile takes four MFMAs, k ascending, operands straight from the buffers: whole tiles, so no zero masks
//   4. the stores to the Ghimj slots, for the solves, all off the chain's path: the diagonal tile (L below, the unscaled diagonal, U'(j,c) = U(j,c)*R(j)
//      right of it, and R(j)) by its owner beside step 2 — it has no panel and no open tile in its own step —, the panels L(i,j) and U'(j,c) by the waves
//      that solved them, beside step 3 — they have no open tile in any step
// The buffers are single: the next step's entry barrier stands between a step's MFMA reads and the next step's writers.
struct DenseRow { double x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15; };
__device__ __forceinline__ void dense_row_load(DenseRow& X, const uint32_t at) {
  const f64x4 q0 = lds_ld4_a16(at), q1 = lds_ld4_a16(at + 32u), q2 = lds_ld4_a16(at + 64u), q3 = lds_ld4_a16(at + 96u);
  X.x0 = q0[0]; X.x1 = q0[1]; X.x2 = q0[2]; X.x3 = q0[3]; X.x4 = q1[0]; X.x5 = q1[1]; X.x6 = q1[2]; X.x7 = q1[3];
  X.x8 = q2[0]; X.x9 = q2[1]; X.x10 = q2[2]; X.x11 = q2[3]; X.x12 = q3[0]; X.x13 = q3[1]; X.x14 = q3[2]; X.x15 = q3[3];
}
__device__ __forceinline__ void dense_row_store(const DenseRow& X, const uint32_t at) {
  lds_st4_a16(at, f64x4{X.x0, X.x1, X.x2, X.x3}); lds_st4_a16(at + 32u, f64x4{X.x4, X.x5, X.x6, X.x7});
  lds_st4_a16(at + 64u, f64x4{X.x8, X.x9, X.x10, X.x11}); lds_st4_a16(at + 96u, f64x4{X.x12, X.x13, X.x14, X.x15});
}
#define MISTRA_TS_L(J, C) "v_fmac_f64_dpp %[x" #C "], -%[d" #C "], %[x" #J "] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define MISTRA_TS_U(J, C) "v_fmac_f64_dpp %[x" #C "], -%[d" #J "], %[x" #J "] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"
#define MISTRA_TS_LP(J, J1) "v_mov_b64_dpp %[rj], %[R] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\tv_mul_f64 %[x" #J "], %[x" #J "], %[rj]\n\t" MISTRA_DPP_FROM_##J1(MISTRA_TS_L, J)
#define MISTRA_TS_UP(J, J1) MISTRA_DPP_FROM_##J1(MISTRA_TS_U, J)
#define MISTRA_TS_ALL(P) P(0, 1) P(1, 2) P(2, 3) P(3, 4) P(4, 5) P(5, 6) P(6, 7) P(7, 8) P(8, 9) P(9, 10) P(10, 11) P(11, 12) P(12, 13) P(13, 14) P(14, 15) P(15, 16)
#define MISTRA_TS_XS [x0] "+v"(X.x0), [x1] "+v"(X.x1), [x2] "+v"(X.x2), [x3] "+v"(X.x3), [x4] "+v"(X.x4), [x5] "+v"(X.x5), [x6] "+v"(X.x6), [x7] "+v"(X.x7), \
                     [x8] "+v"(X.x8), [x9] "+v"(X.x9), [x10] "+v"(X.x10), [x11] "+v"(X.x11), [x12] "+v"(X.x12), [x13] "+v"(X.x13), [x14] "+v"(X.x14), [x15] "+v"(X.x15)
#define MISTRA_TS_DS [d0] "v"(D.x0), [d1] "v"(D.x1), [d2] "v"(D.x2), [d3] "v"(D.x3), [d4] "v"(D.x4), [d5] "v"(D.x5), [d6] "v"(D.x6), [d7] "v"(D.x7), \
                     [d8] "v"(D.x8), [d9] "v"(D.x9), [d10] "v"(D.x10), [d11] "v"(D.x11), [d12] "v"(D.x12), [d13] "v"(D.x13), [d14] "v"(D.x14), [d15] "v"(D.x15)
// step 2 for the lane's row (LSIDE) or column of the tile buffer at XB, against the finished diagonal tile at DB.  LSIDE: R = R(lane & 15) = 1/U(i,i),
// the pivot's own division again, and left behind the tile's row for the wave that stores the U rows.  (The s_nop: the wait states of a DPP source that
// a VALU instruction wrote — the division's result, or a copy the compiler put in front.)
template <bool LSIDE>
__device__ __forceinline__ void dense_tile_solve(DenseRow& X, double& R, const uint32_t DB, const uint32_t XB, const int lane) {
  const uint32_t i = (uint32_t)(lane & 15);
  DenseRow D;
  dense_row_load(D, DB + 144u * i);
  dense_row_load(X, XB + 144u * i);
  if constexpr (LSIDE) {
    R = 1.0 / lds_ld(DB + 144u * i + 8u * i);
    double rj;      // R(j) in every lane (v_mul_f64 has no DPP form)
    asm volatile("s_nop 1\n\t" MISTRA_TS_ALL(MISTRA_TS_LP) : [rj] "=&v"(rj), MISTRA_TS_XS : [R] "v"(R), MISTRA_TS_DS);
  } else {
    asm volatile("s_nop 1\n\t" MISTRA_TS_ALL(MISTRA_TS_UP) : MISTRA_TS_XS : MISTRA_TS_DS);
  }
  dense_row_store(X, XB + 144u * i);
  if constexpr (LSIDE)
    if (lane < 16) lds_st(DB + 144u * i + 128u, R);
}
#undef MISTRA_TS_L
#undef MISTRA_TS_U
#undef MISTRA_TS_LP
#undef MISTRA_TS_UP
#undef MISTRA_TS_ALL
#undef MISTRA_TS_XS
#undef MISTRA_TS_DS
#undef MISTRA_FIN_XS
#undef MISTRA_DPP_FROM_1
#undef MISTRA_DPP_FROM_2
#undef MISTRA_DPP_FROM_3
#undef MISTRA_DPP_FROM_4
#undef MISTRA_DPP_FROM_5
#undef MISTRA_DPP_FROM_6
#undef MISTRA_DPP_FROM_7
#undef MISTRA_DPP_FROM_8
#undef MISTRA_DPP_FROM_9
#undef MISTRA_DPP_FROM_10
#undef MISTRA_DPP_FROM_11
#undef MISTRA_DPP_FROM_12
#undef MISTRA_DPP_FROM_13
#undef MISTRA_DPP_FROM_14
#undef MISTRA_DPP_FROM_15
#undef MISTRA_DPP_FROM_16

// step 4, branch-free: an entry the pattern does not have goes to the trash cell.
// The diagonal tile of block column K, by its owner behind barrier 1, while the panels are solved: from its buffer DB, four columns per lane, with the
// row's R(i) = 1/U(i,i), the pivot's own division again (what dense_diag_tile does for the last tile)
template <class MT, int NT>
__device__ __forceinline__ void dense_tile_store_d(const int K, const uint32_t DB, const int lane) {
  constexpr uint32_t NNZ = MT::NNZ, NVAR = MT::NVAR, H = NVAR - 64, TRASH = 8u * (NNZ + NVAR + 2u);
  constexpr uint32_t INFO = 8u * (uint32_t)LdsLayout<MT, NT>::DINFO, RDIAG = 8u * (NNZ + NVAR + 4u);
  const uint32_t q = (uint32_t)(lane >> 4), i = (uint32_t)(lane & 15), c0 = 16u * (uint32_t)K, cb = c0 + 4u * q;
  const u32x4 info = lds_ldu4(INFO + 16u * (c0 + i));
  const f64x4 v = lds_ld4_a16(DB + 144u * i + 32u * q);
  const double R = 1.0 / lds_ld(DB + 144u * i + 8u * i);
  const uint64_t absent = (uint64_t)info.y | ((uint64_t)info.z << 32);
  uint32_t idx = info.x + cb - (uint32_t)__builtin_popcountll(absent & ((1ull << cb) - 1ull));
  const uint32_t ab = (uint32_t)(absent >> cb);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t a = (ab >> k) & 1u, c = 4u * q + (uint32_t)k;
    lds_st(a ? TRASH : 8u * idx, c > i ? v[k] * R : v[k]);      // U'(i,c) = U(i,c) * R(i); the diagonal and L(i,c) as they are
    idx += 1u - a;
  }
  if (q == 0) lds_st(RDIAG + 8u * (H + c0 + i), R);
}
// the sixteen entries X of row `row` of the block from column c0 on, each times f
__device__ __forceinline__ void dense_row_to_slots(const DenseRow& X, const double f, const bool scaled, const uint32_t row, const uint32_t c0, const uint32_t INFO, const uint32_t TRASH) {
  const u32x4 info = lds_ldu4(INFO + 16u * row);
  const uint64_t absent = (uint64_t)info.y | ((uint64_t)info.z << 32);
  uint32_t idx = info.x + c0 - (uint32_t)__builtin_popcountll(absent & ((1ull << c0) - 1ull));
  const uint32_t ab = (uint32_t)(absent >> c0);
#define MISTRA_TS_ST(k) { const uint32_t a = (ab >> k) & 1u; lds_st(a ? TRASH : 8u * idx, scaled ? X.x##k * f : X.x##k); idx += 1u - a; }
  MISTRA_TS_ST(0) MISTRA_TS_ST(1) MISTRA_TS_ST(2) MISTRA_TS_ST(3) MISTRA_TS_ST(4) MISTRA_TS_ST(5) MISTRA_TS_ST(6) MISTRA_TS_ST(7)
  MISTRA_TS_ST(8) MISTRA_TS_ST(9) MISTRA_TS_ST(10) MISTRA_TS_ST(11) MISTRA_TS_ST(12) MISTRA_TS_ST(13) MISTRA_TS_ST(14) MISTRA_TS_ST(15)
#undef MISTRA_TS_ST
}
// The L panel, behind barrier 2 in the wave that solved it, from its registers: the lane's row of L(16(K+1+q)+i, 16K ..), q = lane >> 4 (lane rows past
// the block's last tile row hold a copy of the last one and store the same values to the same slots)
template <class MT, int NT>
__device__ __forceinline__ void dense_tile_store_l(const DenseRow& X, const int K, const int lane) {
  constexpr uint32_t NNZ = MT::NNZ, NVAR = MT::NVAR;
  const int q = (lane >> 4) < 2 - K ? (lane >> 4) : 2 - K;
  dense_row_to_slots(X, 0.0, false, 16u * (uint32_t)(K + 1 + q) + (uint32_t)(lane & 15), 16u * (uint32_t)K, 8u * (uint32_t)LdsLayout<MT, NT>::DINFO, 8u * (NNZ + NVAR + 2u));
}
// ... and the U panel in the wave that solved it: row by row as well, so that a lane finds its sixteen slots by counting on from the first — the
// wave reads its tiles back from the buffers UB (tile K+1+q at UB + q * TB), where it left them as columns, lane = row; U'(i,c) = U(i,c) * R(i) with
// R(i) from behind the diagonal tile's row, where the other solving wave left it in front of barrier 2
template <class MT, int NT>
__device__ __forceinline__ void dense_tile_store_u(const int K, const uint32_t DB, const uint32_t UB, const uint32_t TB, const int lane) {
  constexpr uint32_t NNZ = MT::NNZ, NVAR = MT::NVAR;
  const int q = (lane >> 4) < 2 - K ? (lane >> 4) : 2 - K;
  const uint32_t i = (uint32_t)(lane & 15), at = UB + TB * (uint32_t)q + 8u * i;
  DenseRow Y;
  Y.x0 = lds_ld(at); Y.x1 = lds_ld(at + 144u); Y.x2 = lds_ld(at + 2u * 144u); Y.x3 = lds_ld(at + 3u * 144u);
  Y.x4 = lds_ld(at + 4u * 144u); Y.x5 = lds_ld(at + 5u * 144u); Y.x6 = lds_ld(at + 6u * 144u); Y.x7 = lds_ld(at + 7u * 144u);
  Y.x8 = lds_ld(at + 8u * 144u); Y.x9 = lds_ld(at + 9u * 144u); Y.x10 = lds_ld(at + 10u * 144u); Y.x11 = lds_ld(at + 11u * 144u);
  Y.x12 = lds_ld(at + 12u * 144u); Y.x13 = lds_ld(at + 13u * 144u); Y.x14 = lds_ld(at + 14u * 144u); Y.x15 = lds_ld(at + 15u * 144u);
  dense_row_to_slots(Y, lds_ld(DB + 144u * i + 128u), true, 16u * (uint32_t)K + i, 16u * (uint32_t)(K + 1 + q), 8u * (uint32_t)LdsLayout<MT, NT>::DINFO, 8u * (NNZ + NVAR + 2u));
}

// The dense tail block after the LU program and the scaling pass: Schur steps, then the block's own factorisation.  Every
// Ghimj slot it touches is found by arithmetic on the row table in LDS: a global load issued here, in the middle of a cell's
// step, waits behind the table streams of the whole chip (measured: 13 000 cycles in front of the first MFMA).
template <class MT, int NT>
__device__ __attribute__((noinline)) f64x4 dense_lu(int lane) {
  static_assert(NT == 512 && MT::DENSE_ND == 64, "eight waves, two 16x16 tiles each");
  constexpr int KB = MT::DENSE_KB;
  constexpr uint32_t NNZ = MT::NNZ, NVAR = MT::NVAR, H = NVAR - 64, JM = H - 4 * KB, ZERO = 8u * (NNZ + NVAR);
  constexpr uint32_t INFO = 8u * (uint32_t)LdsLayout<MT, NT>::DINFO, RDIAG = 8u * (NNZ + NVAR + 4u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t I = (uint32_t)(wave >> 1), J0 = 2u * (uint32_t)(wave & 1), lrow = (uint32_t)(lane >> 4), lcol = (uint32_t)(lane & 15);
  MISTRA_STAMP(t0)
  // ---- the block's slots as the LU program and the scaling pass leave them -> tiles
  f64x4 T0, T1;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const u32x4 info = lds_ldu4(INFO + 16u * (16u * I + lrow + 4u * r));
    T0[r] = lds_ld(dense_slot(info, 16u * J0 + lcol, ZERO));
    T1[r] = lds_ld(dense_slot(info, 16u * J0 + 16u + lcol, ZERO));
  }
  // ---- Schur steps: pivots jm .. h-1, four per MFMA, ascending: D -= W * U' with W the still unscaled L slots of the
  //      block's rows and U' the row-scaled U slots of the pivots' rows (schedule.hpp: DenseTail).  The operands' cells come from
  //      the host-made table in LDS, and everything is fetched in three batches (cells, values, then the MFMAs): taken step by
  //      step, every step waited out three dependent LDS round trips and ~60 instructions of row-table arithmetic (round 2:
  //      7 500 cycles for these 28 MFMAs).
  constexpr uint32_t SCH = 8u * (uint32_t)LdsLayout<MT, NT>::SCHUR;
  typedef __attribute__((address_space(3))) uint16_t lds_u16;
  const uint32_t wtab = SCH + 2u * ((uint32_t)I * KB * 64u + (uint32_t)lane);                                            // + 128 k
  const uint32_t utab = SCH + 2u * (4u * KB * 64u + (uint32_t)(wave & 1) * KB * 128u + (uint32_t)lane);                   // + 256 k (+ 128: second tile)
  uint32_t wslot[KB];
  double wl[KB];
  static_assert(KB % 2 == 0, "two batches of Schur steps");
#pragma unroll
  for (int half = 0; half < 2; half++) {      // two batches of KB/2 steps: one batch of all KB needed more registers than dense_lu can have without saving callee-saved ones
    constexpr int HB = KB / 2;
    uint32_t us0[HB], us1[HB];
#pragma unroll
    for (int kk = 0; kk < HB; kk++) {
      const int k = half * HB + kk;
      wslot[k] = 8u * (uint32_t)*(const lds_u16*)(uintptr_t)(wtab + 128u * k);
      us0[kk] = 8u * (uint32_t)*(const lds_u16*)(uintptr_t)(utab + 256u * k);
      us1[kk] = 8u * (uint32_t)*(const lds_u16*)(uintptr_t)(utab + 256u * k + 128u);
    }
    __builtin_amdgcn_sched_barrier(0);      // (the compiler's scheduler would otherwise weave the batches back into one chain per step)
    double u0[HB], u1[HB];
#pragma unroll
    for (int kk = 0; kk < HB; kk++) {
      wl[half * HB + kk] = lds_ld(wslot[half * HB + kk]);
      u0[kk] = lds_ld(us0[kk]);
      u1[kk] = lds_ld(us1[kk]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < HB; kk++) {
      T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-wl[half * HB + kk], u0[kk], T0, 0, 0, 0);
      T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-wl[half * HB + kk], u1[kk], T1, 0, 0, 0);
    }
  }
  // R(j) of the steps' pivots for the lane's own multipliers (below); the reads run beside the MFMAs
  double rj[KB / 2];
#pragma unroll
  for (int k2 = 0; k2 < KB / 2; k2++) rj[k2] = lds_ld(RDIAG + 8u * (JM + 4u * (2u * k2 + (uint32_t)(wave & 1)) + lrow));
  MISTRA_STAMP(t1)
  lds_barrier();      // both waves of a block row have read the unscaled slots
  {                   // L = W * R(j) for the solves; the two waves of a block row share the work (steps k even / k odd)
    static_assert(KB % 2 == 0, "the two waves of a block row take every other Schur step");
    if (wave & 1) {   // (wave-uniform branch: compile-time register indices on both sides)
#pragma unroll
      for (int k = 1; k < KB; k += 2)
        if (wslot[k] != ZERO) lds_st(wslot[k], wl[k] * rj[k / 2]);
    } else {
#pragma unroll
      for (int k = 0; k < KB; k += 2)
        if (wslot[k] != ZERO) lds_st(wslot[k], wl[k] * rj[k / 2]);
    }
  }
  MISTRA_STAMP(t2)
  MISTRA_STAMP_ADD(0, t1 - t0) MISTRA_STAMP_ADD(1, t2 - t1) MISTRA_STAMP_ADD(9, 1)
  // ---- the block's own factorisation
  // Twelve panels, pivots 0 .. 47; the last sixteen pivots are tile (3,3)'s alone and wave 7 finishes them by itself (dense_finish).
#ifndef MISTRA_DENSE_UNROLL      // panels per copy of the loop body.  12 = all of them: every choice among tile registers (panel within its block column,
#define MISTRA_DENSE_UNROLL 12     // odd / even block column) is made at compile time.  The same-box passes of 2, 3, 6, 8 (the compiler adds a copy of four
#endif                            // for the remainder) and 12 are in profiles/r06_ab_dense_finish.txt; 4 makes the function save a register to scratch and
                                  // was not measured.  (All 16 panels unrolled were slower than two copies of eight in round 2: instruction fetch.)
#ifndef MISTRA_DIAG_DENSE_PANELS      // timing diagnostics only (tools/diag_dense.sh): a library built with fewer than 12 panels computes garbage
#define MISTRA_DIAG_DENSE_PANELS 12
#endif
  static_assert(MISTRA_DIAG_DENSE_PANELS <= 12, "the panels end where the in-wave finish begins");
  // ... of which the block columns from MISTRA_DENSE_TILE_FROM on go as tile steps instead (below), four panels each
  constexpr int FROM = MISTRA_DENSE_TILE_FROM, NPANEL = MISTRA_DIAG_DENSE_PANELS < 4 * FROM ? MISTRA_DIAG_DENSE_PANELS : 4 * FROM;
#ifdef MISTRA_DIAG_STAMPS
  unsigned long long acc[5] = {0, 0, 0, 0, 0};
  MISTRA_STAMP(tp0)
#pragma unroll 1
  for (int P = 0; P < NPANEL; P++) dense_panel<MT, NT>(T0, T1, P, wave, lane, acc);
  MISTRA_STAMP(tp1)
  MISTRA_STAMP_ADD(2, acc[0]) MISTRA_STAMP_ADD(3, acc[1]) MISTRA_STAMP_ADD(4, acc[2]) MISTRA_STAMP_ADD(5, acc[3]) MISTRA_STAMP_ADD(8, acc[4]) MISTRA_STAMP_ADD(12, tp1 - tp0)
#else
#pragma unroll MISTRA_DENSE_UNROLL
  for (int P = 0; P < NPANEL; P++) dense_panel<MT, NT>(T0, T1, P, wave, lane);
#endif
  if constexpr (FROM == 3) {
    // behind panel 11's second barrier: its entries go to their Ghimj slots from the odd panel buffers, while wave 7 takes its tile
    // to dense_finish (the caller's call: a call from here would make this function save registers of its own) and works in the even
    // ones; everybody else goes on to the caller's barrier
    if (dense_is_storer(wave)) dense_store_panel<MT, NT>(11, wave, lane);
  } else {
    typedef LdsLayout<MT, NT> L;
    constexpr uint32_t TB = 8u * (uint32_t)L::TILE_CELLS, DBUF = 8u * (uint32_t)L::TILE_D, LBUF = 8u * (uint32_t)L::TILE_L, UBUF = 8u * (uint32_t)L::TILE_U;
    // (the panels' buffers lie where the tile buffers do: the last panel's entries are stored in front of the first step's entry barrier)
    if constexpr (FROM > 0)
      if (dense_is_storer(wave)) dense_store_panel<MT, NT>(4 * FROM - 1, wave, lane);
    // the solving waves, LS for the L panel and US for the U panel: two of the waves 1, 4 and 6, whose own tiles are never open, on two SIMDs and neither
    // on the SIMD of the step's diagonal owner (waves 0, 2, 5: SIMDs 0, 2, 1), which stores its tile while they solve
#ifndef MISTRA_DENSE_TILE_UNROLL      // 3: a copy of the body per step, every choice among the tile registers and the solving waves made at compile time (44 KB
#define MISTRA_DENSE_TILE_UNROLL 3    // of code).  1: one body of 19 KB, the choices selects on K — measured 0.5 % slower (profiles/r18_ab_dense_tiles.txt)
#endif
#pragma unroll MISTRA_DENSE_TILE_UNROLL
    for (int K = FROM; K < 3; K++) {
      const int LS = K == 0 ? 1 : 4, US = K == 1 ? 1 : 6;
      if (K > FROM || FROM > 0) lds_barrier();      // entry: the buffers' readers of the step before (its MFMAs, or the last panel's) are done
      {
        const bool odd = K & 1;
        const f64x4 TK = odd ? T1 : T0;      // the wave's tile in block column K, if it has one
        if ((int)I > K && (wave & 1) == (K >> 1)) {
          const uint32_t at = LBUF + TB * (I - 1u) + 8u * lcol;
#pragma unroll
          for (int r = 0; r < 4; r++) lds_st(at + 144u * (lrow + 4u * r), TK[r]);
        }
        if ((int)I == K) {
          if ((int)J0 > K) {
            const uint32_t at = UBUF + TB * (J0 - 1u) + 144u * lcol + 8u * lrow;
#pragma unroll
            for (int r = 0; r < 4; r++) lds_st(at + 32u * r, T0[r]);
          }
          if ((int)J0 + 1 > K) {
            const uint32_t at = UBUF + TB * J0 + 144u * lcol + 8u * lrow;
#pragma unroll
            for (int r = 0; r < 4; r++) lds_st(at + 32u * r, T1[r]);
          }
        }
#ifdef MISTRA_DIAG_STAMPS
        if (wave == 4 && lane == 0) atomicAdd(&g_dense_stamps[23], 1ull);
#endif
      }
      {
        DenseRow X;      // the solving waves' row or column of their panel
        double R;
        const uint32_t DB = DBUF + TB * (uint32_t)(K & 1);
        MISTRA_STAMP(tc0)
        if (wave == 2 * K + (K >> 1)) dense_diag_tile<MT, NT, false>((K & 1) ? T1 : T0, lane, DB);
        MISTRA_STAMP(tc1)
        lds_barrier();
        MISTRA_STAMP(tc2)
        const uint32_t xt = TB * (uint32_t)(K + ((lane >> 4) < 2 - K ? (lane >> 4) : 2 - K));      // tile K+1+q, the last one again in the lane rows behind it
        if (wave == LS) dense_tile_solve<true>(X, R, DB, LBUF + xt, lane);
        else if (wave == US) dense_tile_solve<false>(X, R, DB, UBUF + xt, lane);
        else if (wave == 2 * K + (K >> 1)) dense_tile_store_d<MT, NT>(K, DB, lane);      // (the owner has no open tile in its own step)
        MISTRA_STAMP(tc3)
        lds_barrier();
        MISTRA_STAMP(tc4)
        if ((int)I > K) {
          const uint32_t la = LBUF + TB * (I - 1u) + 144u * lcol + 8u * lrow;
          const double a0 = -lds_ld(la), a1 = -lds_ld(la + 32u), a2 = -lds_ld(la + 64u), a3 = -lds_ld(la + 96u);
          if ((int)J0 > K) {
            const uint32_t ua = UBUF + TB * (J0 - 1u) + 144u * lcol + 8u * lrow;
            const double b0 = lds_ld(ua), b1 = lds_ld(ua + 32u), b2 = lds_ld(ua + 64u), b3 = lds_ld(ua + 96u);
            T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, T0, 0, 0, 0);
            T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, T0, 0, 0, 0);
            T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, T0, 0, 0, 0);
            T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b3, T0, 0, 0, 0);
          }
          if ((int)J0 + 1 > K) {
            const uint32_t ua = UBUF + TB * J0 + 144u * lcol + 8u * lrow;
            const double b0 = lds_ld(ua), b1 = lds_ld(ua + 32u), b2 = lds_ld(ua + 64u), b3 = lds_ld(ua + 96u);
            T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, T1, 0, 0, 0);
            T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, T1, 0, 0, 0);
            T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, T1, 0, 0, 0);
            T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b3, T1, 0, 0, 0);
          }
        }
        MISTRA_STAMP(tc5)
#ifdef MISTRA_DIAG_STAMPS      // the diagonal tile's owner: slots 16, 17 (dense_diag_tile) and its wait at barrier 1; wave 4: the solve and barrier 2; wave 7: the MFMAs
        if (wave == 2 * K + (K >> 1) && lane == 0) atomicAdd(&g_dense_stamps[18], tc2 - tc1);
        if (wave == LS && lane == 0) { atomicAdd(&g_dense_stamps[19], tc3 - tc2); atomicAdd(&g_dense_stamps[20], tc4 - tc3); }
        if (wave == 7 && lane == 0) atomicAdd(&g_dense_stamps[21], tc5 - tc4);
#endif
        // step 4 beside the MFMAs, in the solving waves, which have no open tile in any step
        MISTRA_STAMP(tq0)
        if (wave == LS) dense_tile_store_l<MT, NT>(X, K, lane);
        else if (wave == US) dense_tile_store_u<MT, NT>(K, DB, UBUF + TB * (uint32_t)K, TB, lane);
        MISTRA_STAMP(tq1)
#ifdef MISTRA_DIAG_STAMPS
        if (wave == LS && lane == 0) atomicAdd(&g_dense_stamps[22], tq1 - tq0);
#endif
      }
    }
  }
#ifdef MISTRA_DIAG_STAMPS
  lds_barrier();
  MISTRA_STAMP(tz)
  MISTRA_STAMP_ADD(11, tz - t0)
#endif
  return T1;
}

}  // namespace

// VARIANT: 0 = the product kernel; 1 = phase timing (MISTRA_CHEM_PROFILE, capi.cpp); 2 = first-step dump: the intermediate
// results of the FIRST attempt of the first step of every cell go to a.dump (layout: kernel_args.hpp), for the phase-level
// parity tests (tests/test_gpu_parity.py); the integration itself is untouched.  3 = Rosenbrock_x's options (gas.f:936-1053) out of
// a.opt instead of the values INTEGRATE_x fixes (kernel_args.hpp: RosOptSlot; capi.cpp: mistra_chem_set_options): every difference
// from variant 0 sits behind `if constexpr (OPT)`, the other three compile from the statements they always had.
// 5 = a series (ros_unit_kernel.hip; mistra_chem_rosenbrock_series_ex / _device): variant 3 with the part from the step-control set-up to the
// results inside a loop over a.nleg legs, leg k one call of Rosenbrock_x from a.times[k] to a.times[k+1] on the state leg k-1 left, its results in
// block k of the output arrays.  Everything the loop adds sits behind `if constexpr (SERIES)`; for the others the loop is one pass.  With a.leg_rconst /
// a.leg_fix /= 0 (mistra_chem_rosenbrock_series_rates_ex / _device) leg k integrates with the rate constants at a.rconst +
// k*a.leg_rconst and FIX at a.fix + k*a.leg_fix: a run-time form of the same fifteen kernels, taken up at the head of every leg behind the first.
// 6 = the reaction flux (ros_unit_kernel.hip; mistra_chem_rosenbrock_flux_ex / _device): variant 3 of any of the five methods that also integrates every
// reaction's rate over the call by the trapezoid rule on the accepted states and leaves one [NREACT] row per cell in a.flux.
// Everything it adds sits behind `if constexpr (FLUX)`.
// 7 = dense output (instantiated in the series units of ros_unit_kernel.hip; mistra_chem_rosenbrock_dense_ex / _device): variant 3 of any of the five methods
// that also leaves the state at a.dense_ns sample times inside the call, by the cubic Hermite interpolant between the accepted states.
// Everything it adds sits behind `if constexpr (DENSE)`.
// 8 = the operators (instantiated in the trace units of ros_unit_kernel.hip; mistra_chem_ops_ex / _device): no integration — Fun_x, Jac_SP_x and solves with
// shift*I - Jac_SP_x at the state given, by the step loop's own pieces, once.  One block behind the definitions of those pieces that ends
// with a return; everything it adds sits behind `if constexpr (OPS)`.
// 9 = the replay (instantiated in the trace units of ros_unit_kernel.hip; mistra_chem_rosenbrock_replay_ex / _device): variant 3 of Ros3 along a step
// sequence the caller prescribes (a.replay_*): step n of the cell's row is made with H = hsteps[n] and accepted whatever its Err, which
// goes to a.replay_err.  A step works as the options kernel's does, operand for operand; the step control around it (Hmin / Hmax / Hstart, the factors, the
// clipping to Tend, Max_no_steps, the halving at a zero pivot) is not there.  Everything it adds sits behind `if constexpr (REPLAY)`.
// 10 = a series whose rate constants are linear in time over each leg (instantiated in the method units and, for Ros3, the trace units of
// ros_unit_kernel.hip; mistra_chem_rosenbrock_series_linrates_ex / _device): variant 5 of any of the five methods with a.rconst holding nleg + 1 node blocks, block k the rate
// constants AT a.times[k] (a.leg_rconst: the node stride).  Every Fun_x / Jac_SP_x reads R(tau) at its own time — T at the head of a step, T +
// ros_Alpha(i)*Direction*H in a stage that evaluates anew — and the step adds HG*dFdT with dFdT = Fun_x(Y, FIX, dR/dt), one more Fun_x per step, where
// the others add their zero.  Everything it adds sits behind `if constexpr (LINR)`; what a series does it does as SERIES.
// 11 = a series with the reaction flux of every leg (instantiated beside variant 10, in the method units and, for Ros3, the trace units of
// ros_unit_kernel.hip; mistra_chem_rosenbrock_series_flux_ex / _device): variant 5 (with a.leg_rconst / a.leg_fix as there) of any of the five methods that
// also does per leg what variant 6 does per call — the flux state lives inside the legs' loop, starts afresh with every leg and is closed with the leg's own
// rate constants in front of the leg's results — and leaves leg k's [NREACT] row of a cell at a.flux + k*a.leg_flux.  It is SERIES
// and FLUX at once; what only the combination needs sits behind `if constexpr (SFLUX)`.
// METHOD (variant 3 only): the Rosenbrock method, IPAR(4) of Rosenbrock_x (ros_methods.hpp).  Ros3 is the kernel as it was; Ros2, Ros4, Rodas3
// and Rodas4 (the method kernels, instantiated by ros_unit_kernel.hip in translation units of their own) differ in the stage loop, in the
// number of stage vectors a thread keeps and in the constants — every such difference sits behind `if constexpr (METHOD == kRos3) ... else`.
template <class MT, int NT, int VARIANT, int METHOD = kRos3>
__global__ __launch_bounds__(NT, MT::WAVES_PER_SIMD) void ros3_integrate_kernel(const KernelArgs a) {
  constexpr bool PROF = VARIANT == 1, DUMP = VARIANT == 2, TRACE = VARIANT == 4, LINR = VARIANT == 10, SFLUX = VARIANT == 11, SERIES = VARIANT == 5 || LINR || SFLUX, FLUX = VARIANT == 6 || SFLUX, DENSE = VARIANT == 7, REPLAY = VARIANT == 9, OPT = VARIANT == 3 || TRACE || SERIES || FLUX || DENSE || REPLAY;
  constexpr bool OPS = VARIANT == 8;
  static_assert(!REPLAY || METHOD == kRos3, "the replay is a Ros3 instantiation (ros_unit_kernel.hip), as is the trace that supplies its sequence");
  static_assert(!OPS || METHOD == kRos3, "the operators are Ros3 instantiations (ros_unit_kernel.hip): no method is involved");
  static_assert(!TRACE || METHOD == kRos3, "the step-control trace is a Ros3 instantiation (ros_unit_kernel.hip)");
  static_assert(METHOD == kRos3 || (OPT && METHOD >= kRos2 && METHOD <= kRodas4), "the method kernels are options instantiations");
  constexpr double kGamma1 = METHOD == kRos3 ? kRosGamma1 : kRosMethod<METHOD>.Gamma[0];
  constexpr int NVAR = MT::NVAR, NFIX = MT::NFIX, NREACT = MT::NREACT, NNZ = MT::NNZ, NCONST = MT::NCONST;
  constexpr int NW = NT / 64;
  constexpr int SPT = (NVAR + NT - 1) / NT, RPT = (NREACT + NT - 1) / NT;
  constexpr int JPT = (MT::NJNZ + NT - 1) / NT, ZPT = (NNZ - MT::NJNZ + NT - 1) / NT;
  using L = LdsLayout<MT, NT>;

  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* const M = lds + L::M;
  double* const XS = M + NNZ;
  double* const X = lds + L::X;
  double* const AB = lds + L::AB;
  double* const JBp = lds + L::JB;      // Jac_SP's B products: inside the Ghimj area where it is large enough, else the A array (ros3_kernel.hpp)
  double* const red = lds + L::RED;
  int* const flags = reinterpret_cast<int*>(lds + L::FLAGS);

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int cell = blockIdx.x;
  if (cell >= a.ncell) return;
  if (lds_addr(lds) != 0u) {      // the VM and the tail chain address M by absolute LDS offsets
    if constexpr (OPS) {      // (no ierr: the refusal goes where the call has an integer per cell)
      if (t == 0 && a.ops_ising) GM_(a.ops_ising)[cell] = -99;
      return;
    }
    if constexpr (SERIES) {      // every leg's
      if (t == 0)
        for (int k = 0; k < a.nleg; k++) GM_(a.ierr)[(int64_t)k * a.leg_ierr + cell] = -99;
      return;
    }
    if (t == 0) GM_(a.ierr)[cell] = -99;
    if constexpr (TRACE) {
      if (t == 0) GM_(a.ntrace)[cell] = 0;
    }
    if constexpr (DENSE) {
      if (t == 0) GM_(a.dense_nout)[cell] = 0;
    }
    return;
  }

  // ---- where this wave's stream starts in each table program (and how long the gather-sum ones are): the same for the whole
  //      call, kept in scalar registers
  struct { uint32_t lu_row0, fwd_row0, bwd_row0, vdot_row0, jvs_row0, pass_row0, mask_lo, mask_hi; int vdot_rows, jvs_rows, pass_rows; } hdr;
  constexpr bool kGsumPass = MT::GSUM_CHAIN;      // the long Vdot sums as chain passes (schedule.hpp: GsumChain)
  {
    const auto u = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    hdr.lu_row0 = u(G_(a.lu.wave_base)[wave]);
    hdr.fwd_row0 = u(G_(a.solve_head_fwd.wave_base)[wave]);
    hdr.bwd_row0 = u(G_(a.solve_head_bwd.wave_base)[wave]);
    hdr.vdot_row0 = u(G_(a.vdot.wave_base)[wave]);
    hdr.jvs_row0 = u(G_(a.jvs.wave_base)[wave]);
    hdr.vdot_rows = (int)u(G_(a.vdot.rows)[wave]);
    hdr.jvs_rows = (int)u(G_(a.jvs.rows)[wave]);
    hdr.pass_row0 = hdr.mask_lo = hdr.mask_hi = 0; hdr.pass_rows = 0;
    if constexpr (kGsumPass) {      // this wave's chain passes (most waves have none) and which of its lanes' species are chained
      hdr.pass_row0 = u(G_(a.vdot_pass.wave_base)[wave]);
      hdr.pass_rows = (int)u(G_(a.vdot_pass.rows)[wave]);
      const uint64_t mask = G_(a.vdot_chain_mask)[wave];
      hdr.mask_lo = u((uint32_t)mask);
      hdr.mask_hi = u((uint32_t)(mask >> 32));
    }
  }

  // ---- per-cell inputs: coalesced cell-major reads, once
  double y[SPT], rct[RPT];
#pragma unroll
  for (int q = 0; q < SPT; q++) {
    const int s = q * NT + t;
    y[q] = s < NVAR ? G_(a.var_in)[(size_t)cell * NVAR + s] : 0.0;
  }
  // VARIANT 7: the rows of the samples k0 .. dense_ns-1 of this cell as +0.0 (not reached), and the number reached
  [[maybe_unused]] auto dense_leave = [&](int k0) {
    for (int k = k0; k < a.dense_ns; k++) {
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + t;
        if (s < NVAR) GM_(a.dense_out)[(int64_t)k * a.dense_block + (int64_t)cell * NVAR + s] = 0.0;
      }
    }
    if (t == 0) GM_(a.dense_nout)[cell] = k0;
  };
  // VARIANT 3: AbsTol / RelTol of this thread's species, out of the call's options block: one vector pair shared by all cells as in KPP.  Fetched once, here:
  // a global load in the middle of a step would wait behind the table streams.  The scalars of the block are fetched where the step
  // control uses them (opt), not kept across the step loop.
  [[maybe_unused]] double atol_r[SPT], rtol_r[SPT];
  [[maybe_unused]] bool autonomous = false;
  [[maybe_unused]] auto opt = [&](int slot) -> double {
    const double* ob = a.opt;
    asm volatile("" : "+s"(ob));      // opaque: the load stays where the value is used
    return G_(ob)[slot];
  };
  // a.tol_abs set: the cell's own rows instead (kernel_args.hpp), and Rosenbrock_x's check of them (gas.f:1045-1053) is made here, per cell: the
  // arrays may live on the device, the host has not seen them.  Every thread tests the entries it reads (vector mode: all NVAR between them;
  // scalar mode: entry 0 of the row), the cell takes the OR.  A refused cell leaves as a call the host refuses leaves: Y untouched, IERR = -5,
  // statistics, Texit / Hexit and H zero, no trace record.  All of it in front of the step loop: nothing of it is live inside.
  if constexpr (OPT) {
    const bool cells = a.tol_abs != nullptr;
    const double* ta = cells ? a.tol_abs + (size_t)cell * (size_t)a.tol_cell_stride : a.opt + kOptTol;
    const double* tr = cells ? a.tol_rel + (size_t)cell * (size_t)a.tol_cell_stride : a.opt + kOptTol + NVAR;
    const int ss = cells ? a.tol_spec_stride : 1;
#pragma unroll
    for (int q = 0; q < SPT; q++) {
      const int s = q * NT + t;
      atol_r[q] = s < NVAR ? G_(ta)[s * ss] : 1.0;
      rtol_r[q] = s < NVAR ? G_(tr)[s * ss] : 0.0;
    }
    // a.tol_cell_factor != 0 (the integrator policy, capi.cpp: policy_args): AbsTol of every species = max(floor, factor * max_i |Y(i)|) over the state as
    // received, as cell_atol_kernel (pack.hip) forms it — a NaN stays out of the maximum, the padding entries are 0.  Each thread over its own species,
    // the wave by wave_max, the workgroup through one cell of red[] per wave and one barrier (as the -5 check below).  The host has validated factor,
    // floor and RelTol: no check here.  In front of the step loop like the rest: only atol_r leaves.
    if (!cells && a.tol_cell_factor != 0.0) {      // (uniform over the call)
      double m = 0.0;
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const double v = fabs(y[q]);
        if (v > m) m = v;
      }
      m = wave_max(m);
      if constexpr (NW > 1) {
        if (lane == 0) red[wave] = m;
        lds_barrier();
        m = red[0];
#pragma unroll
        for (int w = 1; w < NW; w++) m = max_nn(m, red[w]);
      }
      const double r = a.tol_cell_factor * m;
      const double at = r > a.tol_cell_floor ? r : a.tol_cell_floor;
#pragma unroll
      for (int q = 0; q < SPT; q++) atol_r[q] = q * NT + t < NVAR ? at : 1.0;
    }
    autonomous = opt(kOptAutonomous) != 0.0;
    if (cells) {      // (uniform over the workgroup)
      bool bad = false;
#pragma unroll
      for (int q = 0; q < SPT; q++) {      // as the reference writes the tests: a NaN passes
        if (q * NT + t < NVAR) bad = bad || atol_r[q] <= 0.0 || rtol_r[q] <= 10.0 * 2.220446049250313e-16 || rtol_r[q] >= 1.0;
      }
      bool refused = __builtin_amdgcn_ballot_w64(bad) != 0ull;
      if constexpr (NW > 1) {      // one cell of red[] per wave, written by its lane 0; the error norm's first use of red[] is behind a barrier of its own
        if (lane == 0) red[wave] = refused ? 1.0 : 0.0;
        lds_barrier();
        refused = false;
#pragma unroll
        for (int w = 0; w < NW; w++) refused = refused || red[w] != 0.0;
      }
      if constexpr (SERIES) {      // once, in front of the first leg: every leg of the cell leaves as the refused call does
        if (refused) {
          for (int k = 0; k < a.nleg; k++) {
#pragma unroll
            for (int q = 0; q < SPT; q++) {
              const int s = q * NT + t;
              if (s < NVAR) GM_(a.var_out)[(int64_t)k * a.leg_var + (int64_t)cell * NVAR + s] = y[q];
            }
            if (t == 0) {
              GM_(a.ierr)[(int64_t)k * a.leg_ierr + cell] = -5;
              gptr_mut<int32_t> st = GM_(a.stats) + ((int64_t)k * a.leg_stats + (int64_t)cell * 8);
#pragma unroll
              for (int j = 0; j < 8; j++) st[j] = 0;
              if (a.texit_hexit) {
                GM_(a.texit_hexit)[(int64_t)k * a.leg_th + (int64_t)cell * 2] = 0.0;
                GM_(a.texit_hexit)[(int64_t)k * a.leg_th + (int64_t)cell * 2 + 1] = 0.0;
              }
              if (a.h_last) GM_(a.h_last)[(int64_t)k * a.leg_h + cell] = 0.0;
            }
            if constexpr (SFLUX) {      // no step was made in any leg: the cell's row of every leg is +0.0
#pragma unroll
              for (int q = 0; q < RPT; q++) {
                const int r = q * NT + t;
                if (r < NREACT) GM_(a.flux)[(int64_t)k * a.leg_flux + (int64_t)cell * NREACT + r] = 0.0;
              }
            }
          }
          return;
        }
      }
      if (refused) {
#pragma unroll
        for (int q = 0; q < SPT; q++) {
          const int s = q * NT + t;
          if (s < NVAR) GM_(a.var_out)[(size_t)cell * NVAR + s] = y[q];
        }
        if (t == 0) {
          GM_(a.ierr)[cell] = -5;
          gptr_mut<int32_t> st = GM_(a.stats) + (size_t)cell * 8;
#pragma unroll
          for (int k = 0; k < 8; k++) st[k] = 0;
          if (a.texit_hexit) {
            GM_(a.texit_hexit)[(size_t)cell * 2] = 0.0;
            GM_(a.texit_hexit)[(size_t)cell * 2 + 1] = 0.0;
          }
          if (a.h_last) GM_(a.h_last)[cell] = 0.0;
          if constexpr (TRACE) GM_(a.ntrace)[cell] = 0;
        }
        if constexpr (FLUX) {      // no step was made: the cell's row is +0.0
#pragma unroll
          for (int q = 0; q < RPT; q++) {
            const int r = q * NT + t;
            if (r < NREACT) GM_(a.flux)[(size_t)cell * NREACT + r] = 0.0;
          }
        }
        if constexpr (DENSE) dense_leave(0);      // no step was made: no sample is reached
        return;
      }
    }
  }
  // (the register-starved kernels fetch them per use, like their factor words)
  constexpr bool RCT_PER_USE = LINR || MT::WAVES_PER_SIMD > kResidentMaxWps || L::RCT_IN_LDS;      // (VARIANT 10: the rate constants are a function of the time, formed per use)
  // VARIANT 5: the leg index (the legs' loop, below).  Declared here because the leg's own rate constants (a.leg_rconst, kernel_args.hpp) start at
  // a.rconst + leg*a.leg_rconst: a base formed from two scalars where the fetch uses it, never a vector value kept across the step loop.
  [[maybe_unused]] int leg = 0;
  // VARIANT 10: the rate constants linear in time over the leg, between the node blocks a.rconst + leg*a.leg_rconst (at times[leg]) and the one behind it
  // (at times[leg + 1]).  lin_w = 1/(times[leg+1] - times[leg]) and lin_s = (tau - times[leg])*lin_w of the evaluation to come are wave-uniform (scalar
  // registers); lin_dot: the evaluation to come takes the time derivative d*lin_w in place of the value.  load_rct forms R(tau) = R0 + lin_s*d, d = R1 - R0,
  // every operation rounded on its own, of the reactions the thread owns: per use, out of global memory, for all three mechanisms (the cell's copy in LDS
  // and the resident registers hold nothing here).
  [[maybe_unused]] double lin_w = 0.0, lin_s = 0.0;
  [[maybe_unused]] bool lin_dot = false;
  auto load_rct = [&](bool opaque) {      // this thread's rate constants; opaque: the per-use fetch (RCT_PER_USE)
    const double* rc = a.rconst;
    if constexpr (SERIES) rc += (int64_t)leg * a.leg_rconst;
    if (opaque) asm volatile("" : "+s"(rc));
    int tt = t;
    if (opaque) asm volatile("" : "+v"(tt));      // (addresses derived where they are used: hoisted out of the step loop they are registers that spill)
    if constexpr (LINR) {
#pragma clang fp contract(off)
      const double* rc1 = rc + a.leg_rconst;
#pragma unroll
      for (int q = 0; q < RPT; q++) {
        const int r = q * NT + tt;
        const double r0 = r < NREACT ? G_(rc)[(size_t)cell * NREACT + r] : 0.0, r1 = r < NREACT ? G_(rc1)[(size_t)cell * NREACT + r] : 0.0;
        const double d = r1 - r0;
        const double up = lin_s * d;
        rct[q] = lin_dot ? d * lin_w : r0 + up;
      }
      return;
    }
#pragma unroll
    for (int q = 0; q < RPT; q++) {
      const int r = q * NT + tt;
      if constexpr (L::RCT_IN_LDS) {      // (per use: out of the cell's copy in LDS, put there once, below)
        if (opaque) { rct[q] = r < NREACT ? lds_ld(8u * (uint32_t)(L::RCT + r)) : 0.0; continue; }
      }
      rct[q] = r < NREACT ? G_(rc)[(size_t)cell * NREACT + r] : 0.0;
    }
  };
  if constexpr (LINR) {      // formed in front of every evaluation (load_rct)
#pragma unroll
    for (int q = 0; q < RPT; q++) rct[q] = 0.0;
  } else if constexpr (L::RCT_IN_LDS) {      // global -> LDS, once; read back by the same thread that wrote them (r = q*NT + t): no barrier involved
#pragma unroll
    for (int q = 0; q < RPT; q++) {
      const int r = q * NT + t;
      if (r < NREACT) lds[L::RCT + r] = G_(a.rconst)[(size_t)cell * NREACT + r];
      rct[q] = 0.0;
    }
  } else {
    load_rct(false);
  }
  // Ghimj slots this thread fills in ros_PrepareMatrix (static per mechanism): fetched once, not once per attempt
  // (two 16-bit positions per register)
  // RESIDENT: the kernel with 256 registers (tot) keeps these words for the whole call; the 128-register ones (aer, gas: four
  // waves per SIMD) fetch them where they are used — there they were spilled to scratch and came back from it one at a time.
  constexpr bool RESIDENT = MT::WAVES_PER_SIMD <= kResidentMaxWps;
  uint32_t jpos[(JPT + 1) / 2], zpos[(ZPT + 1) / 2];
  auto load_pos = [&]() {
    const uint16_t* jp = a.jvs_pos;
    const uint16_t* zp = a.zero_pos;
    int t = threadIdx.x;
    if constexpr (!RESIDENT) asm volatile("" : "+s"(jp), "+s"(zp), "+v"(t));      // opaque: neither the loads nor the per-thread addresses are hoisted out of the step loop
#pragma unroll
    for (int q = 0; q < (JPT + 1) / 2; q++)
      jpos[q] = (uint32_t)G_(jp)[(2 * q) * NT + t] | ((2 * q + 1 < JPT ? (uint32_t)G_(jp)[(2 * q + 1) * NT + t] : (uint32_t)kPosNone) << 16);
#pragma unroll
    for (int q = 0; q < (ZPT + 1) / 2; q++)
      zpos[q] = (uint32_t)G_(zp)[(2 * q) * NT + t] | ((2 * q + 1 < ZPT ? (uint32_t)G_(zp)[(2 * q + 1) * NT + t] : (uint32_t)kPosNone) << 16);
  };
  if constexpr (RESIDENT) load_pos();
  // factor words of the products this thread forms in Fun (one per owned reaction) and in Jac_SP (up to three per reaction): static
  // per mechanism, and fetched PER USE, in one batch of coalesced loads.  Values that live across the calls of the step loop need
  // callee-saved registers, there are not enough of those, and the compiler's answer was to spill nine of Jac_SP's twelve words and
  // reload them one at a time, each load's latency exposed (48 KB table, L2-resident; measured: the batch lands in ~380 cycles,
  // Jac_SP's products went from 11 000 to 7 400 cycles per call, the kernel's scratch from 104 to 8 bytes per lane).  Fun's words
  // likewise: resident, even the 256-register kernel was 3 registers over what it can keep across its calls — one word and an LDS
  // address went through scratch, reloaded right behind a barrier in every Fun, a memory round trip each; fetched per use they ride
  // in the batch of Jac_SP's words that fun_jac issues anyway, and the kernel has no scratch.
  uint64_t ffac[RPT];
  auto load_ffac = [&]() {
    const uint64_t* ff = a.fun_fac;
    asm volatile("" : "+s"(ff));      // opaque: loads through it are not hoisted out of the step loop (and spilled there)
#pragma unroll
    for (int q = 0; q < RPT; q++) ffac[q] = G_(ff)[q * NT + t];
  };
  if (t < NFIX) X[NVAR + t] = G_(a.fix)[(size_t)cell * NFIX + t];
  if (t < NCONST) X[NVAR + NFIX + t] = G_(a.consts)[t];
  if constexpr (MT::DENSE_ND > 0) {      // the dense tail block's row table stays in LDS for the whole call
    if (t < 64) *(lds_u32x4*)(uintptr_t)(8u * (uint32_t)L::DINFO + 16u * (uint32_t)t) = G_(reinterpret_cast<const u32x4*>(a.dense.row_info))[t];
    for (int i = t; i < L::SCHUR_WORDS; i += NT)      // the Schur steps' operand cells (uint16 pairs)
      *(__attribute__((address_space(3))) uint32_t*)(uintptr_t)(8u * (uint32_t)L::SCHUR + 4u * (uint32_t)i) = G_(reinterpret_cast<const uint32_t*>(a.dense.schur_cells))[i];
  }
  if (t == 0) {   // the VM's constant cells: 0.0 (padding update slots), 1.0 (neutral factor), -1.0 (partial-sum combine)
    M[NNZ + NVAR] = 0.0;
    M[NNZ + NVAR + 1] = 1.0;
    M[NNZ + NVAR + 3] = -1.0;
  }

  // optional phase timing (diagnostics only): cycles of wave 0 between phase boundaries, summed per cell
  constexpr bool profiling = PROF;       // a compile-time variant: sixteen 64-bit counters are not carried by the product kernel
  unsigned long long pc[kProfSlots] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t_last = profiling ? clock64() : 0ull;
  const unsigned long long t_begin = t_last;
  auto lap = [&](int slot) {
    if constexpr (profiling) {
      const unsigned long long now = clock64();
      pc[slot] += now - t_last;
      t_last = now;
    }
  };
  // ... and per wave around the gather-sum machine (kernel_args.hpp: kProfStride): thread 0 leaves its clock in the spare half of the flags'
  // cells in front of the evaluator's first barrier, every wave reads it behind that barrier and stamps against it
  unsigned long long pw[4] = {0, 0, 0, 0}, pw_calls[2] = {0, 0}, pw_ref = 0;
  auto wave_ref_put = [&]() {
    if constexpr (profiling) { if (t == 0) *reinterpret_cast<volatile unsigned long long*>(flags + 2) = clock64(); }
  };
  auto wave_ref_get = [&](int which) {
    if constexpr (profiling) { pw_ref = *reinterpret_cast<volatile unsigned long long*>(flags + 2); pw_calls[which]++; }
  };
  auto wave_stamp = [&](int slot) {
    if constexpr (profiling) pw[slot] += clock64() - pw_ref;
  };

  // first-step dump (VARIANT 2): one block of doubles per cell, see DumpLayout in kernel_args.hpp
  bool dumping = DUMP;
  gptr_mut<double> dump = nullptr;
  if constexpr (DUMP) dump = GM_(a.dump) + (size_t)cell * (size_t)(5 * NVAR + 2 * NNZ + 2);
  auto dump_vec = [&](int at, const double (&v)[SPT]) {
    if constexpr (DUMP) {
      if (dumping) {
#pragma unroll
        for (int q = 0; q < SPT; q++) {
          const int s = q * NT + t;
          if (s < NVAR) dump[at + s] = v[q];
        }
      }
    }
  };
  auto dump_matrix = [&](int at) {      // Ghimj as it stands in LDS (every lane's stores are behind a barrier at the call sites)
    if constexpr (DUMP) {
      if (dumping)
        for (int i = t; i < NNZ; i += NT) dump[at + i] = M[i];
    }
  };

  // ---- Fun_x (gas.f:2043): X <- v; A(r) = RCT(r)*X*X*X; Vdot = signed sums of A
  //      Jac_SP_x (gas.f:2656) on the V already in X: B products under their reaction, JVS sums into registers
  //      The pieces first; the three evaluators below (fun, jac, fun_jac) are sequences of them, with the barriers between.
  static_assert(SPT <= 2 && JPT * NT <= NNZ, "output cells of the gather-sum machine: at most two species per thread, JVS sums inside Ghimj");
  auto store_x = [&](const double (&v)[SPT]) {
#pragma unroll
    for (int q = 0; q < SPT; q++) {
      const int s = q * NT + t;
      if (s < NVAR) X[s] = v[q];
    }
  };
  auto a_products = [&]() {
    // every factor read is issued before the first product is stored: X and the product array are one LDS object to the
    // compiler, so a read behind a store stays behind it, and product by product each one waited out its own LDS round trip
    double f0[RPT], f1[RPT], f2[RPT];
    uint32_t slot[RPT];
#pragma unroll
    for (int q = 0; q < RPT; q++) {
      uint64_t w = ffac[q];
      asm volatile("" : "+v"(w));   // decode here: hoisted out of the step loop, the derived addresses only spill
      f0[q] = X[w & 0xFFFFu];
      f1[q] = X[(w >> 16) & 0xFFFFu];
      f2[q] = X[(w >> 32) & 0xFFFFu];
      slot[q] = (uint32_t)(w >> 48);
    }
#pragma unroll
    for (int q = 0; q < RPT; q++) {
      double p = rct[q] * f0[q];
      p = p * f1[q];
      p = p * f2[q];
      AB[slot[q]] = p;            // a slot without a reaction (rct = 0) writes a spare cell: no branch
    }
  };
  // VARIANT 6: A(r) of this thread's reactions r = q*NT + t at the state X holds, as a_products forms them (the same operands in the same order, so the
  // same bits), into registers instead of the product array.  Reads the factor words and rate constants the last Fun_x of the thread fetched.
  [[maybe_unused]] auto flux_products = [&](double (&p)[RPT]) {
#pragma unroll
    for (int q = 0; q < RPT; q++) {
      uint64_t w = ffac[q];
      asm volatile("" : "+v"(w));
      double v = rct[q] * X[w & 0xFFFFu];
      v = v * X[(w >> 16) & 0xFFFFu];
      p[q] = v * X[(w >> 32) & 0xFFFFu];
    }
  };
  auto load_jfac = [&](uint64_t (&jfac)[3 * RPT]) {
    const uint64_t* jf = a.jac_fac;
    asm volatile("" : "+s"(jf));      // opaque: loads through it are not hoisted out of the step loop (and spilled there)
#pragma unroll
    for (int q = 0; q < 3 * RPT; q++) jfac[q] = G_(jf)[q * NT + t];
  };
  auto b_products = [&](const uint64_t (&jfac)[3 * RPT]) {
#pragma unroll
    for (int q = 0; q < RPT; q++) {      // the three products under one reaction: nine factor reads in flight, then the stores (see a_products)
      double f0[3], f1[3], f2[3];
#pragma unroll
      for (int b = 0; b < 3; b++) {
        const uint64_t w = jfac[q * 3 + b];
        f0[b] = X[w & 0xFFFFu];
        f1[b] = X[(w >> 16) & 0xFFFFu];
        f2[b] = X[(w >> 32) & 0xFFFFu];
      }
#pragma unroll
      for (int b = 0; b < 3; b++) {
        double p = rct[q] * f0[b];
        p = p * f1[b];
        p = p * f2[b];
        JBp[(uint32_t)(jfac[q * 3 + b] >> 48)] = p;         // unused product slots write a spare cell: no branch
      }
    }
  };
  // Fun_x's sums land in the thread's own cells of XS (free here: the solves copy their result out before Fun runs again): species t
  // and, where a thread owns two (one wavefront per cell: NT = 64 < NVAR), t + NT.  A thread without a species, or whose second one
  // does not exist, parks that (empty) sum in the trash cell: the stride between a lane's outputs is per lane.
  // (the stream start-up sites: tot's placement of the ring only, see MISTRA_STREAM_* above)
  constexpr bool kGsumBarrier = MISTRA_STREAM_GSUM_BARRIER && !MT::RING_LOW, kGsumChain = MISTRA_STREAM_GSUM_CHAIN && !MT::RING_LOW;
  constexpr bool kSweepBarrier = MISTRA_STREAM_SWEEP_BARRIER && !MT::RING_LOW;
  auto vdot_out = [&](uint32_t& addr, uint32_t& stride) {
    int tt = t;
    if constexpr (!RESIDENT) asm volatile("" : "+v"(tt));      // (derived here: kept across the step loop, the stride was one more register stored to scratch per step)
    constexpr uint32_t trash = 8u * (uint32_t)(NNZ + NVAR + 2);
    addr = tt < NVAR ? 8u * (uint32_t)(NNZ + tt) : trash;
    if constexpr (kGsumPass) {      // a chained species: its wave's pass writes XS[s], the owner's (empty) sum must not land on it
      static_assert(!kGsumPass || SPT == 1, "chain passes: one species per lane");
      if (((lane < 32 ? hdr.mask_lo : hdr.mask_hi) >> (lane & 31)) & 1u) addr = trash;
    }
    if constexpr (SPT == 1) stride = tt < NVAR ? 8u * (uint32_t)NT : 0u;
    else stride = tt + NT < NVAR ? 8u * (uint32_t)NT : trash - addr;
  };
  auto vdot_sums = [&](auto barrier_tag) {      // barrier: in place of the lds_barrier() in front
    uint32_t addr, stride;
    vdot_out(addr, stride);
    if constexpr (kGsumPass) {
      if (hdr.pass_rows > 0) {      // (wave-uniform) the passes first, the barrier inside them; then this wave's rows, if it has any
        gsum_pass_run<NT, decltype(barrier_tag)::value ? 1 : 0, MT::RING_LOW>(a.vdot_pass, hdr.pass_row0, hdr.pass_rows, lane);
        if (hdr.vdot_rows > 0) gsum_run<NT, MT::RING_LOW>(a.vdot, hdr.vdot_row0, hdr.vdot_rows, lane, addr, stride);
        return;
      }
    }
    if constexpr (decltype(barrier_tag)::value) gsum_run_bar<NT, MT::RING_LOW>(a.vdot, hdr.vdot_row0, hdr.vdot_rows, lane, addr, stride);
    else gsum_run<NT, MT::RING_LOW>(a.vdot, hdr.vdot_row0, hdr.vdot_rows, lane, addr, stride);
  };
  auto read_vdot = [&](double (&out)[SPT]) {
#pragma unroll
    for (int q = 0; q < SPT; q++) {
      const int s = q * NT + t;
      out[q] = s < NVAR ? XS[s] : 0.0;
    }
  };
  // Jac_SP_x's sums land in this thread's own cells of the Ghimj area (free here: ros_PrepareMatrix rebuilds it from jac0)
  double jac0[JPT];
  auto jvs_sums = [&]() { gsum_run<NT, MT::RING_LOW>(a.jvs, hdr.jvs_row0, hdr.jvs_rows, lane, 8u * (uint32_t)t, 8u * (uint32_t)NT); };
  auto vdot_jvs_sums = [&]() {      // fun_jac's two programs as one call (gsum_run_pair)
    if constexpr (kGsumChain) {
      uint32_t addr, stride;
      vdot_out(addr, stride);
      if constexpr (kGsumPass) {
        if (hdr.pass_rows > 0) {      // (wave-uniform) the passes take the barrier, the pair enters without one
          gsum_pass_run<NT, kGsumBarrier ? 1 : 0, MT::RING_LOW>(a.vdot_pass, hdr.pass_row0, hdr.pass_rows, lane);
          gsum_run_pair<NT, 0, MT::RING_LOW>(a.vdot, hdr.vdot_row0, hdr.vdot_rows, addr, stride,
                                             a.jvs, hdr.jvs_row0, hdr.jvs_rows, 8u * (uint32_t)t, 8u * (uint32_t)NT, lane);
          return;
        }
      }
      gsum_run_pair<NT, kGsumBarrier ? 1 : 0, MT::RING_LOW>(a.vdot, hdr.vdot_row0, hdr.vdot_rows, addr, stride,
                                                    a.jvs, hdr.jvs_row0, hdr.jvs_rows, 8u * (uint32_t)t, 8u * (uint32_t)NT, lane);
    }
  };
  auto read_jvs = [&]() {
#pragma unroll
    for (int q = 0; q < JPT; q++) jac0[q] = M[q * NT + t];
  };

  auto fun = [&](const double (&v)[SPT], double (&out)[SPT]) {
    load_ffac();
    if constexpr (RCT_PER_USE) load_rct(true);
    store_x(v);
    wave_ref_put();
    lds_barrier();
    wave_ref_get(0);
    a_products();
    if constexpr (!kGsumBarrier) lds_barrier();      // (else: inside the sums' executor, behind its ring fill)
    lap(15);
    wave_stamp(0);
    vdot_sums(std::bool_constant<kGsumBarrier>{});
    wave_stamp(1);
    if constexpr (kGsumPass) lds_barrier();      // a chained species' owner reads a cell another wave wrote
    read_vdot(out);
  };
  auto jac = [&]() {
    uint64_t jfac[3 * RPT];
    load_jfac(jfac);
    if constexpr (RCT_PER_USE) load_rct(true);
    lds_barrier();   // every lane is done reading AB as A
    b_products(jfac);
    lds_barrier();
    lap(13);
    jvs_sums();
    lap(14);
    read_jvs();
  };
  // The step's first Fun_x and its Jac_SP_x in one go (both read the same V): the A and the B products are formed in ONE phase — the
  // B products have an array of their own inside the Ghimj area — and the two gather-sum programs run back to back.  Two
  // barrier phases and one table-stream start-up fewer per step than fun() followed by jac(); operation order inside every
  // product and sum unchanged.
  auto fun_jac = [&](const double (&v)[SPT], double (&out)[SPT]) {
    uint64_t jfac[3 * RPT];
    load_jfac(jfac);
    load_ffac();
    if constexpr (RCT_PER_USE) load_rct(true);
    store_x(v);
    wave_ref_put();
    lds_barrier();   // X is complete; nobody reads the Ghimj area any more (the last solve's sweeps are behind the error norm's barriers)
    wave_ref_get(1);
    a_products();
    b_products(jfac);
    if constexpr (!kGsumBarrier) lds_barrier();      // (else: inside the sums' executor, behind its ring fill)
    lap(13);
    wave_stamp(2);
    if constexpr (kGsumChain) {
      vdot_jvs_sums();
    } else {
      vdot_sums(std::bool_constant<kGsumBarrier>{});
      jvs_sums();      // (other cells, another source array: no barrier between)
    }
    wave_stamp(3);
    if constexpr (kGsumPass) lds_barrier();      // (as in fun)
    lap(14);
    read_vdot(out);
    read_jvs();
  };

  // ---- ros_PrepareMatrix_x (gas.f:1404), first half: Ghimj = -Jac0, diagonal += 1/(H*gamma).
  //      Returns (workgroup-uniform) whether a diagonal is exactly zero, the condition KppDecomp_x tests (gas.f:6157).
  auto prepare = [&](double ghinv, const double (&rhs)[SPT]) -> bool {
    if constexpr (!RESIDENT) load_pos();
    if (t == 0) { flags[0] = 0; flags[1] = 0x7fffffff; }
    lds_barrier();   // also: all readers of M from the previous attempt are done
#pragma unroll
    for (int q = 0; q < SPT; q++) {      // stage-1 right-hand side: the LU program forward-sweeps it while it factorises
      const int s = q * NT + t;
      if (s < NVAR) XS[s] = rhs[q];
    }
    // branch-free: a slot the thread does not have stores to the trash cell, the diagonal term is a select
    bool zero_diag = false;
    auto put = [&](uint32_t p, double minus_jac) {
      const bool none = p == kPosNone, dg = !none && (p & kPosDiag);
      const double vd = minus_jac + ghinv;
      const double v = dg ? vd : minus_jac;
      zero_diag |= dg && (v == 0.0);
      M[none ? (uint32_t)(NNZ + NVAR + 2) : (p & 0x7FFFu)] = v;
    };
#pragma unroll
    for (int q = 0; q < JPT; q++) {
      uint32_t pw = jpos[q / 2];
      asm volatile("" : "+v"(pw));        // unpack here, not hoisted into registers that live across the step loop
      put((q & 1) ? (pw >> 16) : (pw & 0xFFFFu), -jac0[q]);
    }
#pragma unroll
    for (int q = 0; q < ZPT; q++) {      // fill-in slots: -0.0.  A diagonal among them (a species whose rate does not depend on itself) sits in
      uint32_t pw = zpos[q / 2];          // slot 0 of its thread (schedule.cpp sorts them there): the other slots have nothing to select
      asm volatile("" : "+v"(pw));
      const uint32_t p = (q & 1) ? (pw >> 16) : (pw & 0xFFFFu);
      if (q == 0) put(p, scalar_const(-0.0));      // (formed in scalar registers here: as a hoisted vector-register pair the zero was the 128-register kernel's one spilled value)
      else M[p == kPosNone ? (uint32_t)(NNZ + NVAR + 2) : (p & 0x7FFFu)] = -0.0;
    }
    if (zero_diag) flags[0] = 1;
    lds_barrier();
    return flags[0] != 0;
  };

  // ---- KppSolve_x (gas.f:6206) on a register vector.  swept = true: XS already holds the forward-swept vector (the LU
  //      program carried the stage-1 right-hand side through the elimination), only the backward half is left.
  // the tail chain (one wave).  SWEPT: the forward half is done already (stage 1: inside the LU program), up to the dense block's own
  // columns where the mechanism has one
  auto tail = [&](auto swept_tag) {
    constexpr bool SWEPT = decltype(swept_tag)::value;
    constexpr uint32_t xs_tail = 8u * (NNZ + NVAR - 64 * MT::TAIL_REGS), r_tail = 8u * (NNZ + NVAR + 4 + NVAR - 64 * MT::TAIL_REGS);
    static_assert(!MT::RING_LOW || (MT::TAIL_REGS == 1 && MT::DENSE_ND == 0),
                  "the low ring placement runs the block form with one tail register only (tail_block: no room below v64 for two operand sets)");
    if constexpr (MT::RING_LOW) {
      tail_solve<MT::TAIL_REGS, SWEPT ? 4 * MT::TAIL_REGS : 0, true>(a.tail, xs_tail, r_tail, lane);
    } else {
      tail_solve<MT::TAIL_REGS, !SWEPT ? 0 : MT::DENSE_ND ? 4 * (MT::TAIL_REGS - 1) : 4 * MT::TAIL_REGS, false>(a.tail, xs_tail, r_tail, lane);
    }
  };
  auto solve = [&](double (&k)[SPT], bool swept) {
    for (int i = t; i < a.n_temps; i += NT) M[NNZ + 2 * NVAR + 4 + i] = 0.0;         // partial-sum cells of the head sweeps
    if (!swept) {
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + t;
        if (s < NVAR) XS[s] = k[q];
      }
      if constexpr (!kSweepBarrier) lds_barrier();      // (else: inside the sweep's executor, behind its ring fill)
      lap(6);
      vm_run<NT, 4, kVmSweepUpdPerRec, kSweepBarrier>(a.solve_head_fwd, hdr.fwd_row0, lane);                           // head rows, all waves
      lap(8);
      if (wave == 0)                                                                         // tail chain, one wave
        tail(std::false_type{});
    } else {
      lap(6);
      if (wave == 0)      // with the dense tail block the forward chain still has the block's own columns to do
        tail(std::true_type{});
    }
    if constexpr (!kSweepBarrier) lds_barrier();
    lap(9);
    vm_run<NT, 4, kVmSweepUpdPerRec, kSweepBarrier>(a.solve_head_bwd, hdr.bwd_row0, lane);
    lap(10);
#pragma unroll
    for (int q = 0; q < SPT; q++) {
      const int s = q * NT + t;
      if (s < NVAR) k[q] = XS[s];
    }
  };

  // VARIANT 4 (the step-control trace): the largest term of the error norm's sum and its species (1-based; 0: no term is positive), found
  // inside the norm's own reduction — per thread, per wave as (value, index), across waves through 2*NW cells behind L::TOTAL (the trace
  // launcher sizes them) written where the partial sums are written.  Ties go to the lowest species, a NaN term never wins (no comparison
  // with it holds).  No barrier is added and nothing here feeds Err.
  [[maybe_unused]] double tr_val = 0.0;
  [[maybe_unused]] int tr_idx = 0;
  [[maybe_unused]] int tr_halved = 0;    // decompositions of the current attempt that returned a zero pivot.  (Declared here, not in the attempt's
                                         // own scope: a declaration there, unused, changed the product kernels' instructions.)
  [[maybe_unused]] int ctrl_r[SPT];      // attempts this thread's species controlled: stored once, at exit
  // VARIANT 9 (the replay): the number of steps in the cell's row and the step in progress.  (Declared here, not inside the legs' loop: a declaration
  // there, unused, changed the series kernels' instructions.)
  [[maybe_unused]] int rp_n = 0, rp_i = 0;
  if constexpr (TRACE) {
#pragma unroll
    for (int q = 0; q < SPT; q++) ctrl_r[q] = 0;
  }
  // ---- ros_ErrorNorm_x (gas.f:1341): wave shuffle reduction, then the NW partial sums in a fixed order
  auto error_norm = [&](const double (&y0)[SPT], const double (&y1)[SPT], const double (&ye)[SPT]) -> double {
    double part = 0.0;
    [[maybe_unused]] double tv = 0.0;
    [[maybe_unused]] int ti = 0;
#pragma unroll
    for (int q = 0; q < SPT; q++) {
      const int s = q * NT + t;
      if (s < NVAR) {
        const double ymax = fmax_f(fabs(y0[q]), fabs(y1[q]));
        double scale;
        if constexpr (OPT) scale = atol_r[q] + rtol_r[q] * ymax;      // AbsTol(i) + RelTol(i)*Ymax (gas.f:1361)
        else scale = 1.0e-25 + 1.0e-3 * ymax;
        const double e = ye[q] / scale;
        part = part + e * e;
        if constexpr (TRACE) {
          const double term = e * e;
          if (term > tv) { tv = term; ti = s + 1; }      // q ascending: the thread's lowest species keeps a tie
        }
      }
    }
    part = wave_sum(part);
    if constexpr (TRACE) {
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {      // both partners of a pair choose the same one: every lane ends with the wave's
        const double ov = __shfl_xor(tv, m);
        const int oi = __shfl_xor(ti, m);
        if (ov > tv || (ov == tv && oi < ti)) { tv = ov; ti = oi; }
      }
    }
    lds_barrier();   // red[] may still be read from the previous step
    {
      int wv = wave;
      asm volatile("" : "+v"(wv));      // (the cell's address is formed here: kept across the step loop it was one more spilled register)
      if (lane == 0) red[wv] = part;
      if constexpr (TRACE) {
        if (lane == 0) {
          lds[L::TOTAL + wv] = tv;
          lds[L::TOTAL + NW + wv] = (double)ti;
        }
      }
    }
    lds_barrier();
    if constexpr (TRACE) {
      tr_val = 0.0;
      tr_idx = 0;
#pragma unroll
      for (int w = 0; w < NW; w++) {
        const double ov = lds[L::TOTAL + w];
        const int oi = (int)lds[L::TOTAL + NW + w];
        if (ov > tr_val || (ov == tr_val && oi < tr_idx)) { tr_val = ov; tr_idx = oi; }
      }
    }
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < NW; w++) sum += red[w];
    return sqrt(sum / (double)NVAR);
  };

  // ---- VARIANT 8, the operators: the pieces above run once at the state the caller gave, and the kernel returns.  Fun_x (with
  //      Jac_SP_x where the Jacobian or a solve is wanted: the evaluators a step opens with), Vdot and JVS to the caller's arrays, then
  //      ros_PrepareMatrix_x's matrix with the caller's shift in place of 1/(H*gamma), KppDecomp_x as the step loop runs it, and one KppSolve_x per
  //      right-hand side.  The cell's own Fun_x (a.ops_fun_rhs) rides through the LU program as a step's stage 1 does, so that row is K(1) of a step
  //      with that matrix bit for bit; every caller row goes through the full solve (solve(k, false)) and so does not depend on where it stands or
  //      on what else the call asks for.
  if constexpr (OPS) {
    const bool want_solve = a.ops_x != nullptr, want_jac = want_solve || a.ops_jvs != nullptr;
    double f0[SPT];
    if (want_jac) {
      if constexpr (L::MERGE_FUN_JAC) {
        fun_jac(y, f0);
      } else {
        fun(y, f0);
        jac();
      }
    } else {
      fun(y, f0);
    }
    if (a.ops_vdot) {
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + t;
        if (s < NVAR) GM_(a.ops_vdot)[(size_t)cell * NVAR + s] = f0[q];
      }
    }
    if (a.ops_jvs) {      // every slot of the row once: the thread's sums to their Ghimj slots, the fill-in slots +0.0
      if constexpr (!RESIDENT) load_pos();
      gptr_mut<double> jrow = GM_(a.ops_jvs) + (size_t)cell * NNZ;
#pragma unroll
      for (int q = 0; q < JPT; q++) {
        const uint32_t pw = jpos[q / 2], p = (q & 1) ? (pw >> 16) : (pw & 0xFFFFu);
        if (p != kPosNone) jrow[p & 0x7FFFu] = jac0[q];
      }
#pragma unroll
      for (int q = 0; q < ZPT; q++) {
        const uint32_t pw = zpos[q / 2], p = (q & 1) ? (pw >> 16) : (pw & 0xFFFFu);
        if (p != kPosNone) jrow[p & 0x7FFFu] = 0.0;
      }
    }
    if (!want_solve) return;      // (uniform over the call)
    const int nrow = (a.ops_fun_rhs ? 1 : 0) + a.ops_nrhs;
    double kk[SPT];
#pragma unroll
    for (int q = 0; q < SPT; q++) kk[q] = f0[q] + 0.0;      // K1's right-hand side as the step loop forms it (Fcn0 + HG*dFdT, dFdT = +0.0)
    const double shift = wave_uniform(G_(a.ops_shift)[(size_t)cell * (size_t)a.ops_shift_stride]);
    if (prepare(shift, kk)) {
      // KppDecomp_x's IER: the first row whose diagonal is exactly zero as prepared (see the step loop's singular path).  No factorisation runs:
      // the cell's rows are +0.0
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int sp = q * NT + t;
        const uint32_t dp = sp < NVAR ? (uint32_t)G_(a.diag_pos)[sp] : (uint32_t)kPosNone;
        if (dp != kPosNone && M[dp] == 0.0) atomicMin(&flags[1], sp + 1);
      }
      lds_barrier();
      if (t == 0) GM_(a.ops_ising)[cell] = flags[1];
      for (int j = 0; j < nrow; j++) {
#pragma unroll
        for (int q = 0; q < SPT; q++) {
          const int s = q * NT + t;
          if (s < NVAR) GM_(a.ops_x)[(int64_t)j * a.ops_x_block + (int64_t)cell * NVAR + s] = 0.0;
        }
      }
      return;
    }
    if (t == 0) GM_(a.ops_ising)[cell] = 0;
    vm_run<NT, 4>(a.lu, hdr.lu_row0, lane);
    if constexpr (MT::SCALE_PASS) {
      scale_run<NT, MT::RING_LOW>(a.lu_scale, wave, lane);
      lds_barrier();
    }
    if constexpr (MT::DENSE_ND > 0) {
      const f64x4 tile = dense_lu<MT, NT>(lane);
      if (wave == 7) dense_finish<MT, NT>(tile, lane);
      lds_barrier();
    }
    int row = 0;
    if (a.ops_fun_rhs) {      // its forward sweep went through the LU program
      solve(kk, true);
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + t;
        if (s < NVAR) GM_(a.ops_x)[(int64_t)cell * NVAR + s] = kk[q];
      }
      row = 1;
    }
    for (int j = 0; j < a.ops_nrhs; j++) {
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + t;
        kk[q] = s < NVAR ? G_(a.ops_rhs)[(int64_t)j * a.ops_rhs_block + (int64_t)cell * NVAR + s] : 0.0;
      }
      solve(kk, false);
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + t;
        if (s < NVAR) GM_(a.ops_x)[(int64_t)(row + j) * a.ops_x_block + (int64_t)cell * NVAR + s] = kk[q];
      }
    }
    return;
  }

  // ---- RosenbrockIntegrator_x (gas.f:1180-1336); option values are the ones INTEGRATE_x/Rosenbrock_x fix
  // VARIANT 5: Tstart, Tend and what follows from them (Hmax, Direction) are the leg's, set at the head of each leg (below)
  double Tstart = a.tin, Tend = a.tout;
  const double Roundoff = 2.220446049250313e-16, Hmin = 0.0;
  double Hmax = wave_uniform(fabs(Tend - Tstart));
  const double FacMin = 0.2, FacMax = 6.0, FacRej = 0.1, FacSafe = 0.9;
  // VARIANT 3: the same seven out of the options block, fetched where they are used
  auto hmin = [&]() -> double { if constexpr (OPT) return opt(kOptHmin); else return Hmin; };
  auto hmax = [&]() -> double { if constexpr (OPT) return fmin_f(opt(kOptHmax), Hmax); else return Hmax; };      // MIN(RPAR(2), ABS(Tend-Tstart)) (gas.f:989)
  auto facmin = [&]() -> double { if constexpr (OPT) return opt(kOptFacMin); else return FacMin; };
  auto facmax = [&]() -> double { if constexpr (OPT) return opt(kOptFacMax); else return FacMax; };
  auto facrej = [&]() -> double { if constexpr (OPT) return opt(kOptFacRej); else return scalar_const(FacRej); };
  auto facsafe = [&]() -> double { if constexpr (OPT) return opt(kOptFacSafe); else return FacSafe; };
  double Direction = (Tend >= Tstart) ? 1.0 : -1.0;
  // Hstart: INTEGRATE_x fixes RPAR(3) = 1e-3 (gas.f:743).  Opt-in departure from the reference: a caller that keeps
  // each cell's last step size from one chemistry timestep to the next passes it in a.hstart; <= 0 means the reference's value.
  // VARIANT 3: RPAR(3) as resolved by the host (gas.f:996-999) in its place; a per-cell a.hstart > 0 still goes first.
  double hstart_call = 1.0e-3;
  if constexpr (OPT) hstart_call = opt(kOptHstart);
  double hstart0 = (a.hstart && G_(a.hstart)[cell] > 0.0) ? G_(a.hstart)[cell] : hstart_call;
  // The step size H lives across the whole step loop, and the compiler carried a vector-register copy of it (and of Hexit) around
  // the loop through scratch: 8-16 bytes per lane and step, stored through to HBM — most of aer's memory traffic in rounds 2 and 3.
  // So it lives in LDS: one cell per wave behind the error norm's partial sums, written by the wave's lane 0 and read back by the
  // same wave (LDS operations of a wave complete in order: no barrier is involved); every use below fetches it afresh.  Hexit, which
  // only thread 0 needs when the integrator returns, sits in the last cell of that block.
  auto Hget = [&]() -> double {
    int wv = wave;
    asm volatile("" : "+v"(wv));
    return wave_uniform(*(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_H + wv)));
  };
  auto Hset = [&](double v) {
    int wv = wave;
    asm volatile("" : "+v"(wv));
    if (lane == 0) *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_H + wv)) = v;
  };
  static_assert(NW <= L::RED_H && L::RED_H + NW <= L::RED_HEXIT, "red[]: partial sums | H per wave | Hexit");
  // VARIANT 10: the next evaluation reads the rate constants at tau = T + alpha*dh (ros_Alpha(i)*Direction*H behind the step's T): its place in the leg,
  // (tau - times[leg]) * w, each operation rounded on its own
  [[maybe_unused]] auto lin_stage = [&](double T, double alpha, double dh) {
#pragma clang fp contract(off)
    const double up = alpha * dh;
    const double tau = T + up;
    lin_s = wave_uniform((tau - Tstart) * lin_w);
  };
  // ---- the legs (VARIANT 5; one pass for every other variant).  The leg's bookkeeping is wave-uniform and stays in scalar registers: the leg index, the
  //      leg's two times (scalar loads out of the call's options block, which nothing writes while the kernel runs) and the offsets of its output blocks,
  //      formed where they are used.  Every per-call quantity of Rosenbrock_x starts afresh below.  Nothing is carried around the loop in a vector
  //      register: with a.carry_h the leg's first step is read from the Hexit cell, in LDS, before thread 0 resets it.
  do {
    if constexpr (SERIES) {
      const auto times = (const double __attribute__((address_space(4)))*)a.times;
      Tstart = times[leg];
      Tend = times[leg + 1];
      Hmax = wave_uniform(fabs(Tend - Tstart));
      Direction = (Tend >= Tstart) ? 1.0 : -1.0;
      if constexpr (LINR) lin_w = wave_uniform(1.0 / (Tend - Tstart));      // once per leg; the node blocks themselves are read per use (load_rct)
      if (leg > 0) {      // Rosenbrock_x called again: the options' Hstart and no per-cell value; a.carry_h: the previous leg's Hexit where it is > 0
        hstart0 = opt(kOptHstart);
        if (a.carry_h) {
          lds_barrier();      // thread 0's last store to the cell (a leg that made no step leaves only its reset, with no barrier behind it)
          const double hx =wave_uniform(*(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT)));
          if (hx > 0.0) hstart0 = hx;
          lds_barrier();      // every wave has read the cell before thread 0 resets it
        }
        // VARIANT 11: the previous leg ended on flux_close, which reads other threads' species out of X, and this leg's first Fun_x stores Y into X.  The
        // a.carry_h pair above and the a.leg_fix barrier below lie between the two; where the call has neither, this one does.
        if constexpr (SFLUX) {
          if (!a.carry_h && a.leg_fix == 0) lds_barrier();
        }
        // RCONST and FIX of the leg's own (a.leg_rconst / a.leg_fix /= 0, uniform over the call): what Update_RCONST_x left in front of this call of
        // Rosenbrock_x.  The per-use fetch out of global memory needs nothing here: load_rct forms the leg's base itself.
        if (!LINR && a.leg_rconst != 0) {
          if constexpr (L::RCT_IN_LDS) {      // the cell's copy in LDS: every thread rewrites the cells it reads back itself (r = q*NT + t): no barrier involved
            const double* rc = a.rconst + (int64_t)leg * a.leg_rconst;
#pragma unroll
            for (int q = 0; q < RPT; q++) {
              const int r = q * NT + t;
              if (r < NREACT) lds[L::RCT + r] = G_(rc)[(size_t)cell * NREACT + r];
            }
          } else if constexpr (!RCT_PER_USE) {      // resident registers (a lane whose r >= NREACT keeps 0.0)
            load_rct(false);
          }
        }
        if (a.leg_fix != 0) {      // other threads read these cells (the A and B products): the write goes behind a barrier that follows the previous
          if (!a.carry_h) lds_barrier();      // leg's last read of X (a.carry_h: its two, above) and in front of the one the leg's first Fun_x passes behind store_x
          if (t < NFIX) X[NVAR + t] = G_(a.fix + (int64_t)leg * a.leg_fix)[(size_t)cell * NFIX + t];
        }
      }
    }
    double T = Tstart;
    if (t == 0) *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT)) = 0.0;
    {
      double H0 = fmin_f(fmin_f(hstart0, fabs(Tend - Tstart)), hmax());
      if (fabs(H0) <= 10.0 * Roundoff) H0 = 1.0e-5;
      Hset(H0);
    }
    // VARIANT 6: the running sum and A(r) at the last accepted state of this thread's reactions (thread-private: r = q*NT + t in every step), half the
    // signed size of the accepted step that is still open (its end state's A is formed by the next step's first Fun_x, or behind the loop)
    [[maybe_unused]] double fl_sum[RPT], fl_prev[RPT];
    [[maybe_unused]] double fl_half = 0.0;
    [[maybe_unused]] bool fl_open = false;
    if constexpr (FLUX) {
#pragma unroll
      for (int q = 0; q < RPT; q++) { fl_sum[q] = 0.0; fl_prev[q] = 0.0; }
    }
    [[maybe_unused]] auto flux_close = [&]() {      // X holds the state the open step ended on (or, with none open, the call's first state)
      double pa[RPT];
      flux_products(pa);
#pragma unroll
      for (int q = 0; q < RPT; q++) {
        if (fl_open) fl_sum[q] = fl_sum[q] + fl_half * (fl_prev[q] + pa[q]);
        fl_prev[q] = pa[q];
      }
      fl_open = false;
    };
    // VARIANT 7: Y_n and F_n of this thread's species and T_n, dh of the accepted step that is still open (its end state's F is the next step's fcn0, or
    // formed behind the loop), and the number of samples taken so far, uniform over the workgroup.  dense_take evaluates the samples of the open step
    // while y and f1 hold Y_{n+1}, F_{n+1}: in order, every one with Direction*(ts[k] - T) <= 0, T being T_{n+1} (all: every one left).  The operations
    // and their order are the definition's, each rounded once.  One coalesced [NVAR] row per sample; ts by scalar loads.
    [[maybe_unused]] double dn_y0[SPT], dn_f0[SPT];
    [[maybe_unused]] double dn_t0 = 0.0, dn_dh = 0.0;
    [[maybe_unused]] bool dn_open = false;
    [[maybe_unused]] int dn_k = 0;
    [[maybe_unused]] auto dense_take = [&](const double (&f1)[SPT], double Tn1, bool all) {
      const auto ts = (const double __attribute__((address_space(4)))*)a.times;
      while (dn_k < a.dense_ns) {
        const double tk = ts[dn_k];
        if (!all && !(Direction * (tk - Tn1) <= 0.0)) break;
        const double th = wave_uniform((tk - dn_t0) / dn_dh);
        const double om = 1.0 - th, e = 1.0 - 2.0 * th, w = th * om;
#pragma unroll
        for (int q = 0; q < SPT; q++) {
          const int s = q * NT + t;
          const double d = y[q] - dn_y0[q], hf0 = dn_dh * dn_f0[q], hf1 = dn_dh * f1[q];
          const double c = (e * d - om * hf0) + th * hf1;
          const double u = (om * dn_y0[q] + th * y[q]) - w * c;
          if (s < NVAR) GM_(a.dense_out)[(int64_t)dn_k * a.dense_block + (int64_t)cell * NVAR + s] = u;
        }
        dn_k += 1;
      }
      dn_open = false;
    };
    bool RejectLastH = false, RejectMoreH = false;
    int nfun = 0, njac = 0, nstp = 0, nacc = 0, nrej = 0, ndec = 0, nsol = 0, nsng = 0;
    int ierr = 1;

    double ynew[SPT], fcn0[SPT], fcn[SPT], k1[SPT], k2[SPT], k3[SPT], yerr[SPT];
    [[maybe_unused]] double k4[SPT], k5[SPT], k6[SPT];      // the method kernels' further stage vectors (Ros4, Rodas3: k4; Rodas4: k4..k6)
    [[maybe_unused]] double dfdt[SPT];                      // VARIANT 10: the step's dFdT, live from its evaluation to the last stage
    // stage vector J (0-based) by its compile-time number: named register arrays, never an array indexed at run time (that one would live in scratch)
    [[maybe_unused]] auto stage_k = [&](auto J) -> double (&)[SPT] {
      constexpr int j = decltype(J)::value;
      static_assert(j >= 0 && j < 6, "stage vector");
      if constexpr (j == 0) return k1;
      else if constexpr (j == 1) return k2;
      else if constexpr (j == 2) return k3;
      else if constexpr (j == 3) return k4;
      else if constexpr (j == 4) return k5;
      else return k6;
    };

    // VARIANT 9: the cell's row of step sizes and its count (a.replay_h_stride = 0: one row shared by all cells, behind the call's options block, read by
    // scalar loads as a series reads its times; else the cell's own row and count, a count above the capacity clamped to it).  The H cell of each wave
    // holds the step in progress, the Hexit cell the last step TAKEN: both start at 0, the second is written at acceptance.
    if constexpr (REPLAY) {
      const bool own = a.replay_h_stride != 0;
      rp_n = __builtin_amdgcn_readfirstlane(G_(a.replay_n)[own ? cell : 0]);
      if (rp_n > a.replay_cap) rp_n = a.replay_cap;
      Hset(0.0);
    }
    while (REPLAY ? rp_i < rp_n : fabs(Tend - T) >= Roundoff) {
      if constexpr (REPLAY) {      // no clipping to Tend, no Max_no_steps; the -7 test as written
        double H;
        if (a.replay_h_stride != 0) H = wave_uniform(G_(a.replay_h + (int64_t)cell * a.replay_h_stride)[rp_i]);
        else H = ((const double __attribute__((address_space(4)))*)a.replay_h)[rp_i];
        if (((T + scalar_const(0.1) * H) == T) || (H <= Roundoff)) { ierr = -7; break; }
        Hset(H);
      } else {
        if (nstp > a.max_steps) { ierr = -6; break; }      // Max_no_steps: 100000 (gas.f:1042, 1199)
        const double H = Hget();
        if (((T + scalar_const(0.1) * H) == T) || (H <= Roundoff)) { ierr = -7; break; }
        if (t == 0) *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT)) = H;
        Hset(fmin_f(H, fabs(Tend - T)));
      }

      lap(6);
      if constexpr (!RESIDENT) {      // (Jac_SP below defines every entry.  Said here with an empty statement that "writes" them, so that no value — not even an
#pragma unroll                     //  undefined one — is carried around the step loop: the 128-register kernels carried one through scratch)
        for (int q = 0; q < JPT; q++) asm volatile("" : "=v"(jac0[q]));
      }
      if constexpr (LINR) lin_stage(T, 0.0, 0.0);      // Fcn0 and Jac0 read R(T)
      if constexpr (L::MERGE_FUN_JAC) {
        fun_jac(y, fcn0);
        dump_vec(0, fcn0);
      } else {
        fun(y, fcn0);
        dump_vec(0, fcn0);
        lap(0);
        jac();
      }
      // VARIANT 10: dFdT = Fun(Y, FIX, dR/dt), the exact time derivative (Fun is linear in the rate constants, they are linear in the time): the Fun call
      // ros_FunTimeDerivative_x makes, counted below as KPP counts it; not made where the call is autonomous.  Jac0 is in registers by now.
      if constexpr (LINR) {
        if (!autonomous) {
          lin_dot = true;
          fun(y, dfdt);
          lin_dot = false;
        } else {
#pragma unroll
          for (int q = 0; q < SPT; q++) dfdt[q] = 0.0;
        }
      }
      if constexpr (FLUX) flux_close();      // X is Y_n until stage 2 stores into it, behind ros_PrepareMatrix's barriers
      if constexpr (DENSE) {
        if (dn_open) dense_take(fcn0, T, false);
      }
      // ros_FunTimeDerivative_x (gas.f:1375): Fun_x does not depend on T and RCONST is frozen, so
      // dFdT = (1/Delta)*(Fun - Fcn0) is an exact +0.0; the evaluation is skipped, its count and its "+ HG*0.0" are kept.
      if constexpr (OPT) nfun += autonomous ? 1 : 2;      // Autonomous: no ros_FunTimeDerivative_x, no Fun call of its own (gas.f:1221)
      else nfun += 2;
      njac += 1;
      lap(1);

      bool accepted = false;
      while (!accepted) {
        if constexpr (TRACE) tr_halved = 0;
        {
          // K1's right-hand side, Fcn0 + HG*dFdT with dFdT = +0.0 (see above); independent of H
#pragma unroll
          for (int q = 0; q < SPT; q++) {
            if constexpr (LINR) continue;      // (formed inside the loop below)
            if constexpr (METHOD != kRos3) k1[q] = autonomous ? fcn0[q] : fcn0[q] + Direction * 0.0;      // (Direction*H*Gamma(1))*dFdT: a zero of Direction's sign (Gamma(1) > 0 in all five)
            else if constexpr (OPT) k1[q] = autonomous ? fcn0[q] : fcn0[q] + 0.0;      // Autonomous: the HG*dFdT terms are not added at all (gas.f:1268)
            else k1[q] = fcn0[q] + 0.0;
          }
          int nconsecutive = 0;
          bool singular = true;
          while (singular) {
            if constexpr (LINR) {      // K1's right-hand side with its HG*dFdT term: it follows H through ros_PrepareMatrix_x's halvings
              const double hg = wave_uniform((Direction * Hget()) * kGamma1);
#pragma unroll
              for (int q = 0; q < SPT; q++) k1[q] = autonomous ? fcn0[q] : fcn0[q] + hg * dfdt[q];
            }
            const double ghinv = wave_uniform(1.0 / (Direction * Hget() * kGamma1));
            singular = prepare(ghinv, k1);
            dump_matrix(NVAR);      // Ghimj = 1/(H*gamma) - Jac0
            ndec += 1;
            lap(2);
            if (singular) {
              // which row: KppDecomp_x returns the FIRST row whose diagonal is exactly zero as it reaches it (IER = k, gas.f:6157 — rows are
              // untouched until their own turn, so the test sees the prepared value); ros_PrepareMatrix_x prints it (gas.f:1456).  Rare
              // path: Ghimj is still as prepared (no LU ran), every species' thread looks at its diagonal slot.
              if (a.sing_rows && nsng < 8) {
#pragma unroll
                for (int q = 0; q < SPT; q++) {      // every species' thread looks at its diagonal slot(s)
                  const int sp = q * NT + t;
                  const uint32_t dp = sp < NVAR ? (uint32_t)G_(a.diag_pos)[sp] : (uint32_t)kPosNone;
                  if (dp != kPosNone && M[dp] == 0.0) atomicMin(&flags[1], sp + 1);
                }
                lds_barrier();
                if (t == 0) GM_(a.sing_rows)[(size_t)cell * 8 + nsng] = flags[1];
              }
              lds_barrier();   // everyone has read flags[0] (and flags[1]) before the retry clears them
              nsng += 1;
              nconsecutive += 1;
              if constexpr (TRACE) tr_halved += 1;
              if constexpr (REPLAY) { ierr = -8; break; }      // a prescribed step is not halved: the cell leaves at the last accepted state
              if (nconsecutive <= 5) Hset(Hget() * 0.5);
              else { ierr = -8; break; }
            } else {
              vm_run<NT, 4>(a.lu, hdr.lu_row0, lane);
              if constexpr (MT::SCALE_PASS) {      // else the scaling is the LU program's last round
                lap(3);
                scale_run<NT, MT::RING_LOW>(a.lu_scale, wave, lane);      // L(k,j) *= R(j); tail block: U(i,c) *= R(i)
                lds_barrier();
                lap(11);
              }
              if constexpr (MT::DENSE_ND > 0) {
                static_assert(MT::SCALE_PASS, "the Schur steps read what the scaling pass leaves");
                lap(3);
                const f64x4 tile = dense_lu<MT, NT>(lane);      // tile (3,3) of the block with pivots 0 .. 47 applied, in wave 7
                if (wave == 7) dense_finish<MT, NT>(tile, lane);
                lds_barrier();
                lap(12);
              }
              lap(3);
              if constexpr (DUMP) {
                if (MT::DENSE_ND == 0) lds_barrier();      // (the dense tail's caller has just passed one)
                dump_matrix(NVAR + NNZ);      // the factors as the kernel keeps them; R(k) = 1/U(k,k) behind them
                if (dumping)
                  for (int i = t; i < NVAR; i += NT) dump[NVAR + 2 * NNZ + i] = M[NNZ + NVAR + 4 + i];
              }
            }
          }
          if (ierr == -8) break;
        }
        const double dh = wave_uniform(Direction * Hget());
        // stage 1: its right-hand side went through the LU program above, only the backward half of the solve is left
        lap(6);
        solve(k1, true);
        dump_vec(2 * NVAR + 2 * NNZ, k1);
        lap(4);
        if constexpr (METHOD == kRos3) {
          // stage 2: new function value at Y + A21*K1
#pragma unroll
          for (int q = 0; q < SPT; q++) ynew[q] = y[q] + kRosA1 * k1[q];
          lap(6);
          if constexpr (LINR) lin_stage(T, kRosAlpha<kRos3>.Alpha[1], dh);      // ros_Alpha(2) = gamma (Ros3_x); stage 3 reuses the value
          fun(ynew, fcn);
          lap(0);
          nfun += 1;
          {
            const double hc = wave_uniform(kRosC1 / dh);
#pragma unroll
            for (int q = 0; q < SPT; q++) {
              if constexpr (LINR) k2[q] = autonomous ? fcn[q] + hc * k1[q] : (fcn[q] + hc * k1[q]) + wave_uniform(dh * kRosGamma2) * dfdt[q];      // (a declaration of HG in this block changed the other kernels' instructions)
              else if constexpr (OPT) k2[q] = autonomous ? fcn[q] + hc * k1[q] : (fcn[q] + hc * k1[q]) + dh * 0.0;
              else k2[q] = (fcn[q] + hc * k1[q]) + dh * 0.0;      // + HG*dFdT with dFdT = +0.0: (dh*gamma2)*0.0, a zero of dh's sign (gamma2 > 0)
            }
          }
          lap(6);
          solve(k2, false);
          dump_vec(3 * NVAR + 2 * NNZ, k2);
          lap(4);
          // stage 3 reuses the stage-2 function value
          {
            const double hc1 = wave_uniform(kRosC2 / dh), hc2 = wave_uniform(kRosC3 / dh);
#pragma unroll
            for (int q = 0; q < SPT; q++) {
              if constexpr (LINR) k3[q] = autonomous ? (fcn[q] + hc1 * k1[q]) + hc2 * k2[q] : ((fcn[q] + hc1 * k1[q]) + hc2 * k2[q]) + wave_uniform(dh * kRosGamma3) * dfdt[q];
              else if constexpr (OPT) k3[q] = autonomous ? (fcn[q] + hc1 * k1[q]) + hc2 * k2[q] : ((fcn[q] + hc1 * k1[q]) + hc2 * k2[q]) + dh * 0.0;
              else k3[q] = ((fcn[q] + hc1 * k1[q]) + hc2 * k2[q]) + dh * 0.0;      // (dh*gamma3)*0.0 likewise (gamma3 > 0)
            }
          }
          lap(6);
          solve(k3, false);
          dump_vec(4 * NVAR + 2 * NNZ, k3);
          lap(4);
          nsol += 3;
#pragma unroll
          for (int q = 0; q < SPT; q++) {
            ynew[q] = ((y[q] + kRosM1 * k1[q]) + kRosM2 * k2[q]) + kRosM3 * k3[q];
            yerr[q] = ((0.0 + kRosE1 * k1[q]) + kRosE2 * k2[q]) + kRosE3 * k3[q];
          }
        } else {
          // ---- the method kernels: stages 2 .. ros_S (gas.f:1241-1276), unrolled at compile time, in the reference's order of operations.
          //      WAXPY_x returns at once for a zero coefficient (gas.f:6641): such a term is dropped, not multiplied out.
          auto for_stages = [&](auto&& f, auto FROM, auto TO) {      // f(integral_constant<int, FROM>) ... f(integral_constant<int, TO - 1>)
            auto go = [&](auto&& self, auto I) {
              if constexpr (decltype(I)::value < decltype(TO)::value) {
                f(I);
                self(self, std::integral_constant<int, decltype(I)::value + 1>{});
              }
            };
            go(go, FROM);
          };
          for_stages([&](auto I) {
            constexpr int i = decltype(I)::value;      // stage i + 1
            constexpr int row = i * (i - 1) / 2;       // A(i+1, j+1) = ros_A[row + j]
            if constexpr (kRosMethod<METHOD>.NewF[i]) {
#pragma unroll
              for (int q = 0; q < SPT; q++) ynew[q] = y[q];
              for_stages([&](auto J) {
                constexpr double aij = kRosMethod<METHOD>.A[row + decltype(J)::value];
                if constexpr (aij != 0.0) {
                  const double (&kj)[SPT] = stage_k(J);
#pragma unroll
                  for (int q = 0; q < SPT; q++) ynew[q] = ynew[q] + aij * kj[q];
                }
              }, std::integral_constant<int, 0>{}, I);
              lap(6);
              if constexpr (LINR) lin_stage(T, kRosAlpha<METHOD>.Alpha[i], dh);
              fun(ynew, fcn);
              lap(0);
              nfun += 1;
            }
            // Fcn: the last function value formed, Fcn0 while no stage of this step has formed one (Rodas3's stage 2)
            constexpr bool fresh = ros_fresh_fcn(METHOD, i);
            double (&ki)[SPT] = stage_k(I);
#pragma unroll
            for (int q = 0; q < SPT; q++) ki[q] = fresh ? fcn[q] : fcn0[q];
            for_stages([&](auto J) {
              constexpr double cij = kRosMethod<METHOD>.C[row + decltype(J)::value];
              if constexpr (cij != 0.0) {
                const double hc = wave_uniform(cij / dh);
                const double (&kj)[SPT] = stage_k(J);
#pragma unroll
                for (int q = 0; q < SPT; q++) ki[q] = ki[q] + hc * kj[q];
              }
            }, std::integral_constant<int, 0>{}, I);
            constexpr double gi = kRosMethod<METHOD>.Gamma[i];
            if constexpr (gi != 0.0) {      // + HG*dFdT with dFdT = +0.0: a zero with the sign of Direction*H*Gamma(i); nothing where Gamma(i) = 0 or autonomous (gas.f:1268)
              const double hg0 = wave_uniform(LINR ? dh * gi : (dh * gi) * 0.0);      // (VARIANT 10: HG itself, its dFdT is not a zero)
#pragma unroll
              for (int q = 0; q < SPT; q++) ki[q] = autonomous ? ki[q] : ki[q] + (LINR ? hg0 * dfdt[q] : hg0);
            }
            lap(6);
            solve(ki, false);
            lap(4);
          }, std::integral_constant<int, 1>{}, std::integral_constant<int, kRosMethod<METHOD>.S>{});
          { constexpr int S = kRosMethod<METHOD>.S; nsol += S; }
#pragma unroll
          for (int q = 0; q < SPT; q++) { ynew[q] = y[q]; yerr[q] = 0.0; }
          for_stages([&](auto J) {
            constexpr double mj = kRosMethod<METHOD>.M[decltype(J)::value], ej = kRosMethod<METHOD>.E[decltype(J)::value];
            const double (&kj)[SPT] = stage_k(J);
            if constexpr (mj != 0.0) {
#pragma unroll
              for (int q = 0; q < SPT; q++) ynew[q] = ynew[q] + mj * kj[q];
            }
            if constexpr (ej != 0.0) {
#pragma unroll
              for (int q = 0; q < SPT; q++) yerr[q] = yerr[q] + ej * kj[q];
            }
          }, std::integral_constant<int, 0>{}, std::integral_constant<int, kRosMethod<METHOD>.S>{});
        }
        lap(6);
        const double Err = error_norm(y, ynew, yerr);
        if constexpr (DUMP) {
          if (dumping && t == 0) { dump[5 * NVAR + 2 * NNZ] = Err; dump[5 * NVAR + 2 * NNZ + 1] = Hget(); }
          dumping = false;      // the first attempt only
        }
        lap(5);
        if constexpr (REPLAY) {      // every attempt is accepted: Fac, the root and Hnew are not formed
          const double H = Hget();
          if (t == 0) {
            if (a.replay_err) GM_(a.replay_err)[(int64_t)cell * a.replay_cap + rp_i] = Err;
            *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT)) = H;
          }
          rp_i += 1;
          nstp += 1;
          nacc += 1;
#pragma unroll
          for (int q = 0; q < SPT; q++) y[q] = ynew[q];
          T = wave_uniform(T + dh);
          accepted = true;
          continue;
        }
        double root;
        if constexpr (METHOD != kRos3 && kRosMethod<METHOD>.ELO != kRosElo) {      // Err**(1/ros_ELO), ros_ELO = 2 or 4
          constexpr double inv_elo = 1.0 / kRosMethod<METHOD>.ELO;
          if constexpr (MT::WAVES_PER_SIMD > 2) root = err_root_elo(Err, inv_elo);
          else root = pow(Err, inv_elo);
        } else if constexpr (MT::WAVES_PER_SIMD > 2) root = err_root(Err);      // register-starved kernels: see err_root
        else root = pow(Err, 1.0 / kRosElo);
        const double Fac = fmin_f(facmax(), fmax_f(facmin(), facsafe() / root));
        const double H = Hget();
        double Hnew = H * Fac;
        nstp += 1;
        if constexpr (TRACE) {      // the attempt's record: T is still the step's start, H the step as attempted (after ros_PrepareMatrix_x's halvings)
          const bool acc = (Err <= 1.0) || (H <= hmin());
          if (t == 0 && nstp <= a.trace_cap) {
            const size_t r = (size_t)cell * (size_t)a.trace_cap + (size_t)(nstp - 1);
            gptr_mut<double> td = GM_(a.trace_d) + r * 4;
            td[0] = T; td[1] = H; td[2] = Err;
            td[3] = tr_idx > 0 ? tr_val / (((double)NVAR * Err) * Err) : 0.0;
            gptr_mut<int32_t> ti2 = GM_(a.trace_i) + r * 2;
            ti2[0] = tr_idx; ti2[1] = (acc ? 1 : 0) + 2 * tr_halved;
          }
#pragma unroll
          for (int q = 0; q < SPT; q++)
            if (tr_idx == q * NT + t + 1) ctrl_r[q] += 1;
        }
        if ((Err <= 1.0) || (H <= hmin())) {
          nacc += 1;
          if constexpr (DENSE) {      // the step opens: Y_n, F_n, T_n and the signed step
#pragma unroll
            for (int q = 0; q < SPT; q++) { dn_y0[q] = y[q]; dn_f0[q] = fcn0[q]; }
            dn_t0 = T; dn_dh = dh; dn_open = true;
          }
#pragma unroll
          for (int q = 0; q < SPT; q++) y[q] = ynew[q];
          T = wave_uniform(T + dh);
          Hnew = fmax_f(hmin(), fmin_f(Hnew, hmax()));
          if (RejectLastH) Hnew = fmin_f(Hnew, H);
          RejectLastH = false;
          RejectMoreH = false;
          Hset(Hnew);
          if constexpr (FLUX) { fl_half = 0.5 * dh; fl_open = true; }
          accepted = true;
        } else {
          if (RejectMoreH) Hnew = H * facrej();
          RejectMoreH = RejectLastH;
          RejectLastH = true;
          Hset(Hnew);
          if (nacc >= 1) nrej += 1;
        }
      }
      if (ierr < 0) break;
    }

    // VARIANT 6: the last accepted step is still open on a normal return and on -6 / -7 (on -8 the failing step's own Fun_x has closed it): one more
    // evaluation of the A products, at the state the call returns.  Not a Fun_x call, not counted.  fl_open is uniform over the workgroup; every read
    // of X by another thread lies in front of a barrier this thread has passed (the error norm's).
    if constexpr (FLUX) {
      if (fl_open) {
        load_ffac();
        if constexpr (RCT_PER_USE) load_rct(true);
        store_x(y);
        lds_barrier();
        flux_close();
      }
#pragma unroll
      for (int q = 0; q < RPT; q++) {
        const int r = q * NT + t;
        if constexpr (SFLUX) {      // the leg's row
          if (r < NREACT) GM_(a.flux)[(int64_t)leg * a.leg_flux + (int64_t)cell * NREACT + r] = fl_sum[q];
        } else {
          if (r < NREACT) GM_(a.flux)[(size_t)cell * NREACT + r] = fl_sum[q];
        }
      }
    }
    // VARIANT 7: the last accepted step is still open on a normal return and on -6 / -7 (on -8 the failing step's own Fun_x has closed it): one more Fun_x
    // at the state the call returns, not counted, and only where a sample is still to be taken.  A normal return gives every sample left to that step
    // (Tend may lie an ulp beyond T); after an error the ones left are not reached.  dn_open and dn_k are uniform over the workgroup; the closing Fun_x
    // stands where a step's first one would (the loop left at its head).
    if constexpr (DENSE) {
      if (dn_open && dn_k < a.dense_ns) {
        fun(y, fcn0);
        dense_take(fcn0, T, ierr == 1);
      }
      dense_leave(dn_k);
    }
    // ---- results
    {
      int tt = t;
      asm volatile("" : "+v"(tt));      // (the output offset is formed here: shared with the input load's it was a 64-bit value kept across the whole step loop — in scratch, in the 128-register kernels)
#pragma unroll
      for (int q = 0; q < SPT; q++) {
        const int s = q * NT + tt;
        if constexpr (SERIES) {
          if (s < NVAR) GM_(a.var_out)[(int64_t)leg * a.leg_var + (int64_t)cell * NVAR + s] = y[q];
        } else {
          if (s < NVAR) GM_(a.var_out)[(size_t)cell * NVAR + s] = y[q];
        }
      }
    }
    if constexpr (TRACE) {
      if (a.ctrl) {
#pragma unroll
        for (int q = 0; q < SPT; q++) {
          const int s = q * NT + t;
          if (s < NVAR) GM_(a.ctrl)[(size_t)cell * NVAR + s] = ctrl_r[q];
        }
      }
      if (t == 0) GM_(a.ntrace)[cell] = nstp;
    }
    if constexpr (SERIES) {      // the leg's results, into its block of every array
      if (t == 0) {
        GM_(a.ierr)[(int64_t)leg * a.leg_ierr + cell] = ierr;
        gptr_mut<int32_t> st = GM_(a.stats) + ((int64_t)leg * a.leg_stats + (int64_t)cell * 8);
        st[0] = nfun; st[1] = njac; st[2] = nstp; st[3] = nacc; st[4] = nrej; st[5] = ndec; st[6] = nsol; st[7] = nsng;
        if (a.texit_hexit) {
          GM_(a.texit_hexit)[(int64_t)leg * a.leg_th + (int64_t)cell * 2] = T;
          GM_(a.texit_hexit)[(int64_t)leg * a.leg_th + (int64_t)cell * 2 + 1] = *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT));
        }
        if (a.h_last) GM_(a.h_last)[(int64_t)leg * a.leg_h + cell] = Hget();
      }
    } else if (t == 0) {
      GM_(a.ierr)[cell] = ierr;
      gptr_mut<int32_t> st = GM_(a.stats) + (size_t)cell * 8;
      st[0] = nfun; st[1] = njac; st[2] = nstp; st[3] = nacc; st[4] = nrej; st[5] = ndec; st[6] = nsol; st[7] = nsng;
      if constexpr (profiling) {
        lap(6);
        pc[7] = clock64() - t_begin;
        for (int k = 0; k < kProfSlots; k++) GM_(a.prof)[(size_t)cell * kProfStride + k] = pc[k];
        for (int k = 0; k < 2; k++) GM_(a.prof)[(size_t)cell * kProfStride + kProfSlots + 4 * kProfWaves + k] = pw_calls[k];
      }
      if (a.texit_hexit) {
        GM_(a.texit_hexit)[(size_t)cell * 2] = T;
        GM_(a.texit_hexit)[(size_t)cell * 2 + 1] = *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT));
      }
      if constexpr (REPLAY) {      // the last step taken, not the one in progress when an error ended the call
        if (a.h_last) GM_(a.h_last)[cell] = *(volatile lds_f64*)(uintptr_t)(8u * (uint32_t)(L::RED + L::RED_HEXIT));
      } else {
        if (a.h_last) GM_(a.h_last)[cell] = Hget();
      }
    }
    if constexpr (profiling) {
      if (lane == 0 && wave < kProfWaves)
        for (int k = 0; k < 4; k++) GM_(a.prof)[(size_t)cell * kProfStride + kProfSlots + 4 * wave + k] = pw[k];
    }
    if constexpr (SERIES) {
      if (++leg >= a.nleg) break;
    }
  } while (SERIES);
}

#ifndef MISTRA_METHOD_TU      // (ros_unit_kernel.hip and ros_user_kernel.hip include this file for the kernel template alone)
// ---- launchers (one explicit instantiation per supported <mechanism, workgroup size>)
template <class MT, int NT>
hipError_t launch_ros3(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<MT, NT>::TOTAL * sizeof(double);
  bool& configured = *lds_configured;      // per device (capi.cpp: DeviceState): the attribute is a property of the device's code object
  auto kern = ros3_integrate_kernel<MT, NT, 0>;
  auto kern_prof = ros3_integrate_kernel<MT, NT, 1>;      // MISTRA_CHEM_PROFILE diagnostics (capi.cpp)
  auto kern_dump = ros3_integrate_kernel<MT, NT, 2>;      // first-step dump (mistra_chem_debug_first_step)
  auto kern_opt = ros3_integrate_kernel<MT, NT, 3>;       // Rosenbrock_x's options (mistra_chem_set_options); capi.cpp keeps a.dump and a.prof off while they are set
  if (!configured) {
    for (const void* k : {reinterpret_cast<const void*>(kern), reinterpret_cast<const void*>(kern_prof), reinterpret_cast<const void*>(kern_dump),
                          reinterpret_cast<const void*>(kern_opt)}) {
      hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) return e;
    }
    configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  if (a.dump) hipLaunchKernelGGL(kern_dump, dim3((unsigned)a.ncell), dim3(NT), lds_bytes, stream, a);
  else if (a.prof) hipLaunchKernelGGL(kern_prof, dim3((unsigned)a.ncell), dim3(NT), lds_bytes, stream, a);
  else if (a.opt) hipLaunchKernelGGL(kern_opt, dim3((unsigned)a.ncell), dim3(NT), lds_bytes, stream, a);
  else hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(NT), lds_bytes, stream, a);
  return hipGetLastError();
}

#ifdef MISTRA_DIAG_STAMPS
extern "C" int mistra_diag_dense_stamps(unsigned long long* out24, int reset) {
  if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_dense_stamps), 24 * sizeof(unsigned long long)) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[24] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_dense_stamps), z, sizeof z) != hipSuccess) return 1;
  }
  return 0;
}
#endif

template hipError_t launch_ros3<GasTraits, kGasNT>(const KernelArgs&, hipStream_t, bool*);
template hipError_t launch_ros3<AerTraits, kAerNT>(const KernelArgs&, hipStream_t, bool*);
template hipError_t launch_ros3<TotTraits, kTotNT>(const KernelArgs&, hipStream_t, bool*);
// (a 1024-thread tot variant was measured slower, and instantiating it caps the register budget of the shared
//  non-inlined device functions at that of a 16-wave workgroup)
#endif      // MISTRA_METHOD_TU

}  // namespace mistra
