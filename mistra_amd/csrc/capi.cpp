// C ABI of libmistra_chem.so (include/mistra_chem.h).  Host plumbing only: load tables, compile schedules, move
// buffers, launch the HIP kernel.  There is deliberately NO host compute path here — if the device is unusable the
// calls fail.
#include "../../include/mistra_chem.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "cell_split.hpp"
#include "kernel_args.hpp"
#include "mech_tables.hpp"
#include "pack.hpp"
#include "rates.hpp"
#include "ros3_kernel.hpp"
#include "ros_methods.hpp"
#include "schedule.hpp"
#include "user_mechs.hpp"

using namespace mistra;

namespace {

thread_local std::string g_err;
int fail(const std::string& msg) {
  g_err = msg;
  return 1;
}
#define HIP_TRY(expr)                                                                                    \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));               \
  } while (0)
#define LAUNCH_TRY(expr)                                                                                 \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e_));          \
  } while (0)

// the sizes of gas_Parameters.h | aer_Parameters.h | tot_Parameters.h, as the kernel is compiled for them (mistra_chem_dims needs no init)
struct MechDims {
  int nvar, nfix, nreact, lu_nonzero;
};
template <class MT>
bool traits_match(const MechTables& t, int n_jnz, int tail_regs, bool scale_pass, const DenseTail& dense) {
  return dense.nd == MT::DENSE_ND && dense.kb == MT::DENSE_KB && tail_regs == MT::TAIL_REGS && scale_pass == MT::SCALE_PASS && t.nvar == MT::NVAR && t.nfix == MT::NFIX && t.nreact == MT::NREACT && t.nnz == MT::NNZ && t.nb == MT::NB &&
         t.nconst == MT::NCONST && n_jnz == MT::NJNZ;
}

// ---- ONE ROW PER MECHANISM: everything the entries below need to know about a compiled kernel.  gas, aer, tot, then the user slots this library was
// built with (user_mechs.hpp: traits generated from the slots' tables at build time).  A user slot has the product, first-step-dump and options
// (Ros3) kernels and no method or trace kernels; its table is <mech dir>/<name>.mech and it never runs the dense tail block.
using LaunchFn = hipError_t (*)(const KernelArgs&, hipStream_t, bool*);
// The kernels of ros_unit_kernel.hip, [kernel VARIANT 3 .. 6][IPAR(4) resolved, ros_methods.hpp]: 3 the method kernels (Ros2, Ros4, Rodas3, Rodas4), 4 the
// step-control trace (Ros3), 5 the series and 6 the flux kernels (all five methods), 7 the dense-output kernels (all five methods; they live in the series
// units), 8 the operator kernels and 9 the replay kernels (Ros3's slot; they live in the trace units), 10 the series kernels with rate constants linear in
// time and 11 the series kernels with the reaction flux of every leg (all five methods; both live in the method units, Ros3's in the trace units).
// nullptr: not built.
constexpr int kVariants = 12, kMethods = 6;
struct UnitTable {
  LaunchFn fn[kVariants][kMethods] = {};
};
template <class MT, int NT, int VARIANT, int METHOD>
constexpr void add_unit(UnitTable& t) {
  if constexpr ((VARIANT != 3 || METHOD != kRos3) && ((VARIANT != 4 && VARIANT != 8 && VARIANT != 9) || METHOD == kRos3)) t.fn[VARIANT][METHOD] = &launch_ros_unit<MT, NT, VARIANT, METHOD>;
}
template <class MT, int NT, int... METHOD>
constexpr UnitTable unit_table(std::integer_sequence<int, METHOD...>) {
  UnitTable t;
  (..., (add_unit<MT, NT, 3, METHOD + 1>(t), add_unit<MT, NT, 4, METHOD + 1>(t), add_unit<MT, NT, 5, METHOD + 1>(t), add_unit<MT, NT, 6, METHOD + 1>(t),
        add_unit<MT, NT, 7, METHOD + 1>(t), add_unit<MT, NT, 8, METHOD + 1>(t), add_unit<MT, NT, 9, METHOD + 1>(t), add_unit<MT, NT, 10, METHOD + 1>(t),
        add_unit<MT, NT, 11, METHOD + 1>(t)));
  return t;
}
static_assert(kRos2 == 1 && kRodas4 == 5, "IPAR(4) resolved: 1 .. 5");
struct MechDesc {
  const char* name;
  MechDims dims;
  int nt;                          // workgroup size the kernels are instantiated with
  uint32_t ab_base, jb_base;       // LDS byte addresses of the A/B product array and of Jac_SP's B products (the gather-sum tables hold addresses)
  int max_temps;
  bool user;
  bool gsum_chain;                 // the kernels' trait GSUM_CHAIN: the long Vdot sums run as chain passes (schedule.hpp: GsumChain)
  bool (*match)(const MechTables&, int, int, bool, const DenseTail&);      // the loaded table against the compiled sizes
  LaunchFn ros3;                                                           // product | phase timing | first-step dump | options (Ros3)
  UnitTable unit;                                                          // every other options kernel (a user slot: none)
};
template <class MT, int NT>
constexpr MechDesc builtin_mech(const char* name) {
  return MechDesc{name, MechDims{MT::NVAR, MT::NFIX, MT::NREACT, MT::NNZ}, NT, 8u * (uint32_t)LdsLayout<MT, NT>::AB, 8u * (uint32_t)LdsLayout<MT, NT>::JB,
                  MT::MAX_TEMPS, false, MT::GSUM_CHAIN, &traits_match<MT>, &launch_ros3<MT, NT>, unit_table<MT, NT>(std::make_integer_sequence<int, 5>{})};
}
template <class MT, int NT>
constexpr MechDesc user_mech(const char* name) {
  return MechDesc{name, MechDims{MT::NVAR, MT::NFIX, MT::NREACT, MT::NNZ}, NT, 8u * (uint32_t)LdsLayout<MT, NT>::AB, 8u * (uint32_t)LdsLayout<MT, NT>::JB,
                  MT::MAX_TEMPS, true, MT::GSUM_CHAIN, &traits_match<MT>, &launch_ros3<MT, NT>, UnitTable{}};
}
constexpr int kBuiltinMechs = 3, kMaxMechs = 5;
constexpr int kNumMechs = kBuiltinMechs + MISTRA_USER_MECHS;
const MechDesc kMech[kNumMechs] = {
    builtin_mech<GasTraits, kGasNT>("gas"), builtin_mech<AerTraits, kAerNT>("aer"), builtin_mech<TotTraits, kTotNT>("tot"),
#if MISTRA_USER_MECHS >= 1
    user_mech<User0Traits, kUser0NT>(kUser0Name),
#endif
#if MISTRA_USER_MECHS >= 2
    user_mech<User1Traits, kUser1NT>(kUser1Name),
#endif
};
static_assert(MISTRA_MECH_USER0 == kBuiltinMechs && MISTRA_MECH_USER1 == kBuiltinMechs + 1 && kMaxMechs == kBuiltinMechs + 2, "mechanism ids of the user slots");
bool known_mech(int mech) { return mech >= 0 && mech < kNumMechs; }
// "Rosenbrock_g" | "Rosenbrock_a" | "Rosenbrock_t" | "Rosenbrock (<table>)"
std::string rosenbrock_name(int mech) { return kMech[mech].user ? std::string("Rosenbrock (") + kMech[mech].name + ")" : std::string("Rosenbrock_") + "gat"[mech]; }
// What a user slot does not have: every entry but dims, describe, the integrate family on rate constants, singular_rows, the first-step dump, the
// options and Rosenbrock_x with Ros3.  One text, before anything touches a device.
int fail_user_slot(int mech, const char* what) {
  g_err = std::string("user mechanism slot ") + std::to_string(mech - kBuiltinMechs) + " (" + kMech[mech].name + ") has no " + what +
          ": a user slot integrates (INTEGRATE_x on rate constants, Rosenbrock_x with Ros3 and its options, the first-step dump) and nothing else";
  return 1;
}
// Rosenbrock_x on a user slot: a valid method other than Ros3 (IPAR(4) = 0 selects Ros4) is refused before anything touches a device
int user_slot_method(int mech, const int32_t* ipar) {
  if (!known_mech(mech) || !kMech[mech].user || !ipar || ipar[3] == 2 || ipar[3] < 0 || ipar[3] > 5) return 0;
  return fail_user_slot(mech, "kernel for this Rosenbrock method (Ros2, Ros4, Rodas3, Rodas4)");
}
// -> 0 for gas, aer, tot; the refusal for a user slot and for an id that is no mechanism
int builtin_only(int mech, const char* what) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  return kMech[mech].user ? fail_user_slot(mech, what) : 0;
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t upload(const std::vector<T>& v) {
    release();
    n = v.size();
    if (!n) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t reserve(size_t count) {
    if (count <= n) return hipSuccess;
    release();
    n = count;
    return hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

}  // namespace

int mistra::rates_stack_depth(const RatesTable& T) {
  if (T.nreact < 0 || T.offs.size() != (size_t)T.nreact + 1) return -1;
  int deepest = 0;
  for (int r = 0; r < T.nreact; r++) {
    const int32_t w0 = T.offs[(size_t)r], w1 = T.offs[(size_t)r + 1];
    if (w0 < 0 || w1 < w0 || (size_t)w1 > T.words.size()) return -1;
    int sp = 0;
    for (int32_t w = w0; w < w1; w++) {
      const int op = T.words[(size_t)w] & 0xFF, arg = T.words[(size_t)w] >> 8;
      if (op <= 1) sp++;                                             // literal, input
      else if (op <= 5) { if (sp < 2) return -1; sp--; }             // + - * /
      else if (op == 6) { if (sp < 1) return -1; }                   // neg
      else if (op == 7 && arg >= 0 && arg < (int)(sizeof kRatesCallArgs / sizeof kRatesCallArgs[0])) {
        if (sp < kRatesCallArgs[arg]) return -1;
        sp += 1 - kRatesCallArgs[arg];
      } else return -1;
      if (sp > deepest) deepest = sp;
    }
    if (sp != 1) return -1;
  }
  return deepest;
}

namespace {
// the evaluator's operand stack is a fixed LDS column per thread: a deeper program would write past it
bool stack_fits(mistra::RatesTable& T, const std::string& path, std::string* err) {
  T.depth = mistra::rates_stack_depth(T);
  if (T.depth > mistra::kRatesStackDepth && err)
    *err = path + ": a program needs " + std::to_string(T.depth) + " operand-stack entries, the evaluator holds " + std::to_string(mistra::kRatesStackDepth);
  return T.depth <= mistra::kRatesStackDepth;
}
}  // namespace

bool mistra::RatesTable::load(const std::string& path, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  int32_t h[8];
  bool ok = std::fread(h, sizeof h, 1, f) == 1 && h[0] == 0x5441524B && h[1] == 2;
  depth = 0;
  if (ok) {
    nreact = h[2]; nenv = h[3];
    consts.resize((size_t)h[4]); offs.resize((size_t)nreact + 1); words.resize((size_t)h[5]); fslot.resize((size_t)h[6]);
    ok = h[6] == 50 && std::fread(consts.data(), 8, consts.size(), f) == consts.size() && std::fread(offs.data(), 4, offs.size(), f) == offs.size() &&
         std::fread(words.data(), 4, words.size(), f) == words.size() && std::fread(fslot.data(), 4, fslot.size(), f) == fslot.size();
  }
  std::fclose(f);
  if (!ok && err) *err = path + ": not a rate table";
  if (ok) {
    ok = stack_fits(*this, path, err);
    if (ok && depth < 0) { ok = false; if (err) *err = path + ": not a rate table (a program does not leave exactly one result)"; }
  }
  return ok;
}

bool mistra::StcoeffTable::load(const std::string& path, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  bool ok = true;
  for (int i = 0; ok && i < 4; i++) {
    RatesTable& T = v[i];
    int32_t h[8];
    ok = std::fread(h, sizeof h, 1, f) == 1 && h[0] == 0x5441524B && h[1] == 2 && h[2] > 0 && h[2] <= 4096 && h[3] >= 4 && h[3] <= 64 && h[4] >= 0 &&
         h[4] <= 1 << 20 && h[5] >= 0 && h[5] <= 1 << 20 && h[6] == 0 && h[7] == i;
    if (!ok) break;
    T.nreact = h[2]; T.nenv = h[3];
    T.consts.resize((size_t)h[4]); T.offs.resize((size_t)T.nreact + 1); T.words.resize((size_t)h[5]); T.fslot.clear();
    ok = (T.consts.empty() || std::fread(T.consts.data(), 8, T.consts.size(), f) == T.consts.size()) &&
         std::fread(T.offs.data(), 4, T.offs.size(), f) == T.offs.size() && (T.words.empty() || std::fread(T.words.data(), 4, T.words.size(), f) == T.words.size());
    // every index the evaluator follows is checked here: program bounds, literal and input slots, the functions st_coeff_x calls
    ok = ok && T.offs[0] == 0 && T.offs[(size_t)T.nreact] == (int32_t)T.words.size() && (i == 0 || (T.nreact == v[0].nreact && T.nenv == v[0].nenv));
    for (int r = 0; ok && r < T.nreact; r++) ok = T.offs[(size_t)r] < T.offs[(size_t)r + 1];
    for (size_t w = 0; ok && w < T.words.size(); w++) {
      const int op = T.words[w] & 0xFF, arg = T.words[w] >> 8;
      ok = op == 0 ? (arg >= 0 && arg < (int)T.consts.size()) : op == 1 ? (arg >= 0 && arg < T.nenv) : op <= 6 ? arg == 0 : (op == 7 && arg >= 26 && arg <= 28);
    }
  }
  std::fclose(f);
  if (!ok && err) *err = path + ": not a table of accommodation coefficients";
  for (int i = 0; ok && i < 4; i++) {
    ok = stack_fits(v[i], path, err);
    if (ok && v[i].depth < 0) { ok = false; if (err) *err = path + ": not a table of accommodation coefficients (a program does not leave exactly one result)"; }
    if (!ok) v[0].depth = v[i].depth;      // (setup_mech asks the first table why the file was refused)
  }
  return ok;
}

bool mistra::PackTable::load(const std::string& path, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  int32_t h[16];
  bool ok = std::fread(h, sizeof h, 1, f) == 1 && h[0] == 0x4B41504B && h[1] == 1;
  // header counts are bounded before anything is sized by them (a stale or corrupt file must not throw out of an extern "C" entry)
  for (int i = 2; ok && i < 16; i++) ok = h[i] >= 0 && h[i] <= (1 << 20);
  ok = ok && h[2] > 0 && h[3] >= 0 && h[4] > 0 && h[5] > 0 && h[6] >= 1 && h[6] <= 8 && h[7] <= 1 && h[11] <= kBudSlots;
  auto rd = [&](std::vector<int32_t>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), 4, n, f) == n; };
  if (ok) {
    nvar = h[2]; nfix = h[3]; j2 = h[4]; j6 = h[5]; nkc = h[6]; preclamp = h[7];
    ok = rd(pack, (size_t)h[8] * 4) && rd(fix, (size_t)h[9] * 3) && rd(unpack, (size_t)h[10] * 4) && rd(slot_id, (size_t)h[11]) &&
         rd(slot_first, (size_t)h[11] + 1) && rd(terms, (size_t)h[12] * 3) && rd(term_words, (size_t)h[13]) && rd(acc, (size_t)h[14] * 2) &&
         rd(envc, (size_t)h[15] * 2);
  }
  std::fclose(f);
  if (ok) {      // every index the kernels of pack.hip follow (reaction numbers and env slots: setup_mech, which knows NREACT and the env size)
    const int nspec = nvar + nfix, nl = j2 * nkc, ni = j6 * nkc, nterms = (int)terms.size() / 3, nwords = (int)term_words.size();
    for (int i = 0; ok && i < n_pack(); i++) {
      const int32_t* e = &pack[(size_t)4 * i];
      ok = e[0] >= 0 && e[0] < nspec && (e[1] == 0 || e[1] == 1) && e[2] >= 0 && e[2] < (e[1] == 0 ? nl : ni) && (e[3] == 0 || e[3] == 1);
    }
    for (int i = 0; ok && i < n_fix(); i++) {
      const int32_t* e = &fix[(size_t)3 * i];
      ok = e[0] >= 0 && e[0] < nspec && e[1] >= 0 && e[1] <= 3 && e[2] >= 0 && e[2] < 4;
    }
    for (int i = 0; ok && i < n_unpack(); i++) {
      const int32_t* e = &unpack[(size_t)4 * i];
      ok = (e[0] == 0 || e[0] == 1) && e[1] >= 0 && e[1] < (e[0] == 0 ? nl : ni) && e[2] >= 0 && e[2] < nvar && (e[3] == 0 || e[3] == 1);
    }
    for (int i = 0; ok && i < n_slots(); i++)
      ok = slot_id[(size_t)i] >= 1 && slot_id[(size_t)i] <= kBudSlots && slot_first[(size_t)i] >= 0 && slot_first[(size_t)i] <= slot_first[(size_t)i + 1] &&
           slot_first[(size_t)i + 1] <= nterms;
    for (int q = 0; ok && q < nterms; q++) {
      const int w0 = terms[(size_t)3 * q + 2], w1 = q + 1 < nterms ? terms[(size_t)3 * (q + 1) + 2] : nwords;
      ok = terms[(size_t)3 * q + 1] >= 0 && w0 >= 0 && w0 <= w1 && w1 <= nwords;
    }
    for (int32_t w : term_words) ok = ok && w >= 0 && w < nvar;      // (the budget kernel reads V[] only)
    for (size_t a = 0; ok && a < acc.size() / 2; a++) ok = acc[2 * a] >= 1 && acc[2 * a] <= acc[2 * a + 1] && acc[2 * a + 1] <= kBudSlots;
    for (int i = 0; ok && i < n_envc(); i++) ok = envc[(size_t)2 * i] >= 0 && envc[(size_t)2 * i + 1] >= 0 && envc[(size_t)2 * i + 1] < nspec;
  }
  if (!ok && err) *err = path + ": not a hand-over table";
  return ok;
}

bool mistra::KmtTable::load(const std::string& path, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  bool ok = std::fscanf(f, "%d %d %d %d", &nx, &nka, &nkt, &nkc) == 4 && nx > 0 && nx <= 64;
  if (ok) {
    lex.resize((size_t)nx);
    for (int i = 0; ok && i < nx; i++) ok = std::fscanf(f, "%d", &lex[(size_t)i]) == 1;
  }
  std::fclose(f);
  if (!ok && err) *err = path + ": not a species list of fast_k_mt";
  return ok;
}

bool mistra::LiqTable::load(const std::string& path, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  int32_t h[8];
  double d[3];
  bool ok = std::fread(h, sizeof h, 1, f) == 1 && h[0] == 0x5451494C && h[1] == 1 && h[2] > 0 && h[2] <= 4096 && h[3] >= 0 && h[3] <= h[2] &&
            h[4] >= 0 && h[4] <= h[2] && h[5] >= 1 && h[5] <= 8 && h[6] >= 0 && h[6] <= 1 << 20 && std::fread(d, sizeof d, 1, f) == 1;
  std::vector<int32_t> hj, hk, ej;
  std::vector<double> a0, b0;
  auto rdi = [&](std::vector<int32_t>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), 4, n, f) == n; };
  auto rdd = [&](std::vector<double>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), 8, n, f) == n; };
  if (ok) {
    nspec = h[2]; nh = h[3]; ne = h[4]; nkc_eq = h[5]; nfac = h[6];
    henry_tref = d[0]; henry_fct = d[1]; equil_tref = d[2];
    ok = rdi(hj, (size_t)nh) && rdi(hk, (size_t)nh) && rdd(a0, (size_t)nh) && rdd(b0, (size_t)nh) && rdi(ej, (size_t)ne) && rdi(foff, (size_t)ne + 1) &&
         rdi(boff, (size_t)ne + 1) && rdi(fkind, (size_t)nfac) && rdi(farg, (size_t)nfac) && rdd(fa, (size_t)nfac) && rdd(fb, (size_t)nfac);
  }
  std::fclose(f);
  if (ok) {      // dense per-species forms; every index the kernels follow is checked here
    h_kind.assign((size_t)nspec, -1); h_a0.assign((size_t)nspec, 0.0); h_b0.assign((size_t)nspec, 0.0); e_of.assign((size_t)nspec, -1);
    for (int i = 0; ok && i < nh; i++) {
      ok = hj[(size_t)i] >= 1 && hj[(size_t)i] <= nspec && (hk[(size_t)i] == 0 || hk[(size_t)i] == 1);
      if (ok) { const size_t j = (size_t)hj[(size_t)i] - 1; h_kind[j] = hk[(size_t)i]; h_a0[j] = a0[(size_t)i]; h_b0[j] = b0[(size_t)i]; }
    }
    for (int i = 0; ok && i < ne; i++) {
      ok = ej[(size_t)i] >= 1 && ej[(size_t)i] <= nspec && foff[(size_t)i] >= 0 && foff[(size_t)i] < boff[(size_t)i] && boff[(size_t)i] < foff[(size_t)i + 1] &&
           foff[(size_t)i + 1] <= nfac;
      if (ok) e_of[(size_t)ej[(size_t)i] - 1] = i;
    }
    for (int i = 0; ok && i < nfac; i++) ok = fkind[(size_t)i] >= 0 && fkind[(size_t)i] <= 3 && (fkind[(size_t)i] != 3 || (farg[(size_t)i] >= 1 && farg[(size_t)i] <= 4096));
  }
  if (!ok && err) *err = path + ": not a table of Henry / equilibrium constants";
  return ok;
}

bool mistra::VmeanTable::load(const std::string& path, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { if (err) *err = "cannot open " + path; return false; }
  int32_t h[8];
  bool ok = std::fread(h, sizeof h, 1, f) == 1 && h[0] == 0x544E4D56 && h[1] == 1 && h[2] > 0 && h[2] <= 4096 && h[3] >= 0 && h[3] <= h[2] &&
            std::fread(&coef, sizeof coef, 1, f) == 1 && coef > 0.0;
  std::vector<int32_t> j;
  std::vector<double> m;
  if (ok) {
    nspec = h[2];
    j.resize((size_t)h[3]); m.resize((size_t)h[3]);
    ok = (h[3] == 0 || std::fread(j.data(), 4, j.size(), f) == j.size()) && (h[3] == 0 || std::fread(m.data(), 8, m.size(), f) == m.size());
  }
  std::fclose(f);
  if (ok) {      // dense per-species form; every index is checked here
    mass.assign((size_t)nspec, 0.0);
    for (size_t i = 0; ok && i < j.size(); i++) {
      ok = j[i] >= 1 && j[i] <= nspec && m[i] > 0.0;
      if (ok) mass[(size_t)j[i] - 1] = m[i];
    }
  }
  if (!ok && err) *err = path + ": not a table of molar masses of v_mean";
  return ok;
}

namespace {

struct VmBufs {
  DevBuf<uint32_t> wave_base, recs;
  DevBuf<uint16_t> blk_n;
  int nrounds = 0;
  hipError_t upload(const VmProgram& P) {
    nrounds = P.nbarriers;      // what the executor counts down: the rounds that end in a barrier
    hipError_t e;
    if ((e = wave_base.upload(P.wave_base)) != hipSuccess) return e;
    if ((e = blk_n.upload(P.blk_n)) != hipSuccess) return e;
    return recs.upload(P.recs);
  }
  VmDev dev() const { return VmDev{wave_base.p, blk_n.p, recs.p, nrounds}; }
  void release() { wave_base.release(); recs.release(); blk_n.release(); }
};

struct GsBufs {
  DevBuf<uint32_t> wave_base, recs;
  DevBuf<uint16_t> rows;
  hipError_t upload(const GsumProgram& P) {
    hipError_t e;
    // whole ring turns per wave: gsum_run's loop counts in fours, and gsum_run_pair derives the next program's base from the count
    static_assert(GS_ROW_ALIGN == 4, "ring turn of gsum_exec_asm.inc");
    for (const auto r : P.rows)
      if (r % GS_ROW_ALIGN != 0) return hipErrorInvalidValue;
    if ((e = wave_base.upload(P.wave_base)) != hipSuccess) return e;
    if ((e = rows.upload(P.rows)) != hipSuccess) return e;
    return recs.upload(P.recs);
  }
  GsDev dev() const { return GsDev{wave_base.p, rows.p, recs.p}; }
  void release() { wave_base.release(); recs.release(); rows.release(); }
};

// ---- the per-mechanism device tables, one group per kernel-argument block: upload, release, `ready`, and the one place its block is built

struct KernelBufs {      // the integrator's (ros3_kernel.hip; make_args)
  int n_temps = 0, lu_scale_slots = 0;
  DevBuf<double> consts;
  DevBuf<uint64_t> fun_fac, jac_fac;
  DevBuf<uint16_t> jvs_pos, zero_pos, diag_pos, schur_cells;
  GsBufs vdot, jvs, vdot_pass;      // vdot: the program the kernel runs (KernelSchedule::vdot_chain.lean: the full one where the mechanism has no chain passes)
  DevBuf<uint64_t> vdot_chain_mask;
  VmBufs lu, solve_head_fwd, solve_head_bwd;
  DevBuf<uint32_t> tail_fwd, tail_bwd, tail_fwd_addr[2], tail_bwd_addr[2], lu_scale, dense_rows;
  int upload(const MechTables& t, const KernelSchedule& K) {
    n_temps = K.n_temps;
    lu_scale_slots = K.lu_scale.nslots;
    HIP_TRY(consts.upload(t.consts));
    HIP_TRY(fun_fac.upload(K.fun_fac));
    HIP_TRY(jac_fac.upload(K.jac_fac));
    HIP_TRY(jvs_pos.upload(K.jvs_pos));
    HIP_TRY(zero_pos.upload(K.zero_pos));
    HIP_TRY(diag_pos.upload(K.diag_pos));
    HIP_TRY(vdot.upload(K.vdot_chain.lean));
    HIP_TRY(vdot_pass.upload(K.vdot_chain.pass));
    HIP_TRY(vdot_chain_mask.upload(K.vdot_chain.mask));
    HIP_TRY(jvs.upload(K.jvs));
    HIP_TRY(lu.upload(K.lu));
    HIP_TRY(solve_head_fwd.upload(K.solve_head_fwd));
    HIP_TRY(solve_head_bwd.upload(K.solve_head_bwd));
    HIP_TRY(tail_fwd.upload(K.tail.fwd));
    HIP_TRY(tail_bwd.upload(K.tail.bwd));
    for (int r = 0; r < 2; r++) {
      HIP_TRY(tail_fwd_addr[r].upload(K.tail.fwd_addr[r]));
      HIP_TRY(tail_bwd_addr[r].upload(K.tail.bwd_addr[r]));
    }
    HIP_TRY(lu_scale.upload(K.lu_scale.recs));
    HIP_TRY(dense_rows.upload(K.dense.row_info));
    HIP_TRY(schur_cells.upload(K.dense.schur_cells));
    return 0;
  }
  void release() {
    consts.release(); fun_fac.release(); jac_fac.release(); jvs_pos.release(); zero_pos.release(); diag_pos.release(); schur_cells.release();
    vdot.release(); vdot_pass.release(); vdot_chain_mask.release(); jvs.release(); lu.release(); solve_head_fwd.release(); solve_head_bwd.release();
    tail_fwd.release(); tail_bwd.release(); lu_scale.release(); dense_rows.release();
    for (int r = 0; r < 2; r++) { tail_fwd_addr[r].release(); tail_bwd_addr[r].release(); }
  }
};

struct RatesBufs {       // Update_RCONST_x on the device (rates.hip): the mechanisms whose table and rate-law functions exist
  bool ready = false;
  int nreact = 0, nenv = 0;
  DevBuf<double> consts;
  DevBuf<int32_t> offs, words, fslot;
  int upload(const RatesTable& T) {
    HIP_TRY(consts.upload(T.consts));
    HIP_TRY(offs.upload(T.offs));
    HIP_TRY(words.upload(T.words));
    HIP_TRY(fslot.upload(T.fslot));
    nreact = T.nreact; nenv = T.nenv;
    ready = true;
    return 0;
  }
  RatesDev dev() const { return RatesDev{consts.p, offs.p, words.p, fslot.p, nreact, nenv}; }
  void release() { consts.release(); offs.release(); words.release(); fslot.release(); ready = false; }
};

struct PackBufs {        // the hand-over halves of x_drive (pack.hip): tables of the mechanism + the model's species maps
  bool ready = false, maps_ready = false;
  PackTable tab;
  DevBuf<int32_t> pack, fix, unpack, slot_id, slot_first, terms, words, acc, envc, a_ptr, a_fac;
  DevBuf<int32_t> gas_m2k, gas_k2m, rad_m2k, rad_k2m;
  int j1 = 0, j5 = 0;
  int upload(const MechTables& t) {      // (tab: loaded and checked by setup_mech)
    HIP_TRY(pack.upload(tab.pack)); HIP_TRY(fix.upload(tab.fix)); HIP_TRY(unpack.upload(tab.unpack));
    HIP_TRY(slot_id.upload(tab.slot_id)); HIP_TRY(slot_first.upload(tab.slot_first)); HIP_TRY(terms.upload(tab.terms));
    HIP_TRY(words.upload(tab.term_words)); HIP_TRY(acc.upload(tab.acc)); HIP_TRY(envc.upload(tab.envc));
    HIP_TRY(a_ptr.upload(t.a_ptr)); HIP_TRY(a_fac.upload(t.a_fac));
    ready = true;
    return 0;
  }
  int set_maps(int n1, const int32_t* g_m2k, const int32_t* g_k2m, int n5, const int32_t* r_m2k, const int32_t* r_k2m) {
    HIP_TRY(gas_m2k.upload(std::vector<int32_t>(g_m2k, g_m2k + 2 * (size_t)n1)));
    HIP_TRY(gas_k2m.upload(std::vector<int32_t>(g_k2m, g_k2m + (size_t)n1)));
    HIP_TRY(rad_m2k.upload(std::vector<int32_t>(r_m2k, r_m2k + 2 * (size_t)n5)));
    HIP_TRY(rad_k2m.upload(std::vector<int32_t>(r_k2m, r_k2m + (size_t)n5)));
    j1 = n1; j5 = n5;
    maps_ready = true;
    return 0;
  }
  PackDev dev(int nreact, const double* consts) const {
    const PackTable& T = tab;
    return PackDev{pack.p, fix.p, unpack.p, slot_id.p, slot_first.p, terms.p, words.p, acc.p, envc.p,
                   T.n_pack(), T.n_fix(), T.n_unpack(), T.n_slots(), (int)T.terms.size() / 3, (int)T.term_words.size(), (int)T.acc.size() / 2, T.n_envc(),
                   T.nvar, T.nfix, nreact, T.j2, T.j6, T.nkc, T.preclamp, gas_m2k.p, gas_k2m.p, rad_m2k.p, rad_k2m.p, j1, j5, a_ptr.p, a_fac.p, consts};
  }
  void release() {
    pack.release(); fix.release(); unpack.release(); slot_id.release(); slot_first.release(); terms.release(); words.release(); acc.release();
    envc.release(); a_ptr.release(); a_fac.release(); gas_m2k.release(); gas_k2m.release(); rad_m2k.release(); rad_k2m.release();
    ready = maps_ready = false;
  }
};

struct KmtBufs {         // fast_k_mt_a / fast_k_mt_t (aer, tot): the exchanged species
  bool ready = false;
  KmtTable tab;
  DevBuf<int32_t> lex;
  int upload() {
    HIP_TRY(lex.upload(tab.lex));
    ready = true;
    return 0;
  }
  KmtDev dev(int nspec, int ka, int ifeed, int nkc_l) const { return KmtDev{lex.p, {0}, tab.nx, tab.nka, tab.nkt, tab.nkc, nspec, ka, ifeed, nkc_l}; }
  void release() { lex.release(); ready = false; }
};

struct LiqBufs {         // henry_x / equil_co_x (aer, tot)
  bool ready = false;
  LiqTable tab;
  DevBuf<int32_t> h_kind, e_of, foff, boff, fkind, farg;
  DevBuf<double> h_a0, h_b0, fa, fb;
  int upload() {
    HIP_TRY(h_kind.upload(tab.h_kind)); HIP_TRY(e_of.upload(tab.e_of)); HIP_TRY(foff.upload(tab.foff)); HIP_TRY(boff.upload(tab.boff));
    HIP_TRY(fkind.upload(tab.fkind)); HIP_TRY(farg.upload(tab.farg)); HIP_TRY(h_a0.upload(tab.h_a0)); HIP_TRY(h_b0.upload(tab.h_b0));
    HIP_TRY(fa.upload(tab.fa)); HIP_TRY(fb.upload(tab.fb));
    ready = true;
    return 0;
  }
  LiqDev dev() const {
    return LiqDev{h_kind.p, e_of.p, foff.p, boff.p, fkind.p, farg.p, h_a0.p, h_b0.p, fa.p, fb.p, tab.nspec, tab.nkc_eq, tab.henry_tref, tab.henry_fct, tab.equil_tref};
  }
  void release() {
    h_kind.release(); e_of.release(); foff.release(); boff.release(); fkind.release(); farg.release(); h_a0.release(); h_b0.release();
    fa.release(); fb.release(); ready = false;
  }
};

struct StcBufs {         // st_coeff_x (aer, tot): one table per setting of the two namelist switches
  bool ready = false;
  StcoeffTable tab;
  DevBuf<double> consts[4];
  DevBuf<int32_t> offs[4], words[4];
  int upload() {
    for (int i = 0; i < 4; i++) {
      HIP_TRY(consts[i].upload(tab.v[i].consts)); HIP_TRY(offs[i].upload(tab.v[i].offs)); HIP_TRY(words[i].upload(tab.v[i].words));
    }
    ready = true;
    return 0;
  }
  RatesDev dev(int v) const { return RatesDev{consts[v].p, offs[v].p, words[v].p, nullptr, tab.v[v].nreact, tab.v[v].nenv}; }
  void release() {
    for (int i = 0; i < 4; i++) { consts[i].release(); offs[i].release(); words[i].release(); }
    ready = false;
  }
};

struct VmeanBufs {       // v_mean_x (aer, tot)
  bool ready = false;
  VmeanTable tab;
  DevBuf<double> mass;
  int upload() {
    HIP_TRY(mass.upload(tab.mass));
    ready = true;
    return 0;
  }
  void release() { mass.release(); ready = false; }
};

// the groups an entry needs (require)
enum : unsigned { kNeedRates = 1, kNeedPackTable = 2, kNeedMaps = 4, kNeedPack = kNeedPackTable | kNeedMaps, kNeedKmt = 8, kNeedLiq = 16, kNeedStc = 32, kNeedVmean = 64 };

// ---- staging of the host-buffer entries

// A grow-only device block, a pinned host mirror of the same layout and a private non-blocking stream.  Freed by release() only: the
// instances are globals, and a destructor would run after the HIP runtime may be gone.
struct Staging {
  char *dev = nullptr, *host = nullptr;
  size_t cap = 0;      // bytes
  hipStream_t st = nullptr;
  hipError_t ensure(size_t bytes) {
    if (!st)
      if (hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) return e;
    if (bytes <= cap) return hipSuccess;
    free_blocks();
    const size_t want = bytes + bytes / 2;
    if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), want)) return e;
    if (hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), want, hipHostMallocDefault)) return e;
    cap = want;
    return hipSuccess;
  }
  template <class T = double>
  T* d(size_t off) const { return reinterpret_cast<T*>(dev + off); }
  template <class T = double>
  T* h(size_t off) const { return reinterpret_cast<T*>(host + off); }
  void free_blocks() {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr; cap = 0;
  }
  void release() {
    free_blocks();
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
  }
};

// 256-byte aligned parts of a staging block: take() gives back a part's byte offset, the same in the device block and in the mirror
struct Layout {
  size_t end = 0;
  size_t take(size_t bytes) {
    const size_t at = end;
    end += (bytes + 255) & ~(size_t)255;
    return at;
  }
};

// one column step in the drive arena of its mechanism.  In/out first — s1 | s3 | sl1 | sion1 | bg | bgs — then in-only — scal | env — then
// out-only — th(2) | hlast | ierr | stats | c_packed — then device only — var | fix | rct.  Counts in doubles per layer, offsets in bytes.
// With step reuse on (mistra_chem_set_step_reuse) the layer list rides behind env in the in-only part and the gathered first steps behind rct.
struct DriveLayout {
  size_t nl = 0, j1 = 0, j5 = 0, nsl = 0, nsi = 0, nv = 0, nf = 0, nr = 0, ne = 0;
  size_t s1 = 0, s3 = 0, sl1 = 0, si = 0, bg = 0, bgs = 0, io_end = 0, scal = 0, env = 0, lyr = 0, in_end = 0;
  size_t th = 0, hl = 0, ierr = 0, stats = 0, cp = 0, out_end = 0, var = 0, fix = 0, rct = 0, hs = 0, end = 0;
};

// The options blocks of mistra_chem_rosenbrock_device: each call's own (kernel_args.hpp: RosOptSlot), copied to the device on the call's stream in front
// of its kernel.  kRosCallsInFlight blocks per mechanism and device slot, used in turn, each with a pinned host mirror and an event recorded behind the
// kernel that reads it: the call that comes round to a block whose kernel has not finished waits for that event.
constexpr int kRosCallsInFlight = MISTRA_ROSENBROCK_CALLS_IN_FLIGHT;
struct RosCallRing {
  double *dev = nullptr, *host = nullptr;      // kRosCallsInFlight blocks of `words` doubles each
  size_t words = 0;
  hipEvent_t ev[kRosCallsInFlight] = {};
  bool pending[kRosCallsInFlight] = {};
  int next = 0;
  hipError_t ensure(size_t w) {
    if (dev) return hipSuccess;
    words = (w + 31) & ~(size_t)31;
    if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), kRosCallsInFlight * words * sizeof(double))) return e;
    if (hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), kRosCallsInFlight * words * sizeof(double), hipHostMallocDefault)) return e;
    for (auto& e : ev)
      if (hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming)) return rc;
    return hipSuccess;
  }
  void release() {
    for (int i = 0; i < kRosCallsInFlight; i++) {
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      ev[i] = nullptr;
      pending[i] = false;
    }
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr; words = 0; next = 0;
  }
  // the next block in turn, `w` words at least (the ring is sized by its first call), once the kernel that read it kRosCallsInFlight calls ago has
  // finished -> its index, host mirror and device block
  hipError_t acquire(size_t w, int* i, double** hb, double** db) {
    if (hipError_t e = ensure(w)) return e;
    *i = next;
    next = (next + 1) % kRosCallsInFlight;
    if (pending[*i])
      if (hipError_t e = hipEventSynchronize(ev[*i])) return e;
    pending[*i] = false;
    *hb = host + (size_t)*i * words; *db = dev + (size_t)*i * words;
    return hipSuccess;
  }
  // behind the kernel that reads block i, also behind a failed launch: the copy is queued
  void mark(int i, hipStream_t st) {
    if (hipEventRecord(ev[i], st) == hipSuccess) pending[i] = true;
  }
};

struct MechState {
  bool ready = false;
  int nt = 0;
  MechTables tab;
  std::string text;
  KernelBufs k;
  RatesBufs rates;
  PackBufs pack;
  KmtBufs kmt;
  LiqBufs liq;
  StcBufs stc;
  VmeanBufs vmean;
  DevBuf<double> d_rct;      // scratch of mistra_chem_drive_device (grow-only)
  // Rosenbrock_x's options on this slot (mistra_chem_set_options): the block the options kernel reads (kernel_args.hpp: RosOptSlot), null while
  // none are set, and IPAR(3) (0: the library's Max_no_steps)
  DevBuf<double> opt;
  int opt_max_steps = 0;
  // the integrator policy on this slot (mistra_chem_set_policy): method 0 = none; pol_opt: INTEGRATE_x's values as an options block, read while a policy
  // is set and no options are
  int pol_method = 0;
  double pol_factor = 0.0, pol_floor = 0.0;
  DevBuf<double> pol_opt;
  // the per-call options of mistra_chem_rosenbrock_ex (host buffers: one block, the call is synchronous) and mistra_chem_rosenbrock_device
  DevBuf<double> call_opt;
  RosCallRing call_ring;
  // ... and of the series entries: a block is the call's options, then its times (kernel_args.hpp: times).  A ring of its own: every block has room
  // for MISTRA_SERIES_MAX_LEGS + 1 times, which the single calls' blocks need not carry
  RosCallRing series_ring;
  // staging of the series' _ex entries: the legs' states of this slot's cells (grow-only).  Their other outputs — ierr, stats, th, the flux — take nleg
  // blocks of the single calls' buffers below: a host call is synchronous under g_mu and the buffers only grow, so no call finds them smaller than it left them
  DevBuf<double> s_ser_var;
  // the step memory of the batched driver (mistra_chem_set_step_reuse): per model layer k = 1..step_n the last accepted step size of the layer's previous
  // column step of this mechanism, 0 = none.  step_n = 0: forgotten — the next column step under reuse sizes it to its n and zeroes it on the drive stream
  DevBuf<double> step_mem;
  int step_n = 0;
  // staging of the batched host-buffer entries (grow-only)
  DevBuf<double> s_var, s_fix, s_rct, s_th, s_env, s_hst;
  DevBuf<double> s_tol;                    // ... and of mistra_chem_rosenbrock_cells_ex: the block's AbsTol rows, then its RelTol rows
  DevBuf<int32_t> s_ierr, s_stats, s_sing;
  DevBuf<double> s_trd;                    // ... and of mistra_chem_rosenbrock_trace_ex: the records, the attempt counts, the per-species counts
  DevBuf<int32_t> s_tri, s_ntr, s_ctl;      // (s_ntr also: the cells' own step counts of a replay call, which has no trace)
  DevBuf<double> s_flux;                   // ... and of mistra_chem_rosenbrock_flux_ex: the block's flux rows
  DevBuf<double> s_dn_y;                   // ... and of mistra_chem_rosenbrock_dense_ex: the samples' blocks of this slot's cells, the numbers reached
  DevBuf<int32_t> s_dn_n;
  DevBuf<double> s_ops;                    // ... and of mistra_chem_ops_ex: vdot | jvs | shift | rhs | x of this slot's cells
  DevBuf<double> s_rp;                     // ... and of mistra_chem_rosenbrock_replay_ex: this slot's cells' rows of steps | their Err rows
  // where the zero-pivot rows of the LAST host-buffer call of this slot are (mistra_chem_singular_rows): cells [sing_start,
  // sing_start + sing_count) of the caller's batch in s_sing, or the one cell of the COMMON-block call in one_sing
  size_t sing_start = 0, sing_count = 0;
  bool sing_one = false;
  int32_t one_sing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  Staging drive;      // mistra_chem_drive(_begin): everything that crosses PCIe for a batch of layers, one copy up and the chain on its stream
  Staging one;        // one-cell calls (the Fortran shim): one copy in, one out
  struct PendingDrive {      // a column step issued by mistra_chem_drive_begin and not yet fetched by mistra_chem_drive_end
    bool active = false;
    DriveLayout lay;
    std::vector<int32_t> layer, level;
    double *s1 = nullptr, *s3 = nullptr, *sl1 = nullptr, *sion1 = nullptr, *bg = nullptr, *bgs = nullptr, *t_h = nullptr, *c_packed = nullptr;
    int32_t *ierr = nullptr, *stats = nullptr;
    int nrxn = 0;
  } pend;
  void release() {
    k.release(); rates.release(); pack.release(); kmt.release(); liq.release(); stc.release(); vmean.release();
    d_rct.release();
    opt.release(); opt_max_steps = 0;
    pol_opt.release(); pol_method = 0; pol_factor = pol_floor = 0.0;
    call_opt.release(); call_ring.release(); series_ring.release();
    s_ser_var.release();
    step_mem.release(); step_n = 0;
    s_hst.release(); s_tol.release();
    s_var.release(); s_fix.release(); s_rct.release(); s_th.release(); s_env.release(); s_ierr.release(); s_stats.release(); s_sing.release();
    s_trd.release(); s_tri.release(); s_ntr.release(); s_ctl.release(); s_flux.release(); s_dn_y.release(); s_dn_n.release(); s_ops.release(); s_rp.release();
    sing_count = 0; sing_one = false;
    drive.release(); one.release();
    pend = PendingDrive{};      // (a step issued and never fetched dies with its buffers)
    ready = false;
  }
};

// One DeviceState per GPU the library was initialised on (mistra_chem_init: one; mistra_chem_init_devices: several).
// Slot 0 is the primary device: the host-buffer entry points and mistra_chem_describe use it.
struct DeviceState {
  int id = -1;
  MechState mech[kMaxMechs];                          // (the rows of kMech: the slots past kNumMechs are never set up)
  // hipFuncAttributeMaxDynamicSharedMemorySize is per device and kernel: [mechanism][kernel VARIANT][IPAR(4)] as MechDesc::unit, [mechanism][0][0] the
  // kernels of launch_ros3
  bool lds_configured[kMaxMechs][kVariants][kMethods] = {};
  void release() {
    if (id >= 0) (void)hipSetDevice(id);
    for (auto& m : mech) m.release();
    std::memset(lds_configured, 0, sizeof lds_configured);
    id = -1;
  }
};

std::mutex g_mu;
bool g_inited = false;
int g_max_steps = 100000;      // Max_no_steps (gas.f:1042); only mistra_chem_debug_set_max_steps changes it
std::vector<DeviceState> g_devs;

// ---- Rosenbrock_x's options (gas.f:777-1108 | aer.f | tot.f), which INTEGRATE_x fixes and mistra_chem_set_options opens: per mechanism,
// process-wide.  They outlive a re-initialisation on other devices (setup_mech uploads them again); mistra_chem_finalize drops them.
struct RosResolved {      // what Rosenbrock_x's decode (gas.f:936-1053) hands to RosenbrockIntegrator_x
  double hmin = 0.0, hmax = 0.0, hstart = 0.0, facmin = 0.0, facmax = 0.0, facrej = 0.0, facsafe = 0.0;      // hmax: RPAR(2), +inf where it is 0
  int max_steps = 0, autonomous = 0, vector = 0;
};
struct RosOptions {
  bool set = false;
  int32_t ipar[20] = {0};
  double rpar[20] = {0.0};
  RosResolved r;
  std::vector<double> block;      // the device block: RosOptSlot scalars, then AbsTol(1:NVAR), RelTol(1:NVAR) as the integrator uses them
} g_opts[kMaxMechs];

// ---- OPT-IN integrator policy (mistra_chem_set_policy): per mechanism, process-wide.  What the entries that carry no options of their own — the
// integrate family and the column driver — run instead of Ros3 with the options' AbsTol: a method of Rosenbrock_x's five and / or a cell-relative
// AbsTol (kernel_args.hpp: tol_cell_factor).  Everything else stays the options in force; with none set, INTEGRATE_x's values go into a block of the
// library's own (MechState::pol_opt), which gives the product kernel's bits (DESIGN.md §8 a2').  Like the options it outlives a re-initialisation;
// mistra_chem_finalize puts back what the environment asked for (read_policy_env).
struct Policy {
  bool set = false;
  int method = kRos3;
  double factor = 0.0, floor = 0.0;
} g_policy[kMaxMechs], g_policy_env[kMaxMechs];

// the checks of a policy, no device: 0, or the refusal
int check_policy(int mech, int method, double factor, double floor) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (method == 0)
    return fail("policy: method 0 is refused: in " + rosenbrock_name(mech) + " IPAR(4) = 0 selects Ros4; name the method, 1 .. 5 (Ros2, Ros3, Ros4, Rodas3, Rodas4; 2 keeps Ros3)");
  if (method < 1 || method > 5) return fail("policy: method " + std::to_string(method) + " is none of " + rosenbrock_name(mech) + "'s: 1 .. 5 (Ros2, Ros3, Ros4, Rodas3, Rodas4)");
  if (kMech[mech].user && method != kRos3) return fail_user_slot(mech, "kernel for this Rosenbrock method (Ros2, Ros4, Rodas3, Rodas4)");
  if (factor != 0.0) {      // mistra_chem_cell_atol_device's rule and texts
    if (!(factor > 0.0) || !std::isfinite(factor)) return fail("cell_atol: factor must be finite and positive");
    if (!(floor > 0.0) || !std::isfinite(floor)) return fail("cell_atol: floor must be finite and positive");
  }
  return 0;
}

// INTEGRATE_x's values as an options block (gas.f:745-756): RTOL 1e-3, ATOL 1e-25, RPAR(3) = 1e-3, everything else Rosenbrock_x's default
std::vector<double> options_block(int mech, const RosResolved& r, const double* atol, const double* rtol);
int resolve_options(int mech, const int32_t* ipar, const double* rpar, const double* atol, const double* rtol, RosResolved* r);
std::vector<double> base_options_block(int mech) {
  int32_t ipar[20] = {0};
  double rpar[20] = {0.0};
  ipar[1] = 1; ipar[3] = 2;
  rpar[2] = 1.0e-3;
  const double atol = 1.0e-25, rtol = 1.0e-3;
  RosResolved r;
  (void)resolve_options(mech, ipar, rpar, &atol, &rtol, &r);
  return options_block(mech, r, &atol, &rtol);
}

// The environment of a model binary that is already linked, read once (g_mu held) beside read_step_env: MISTRA_CHEM_METHOD and MISTRA_CHEM_ATOL_REL for
// gas, aer and tot, MISTRA_CHEM_METHOD_G / _A / _T and MISTRA_CHEM_ATOL_REL_G / _A / _T for one of them (they go before the former).  A method is a name
// (ros2, ros3, ros4, rodas3, rodas4, any letter case) or 1 .. 5; ATOL_REL is `factor` or `factor,floor` (floor: INTEGRATE_x's ATOL, 1e-25).  A value that
// cannot be read that way is an error every initialisation and every policy entry reports with the variable's name: never a quiet run with something else.
bool g_policy_env_read = false;
std::string g_policy_env_err;
bool parse_method(const char* s, int* method) {
  static const char* names[5] = {"ros2", "ros3", "ros4", "rodas3", "rodas4"};
  std::string v;
  for (const char* p = s; *p; p++) v += (char)std::tolower((unsigned char)*p);
  for (int i = 0; i < 5; i++)
    if (v == names[i]) { *method = i + 1; return true; }
  if (v.size() == 1 && v[0] >= '1' && v[0] <= '5') { *method = v[0] - '0'; return true; }
  return false;
}
bool parse_double(const std::string& s, double* v) {
  if (s.empty() || std::isspace((unsigned char)s[0])) return false;
  char* end = nullptr;
  *v = std::strtod(s.c_str(), &end);
  return end && *end == '\0';
}
bool parse_atol_rel(const char* s, double* factor, double* floor) {
  const std::string v = s;
  const size_t k = v.find(',');
  *floor = 1.0e-25;
  if (!parse_double(v.substr(0, k), factor)) return false;
  if (k != std::string::npos && !parse_double(v.substr(k + 1), floor)) return false;
  return *factor > 0.0 && std::isfinite(*factor) && *floor > 0.0 && std::isfinite(*floor);
}
int read_policy_env() {
  if (!g_policy_env_read) {
    g_policy_env_read = true;
    for (int mech = 0; mech < kBuiltinMechs; mech++) {
      Policy p;
      const std::string sfx = std::string("_") + "GAT"[mech];
      for (const std::string& name : {std::string("MISTRA_CHEM_METHOD"), "MISTRA_CHEM_METHOD" + sfx}) {
        const char* e = std::getenv(name.c_str());
        if (!e) continue;
        if (!parse_method(e, &p.method)) {
          g_policy_env_err = name + "=" + e + ": a method is a name (ros2, ros3, ros4, rodas3, rodas4) or a number 1 .. 5";
          break;
        }
        p.set = true;
      }
      for (const std::string& name : {std::string("MISTRA_CHEM_ATOL_REL"), "MISTRA_CHEM_ATOL_REL" + sfx}) {
        const char* e = std::getenv(name.c_str());
        if (!e) continue;
        if (!parse_atol_rel(e, &p.factor, &p.floor)) {
          g_policy_env_err = name + "=" + e + ": a cell-relative AbsTol is `factor` or `factor,floor`, both finite and positive";
          break;
        }
        p.set = true;
      }
      if (!g_policy_env_err.empty()) break;
      g_policy_env[mech] = p;
    }
    if (g_policy_env_err.empty())
      for (int mech = 0; mech < kBuiltinMechs; mech++) g_policy[mech] = g_policy_env[mech];
  }
  return g_policy_env_err.empty() ? 0 : fail(g_policy_env_err);
}

// ---- OPT-IN step reuse of the batched driver (mistra_chem_set_step_reuse): per mechanism, process-wide host state; MISTRA_CHEM_HSTART_REUSE=1 in the
// environment turns all three on, read once — by the first initialisation or the first look at the flags, whichever comes first (g_mu held)
bool g_step_reuse[kBuiltinMechs] = {false, false, false};      // (a user slot has no batched driver)
bool g_step_env_read = false;
void read_step_env() {
  if (g_step_env_read) return;
  g_step_env_read = true;
  const char* e = std::getenv("MISTRA_CHEM_HSTART_REUSE");
  if (e && std::atoi(e) != 0)
    for (bool& r : g_step_reuse) r = true;
}

// the host-buffer entries of the liq_parm kernels: one arena on the primary device (DevBlock below), and the caller ranges that
// mistra_chem_pin_host registered, which those entries copy to and from directly
Staging g_liq;
struct PinnedRanges {
  std::vector<std::pair<const char*, size_t>> r;
  bool contains(const void* p, size_t n) const {
    const char* c = static_cast<const char*>(p);
    for (const auto& x : r)
      if (c >= x.first && c + n <= x.first + x.second) return true;
    return false;
  }
  void release() {
    for (const auto& x : r) (void)hipHostUnregister(const_cast<char*>(x.first));
    r.clear();
  }
} g_pinned;

void release_all() {
  if (!g_devs.empty() && g_devs[0].id >= 0) (void)hipSetDevice(g_devs[0].id);
  g_pinned.release();
  g_liq.release();
  for (auto& d : g_devs) d.release();
  g_devs.clear();
  g_inited = false;
}

std::string mech_dir() {
  if (const char* e = std::getenv("MISTRA_MECH_DIR")) return e;
  Dl_info info;
  if (dladdr(reinterpret_cast<const void*>(&mistra_chem_init), &info) && info.dli_fname) {
    std::string p = info.dli_fname;
    size_t k = p.rfind('/');
    std::string dir = k == std::string::npos ? "." : p.substr(0, k);
    return dir + "/../mech";
  }
  return "mech";
}

int setup_mech(DeviceState& D, int mech) {
  MechState& S = D.mech[mech];
  const MechDesc& M = kMech[mech];
  const std::string name = M.name, base = mech_dir() + "/" + name;
  std::string err;
  if (M.user) {      // a mechanism directory without the slot's table (a caller's own MISTRA_MECH_DIR with gas, aer and tot alone): the library comes up
                     // as it did before it had slots, and the slot's entries say that its table was not there (check_call).  A table that is there and
                     // cannot be read or has other sizes fails the init like any other.
    FILE* f = std::fopen((base + ".mech").c_str(), "rb");
    if (!f) return 0;
    std::fclose(f);
  }
  if (!S.tab.load(base + ".mech", &err)) return fail(err);
  S.nt = M.nt;
  KernelSchedule K;
  try {
    // (a user slot never runs the dense tail block, whatever its NVAR: its kernels are compiled without it)
    const DenseConfig dc = M.user ? DenseConfig{0, 0} : dense_config(S.tab);
    K = build_kernel_schedule(S.tab, S.nt, M.ab_base, M.max_temps, dc.nd, dc.kb, M.jb_base, M.gsum_chain);
  } catch (const std::exception& ex) {
    return fail(std::string("schedule compiler: ") + ex.what());
  }
  if (!M.match(S.tab, K.n_jnz, K.tail.regs, K.lu_scale.nslots > 0, K.dense)) return fail(name + ": mechanism table does not match the compiled kernel sizes");
  S.text = name + ": " + describe(K);
  if (int rc = S.k.upload(S.tab, K)) return rc;
  // the optional tables: a mechanism without the file has no such routine (the entries that need one say so)
  const int nspec = S.tab.nvar + S.tab.nfix;
  RatesTable R;
  if (R.load(base + ".rates", &err)) {      // (gas today)
    if (R.nreact != S.tab.nreact) return fail(name + ".rates does not belong to this mechanism");
    if (int rc = S.rates.upload(R)) return rc;
  } else if (R.depth > kRatesStackDepth) {
    return fail(err);      // (a missing table is a mechanism without the routine; a table the evaluator cannot run is an error)
  }
  if (S.pack.tab.load(base + ".pack", &err)) {      // the drivers' hand-over tables
    const PackTable& T = S.pack.tab;
    if (T.nvar != S.tab.nvar || T.nfix != S.tab.nfix) return fail(name + ".pack does not belong to this mechanism");
    for (size_t q = 0; q < T.terms.size() / 3; q++)
      if (T.terms[3 * q + 1] >= S.tab.nreact) return fail(name + ".pack: a budget term names a reaction the mechanism does not have");
    for (int i = 0; i < T.n_envc(); i++)
      if (S.rates.ready && T.envc[(size_t)2 * i] >= S.rates.nenv) return fail(name + ".pack: a concentration slot lies outside the rate evaluator's input");
    if (int rc = S.pack.upload(S.tab)) return rc;
  }
  if (S.kmt.tab.load(base + ".kmt", &err)) {      // species list of the mass-transfer routines (aer, tot)
    for (int32_t i : S.kmt.tab.lex)
      if (i < 1 || i > nspec) return fail(name + ".kmt does not belong to this mechanism");
    if (int rc = S.kmt.upload()) return rc;
  }
  if (S.liq.tab.load(base + ".liq", &err)) {      // Henry and equilibrium constants (aer, tot)
    if (S.liq.tab.nspec != nspec) return fail(name + ".liq does not belong to this mechanism");
    if (int rc = S.liq.upload()) return rc;
  }
  if (S.stc.tab.load(base + ".stcoeff", &err)) {      // accommodation coefficients (aer, tot)
    if (S.stc.tab.v[0].nreact != nspec) return fail(name + ".stcoeff does not belong to this mechanism");
    if (int rc = S.stc.upload()) return rc;
  } else if (S.stc.tab.v[0].depth > kRatesStackDepth) {
    return fail(err);
  }
  if (S.vmean.tab.load(base + ".vmean", &err)) {      // mean molecular speeds (aer, tot)
    if (S.vmean.tab.nspec != nspec) return fail(name + ".vmean does not belong to this mechanism");
    if (int rc = S.vmean.upload()) return rc;
  }
  if (g_opts[mech].set) {      // options set before this (re-)initialisation stay in force
    HIP_TRY(S.opt.upload(g_opts[mech].block));
    S.opt_max_steps = g_opts[mech].ipar[2];
  }
  if (g_policy[mech].set) {      // ... and so does a policy
    HIP_TRY(S.pol_opt.upload(base_options_block(mech)));
    S.pol_method = g_policy[mech].method; S.pol_factor = g_policy[mech].factor; S.pol_floor = g_policy[mech].floor;
  }
  S.ready = true;
  return 0;
}

// text of ros_ErrorMsg_x (gas.f:1474-1509) for an error code
const char* ros_error_text(int code) {
  switch (code) {
    case -1: return "--> Improper value for maximal no of steps";
    case -2: return "--> Selected Rosenbrock method not implemented";
    case -3: return "--> Hmin/Hmax/Hstart must be positive";
    case -4: return "--> FacMin/FacMax/FacRej must be positive";
    case -5: return "--> Improper tolerance values";
    case -6: return "--> No of steps exceeds maximum bound";
    case -7: return "--> Step size too small: T + 10*H = T or H < Roundoff";
    case -8: return "--> Matrix is repeatedly singular";
  }
  return nullptr;
}

// Rosenbrock_x's decode of IPAR, RPAR and the tolerances, test by test in its order (gas.f:936-1053) -> 1, or the IERR it returns through
// ros_ErrorMsg_x; *r is complete only for 1.  Pure host arithmetic.  atol / rtol: entry 1 alone is read unless IPAR(2) = 0.
int resolve_options(int mech, const int32_t* ipar, const double* rpar, const double* atol, const double* rtol, RosResolved* r) {
  r->autonomous = ipar[0] != 0;                                   // gas.f:937
  r->vector = ipar[1] == 0;                                       // gas.f:941
  if (ipar[2] == 0) r->max_steps = 100000;                        // gas.f:950
  else if (ipar[2] > 0) r->max_steps = ipar[2];
  else return -1;
  if (ipar[3] < 0 || ipar[3] > 5) return -2;                      // gas.f:961 (0 selects Ros4)
  if (rpar[0] == 0.0) r->hmin = 0.0;                              // gas.f:976
  else if (rpar[0] > 0.0) r->hmin = rpar[0];
  else return -3;
  if (rpar[1] == 0.0) r->hmax = HUGE_VAL;                         // gas.f:986: ABS(Tend-Tstart), the call's
  else if (rpar[1] > 0.0) r->hmax = rpar[1];
  else return -3;
  if (rpar[2] == 0.0) r->hstart = r->hmin > 1.0e-5 ? r->hmin : 1.0e-5;      // gas.f:996: MAX(Hmin, DeltaMin)
  else if (rpar[2] > 0.0) r->hstart = rpar[2];
  else return -3;
  double* fac[4] = {&r->facmin, &r->facmax, &r->facrej, &r->facsafe};
  const double fac_default[4] = {0.2, 6.0, 0.1, 0.9};
  for (int i = 0; i < 4; i++) {                                   // gas.f:1006-1043
    if (rpar[3 + i] == 0.0) *fac[i] = fac_default[i];
    else if (rpar[3 + i] > 0.0) *fac[i] = rpar[3 + i];
    else return -4;
  }
  const double roundoff = 2.220446049250313e-16;                  // epsilon(ONE), gas.f:973
  const int uplim = r->vector ? kMech[mech].dims.nvar : 1;
  for (int i = 0; i < uplim; i++)                                 // gas.f:1045 (written so that a NaN passes, as it does there)
    if (atol[i] <= 0.0 || rtol[i] <= 10.0 * roundoff || rtol[i] >= 1.0) return -5;
  return 1;
}

std::string options_refusal(int mech, int ierr) {
  return rosenbrock_name(mech) + " would refuse these options, IERR = " + std::to_string(ierr) + " " + ros_error_text(ierr);
}
int method_built(int mech, const int32_t* ipar) {
  static const char* names[6] = {"Ros4 (IPAR(4) = 0 selects it)", "Ros2", "Ros3", "Ros4", "Rodas3", "Rodas4"};
  if (ipar[3] == 2) return 0;
  return fail(std::string("the ") + kMech[mech].name + " kernel is built for Ros3 (IPAR(4) = 2) only: " + names[ipar[3]] + " is a valid method of " +
              rosenbrock_name(mech) + " that this library does not have");
}

// the options block the options kernels read, from a decode that returned 1
std::vector<double> options_block(int mech, const RosResolved& r, const double* atol, const double* rtol) {
  const size_t nv = (size_t)kMech[mech].dims.nvar;
  std::vector<double> b((size_t)kOptTol + 2 * nv, 0.0);
  b[kOptHmin] = r.hmin; b[kOptHmax] = r.hmax; b[kOptHstart] = r.hstart;
  b[kOptFacMin] = r.facmin; b[kOptFacMax] = r.facmax; b[kOptFacRej] = r.facrej; b[kOptFacSafe] = r.facsafe;
  b[kOptAutonomous] = r.autonomous ? 1.0 : 0.0;
  for (size_t i = 0; i < nv; i++) {      // scalar tolerances: AbsTol(1), RelTol(1) for every species (gas.f:1363); the other entries are not read
    b[(size_t)kOptTol + i] = atol[r.vector ? i : 0];
    b[(size_t)kOptTol + nv + i] = rtol[r.vector ? i : 0];
  }
  return b;
}

// One call of Rosenbrock_x as its entry describes it: the plain call and whatever the entry's family adds to it.  Every extern "C" entry fills one of
// these and hands it to ros_host (host buffers: every array the caller's host array for the whole batch) or ros_device (device pointers).  Nothing of it is
// kept, nothing process-wide is read but Max_no_steps' default (mistra_chem_debug_set_max_steps, which ipar[2] /= 0 goes before).
struct RosRequest {
  int mech = 0, ncell = 0;
  const double *var_in = nullptr, *fix = nullptr, *rconst = nullptr;
  const double* env = nullptr;      // the integrate family: the rate evaluator's inputs in place of rconst, RCONST is made on the device
  double tstart = 0.0, tend = 0.0;
  // the call's own options; options = false: the integrate family, which runs under the options and the policy in force
  bool options = false;
  const double *atol = nullptr, *rtol = nullptr, *rpar = nullptr;
  const int32_t* ipar = nullptr;
  bool per_cell = false;            // the cells entries: atol, rtol are rows [ncell][ntol]; else the shared pair
  int ntol = 0;
  double* var_out = nullptr;        // a series: var_series [nleg][ncell][NVAR]; ierr, stats, th then hold nleg blocks as well
  int32_t *ierr = nullptr, *stats = nullptr;
  double* th = nullptr;             // host: [ncell][3]; device: [ncell][2]
  const double* hstart = nullptr;   // the first step size per cell
  bool record_sing = false;         // the host call records its zero-pivot rows for mistra_chem_singular_rows (the series does not)
  // the step-control trace
  bool trace = false;
  int cap = 0;
  double* trace_d = nullptr;
  int32_t *trace_i = nullptr, *ntrace = nullptr, *ctrl = nullptr;
  // every reaction's rate integrated over the call [ncell][NREACT]; a series with the flux: over each leg, [nleg][ncell][NREACT]
  bool wants_flux = false;
  double* flux = nullptr;
  // dense output: the state at ns sample times (ts: a host array) -> ysample [ns][ncell][NVAR], nout [ncell]
  bool dense = false;
  int ns = 0;
  const double* ts = nullptr;
  double* ysample = nullptr;
  int32_t* nout = nullptr;
  // a series: nleg legs over times[0 .. nleg] (a host array); rconst and fix in rconst_legs and fix_legs blocks (1 or nleg); lin: rconst holds nleg + 1
  // node blocks, linear in time over each leg
  int nleg = 0;
  bool series = false, lin = false;
  const double* times = nullptr;
  int carry_h = 0, rconst_legs = 1, fix_legs = 1;
  // the replay: hsteps [hrows][replay_cap], nsteps [hrows], err [ncell][replay_cap] or null.  hrows = 1: one sequence shared by all cells, host arrays
  bool replay = false;
  int replay_cap = 0, hrows = 0;
  const double* hsteps = nullptr;
  const int32_t* nsteps = nullptr;
  double* err = nullptr;

  bool own_rows() const { return replay && hrows != 1; }
  size_t legs() const { return series ? (size_t)nleg : 1; }
  RosRequest& cells(int n) { per_cell = true; ntol = n; return *this; }
  RosRequest& traced(int c, double* d, int32_t* i, int32_t* n, int32_t* ct) { trace = true; cap = c; trace_d = d; trace_i = i; ntrace = n; ctrl = ct; return *this; }
  RosRequest& with_flux(double* f) { wants_flux = true; flux = f; return *this; }
  RosRequest& sampled(int n, const double* t, double* y, int32_t* no) { dense = true; ns = n; ts = t; ysample = y; nout = no; return *this; }
  RosRequest& over(int n, const double* t, int carry, int rlegs = 1, int flegs = 1) { series = true; nleg = n; times = t; carry_h = carry; rconst_legs = rlegs; fix_legs = flegs; return *this; }
  RosRequest& linear() { lin = true; return *this; }
  RosRequest& replayed(int c, int rows, const double* h, const int32_t* n, double* e) { replay = true; replay_cap = c; hrows = rows; hsteps = h; nsteps = n; err = e; return *this; }
};
// the plain call of an entry with options of its own
RosRequest ros_request(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend, const double* atol,
                       const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr, int32_t* stats, double* th,
                       const double* hstart = nullptr) {
  RosRequest q;
  q.mech = mech; q.ncell = ncell; q.var_in = var_in; q.fix = fix; q.rconst = rconst; q.tstart = tstart; q.tend = tend;
  q.options = true; q.atol = atol; q.rtol = rtol; q.rpar = rpar; q.ipar = ipar;
  q.var_out = var_out; q.ierr = ierr; q.stats = stats; q.th = th; q.hstart = hstart;
  return q;
}

// the per-cell tolerance arguments, checked before anything touches a device: the widths are the entries' own rule, not codes of Rosenbrock_x
int check_cell_tol(const RosRequest& q) {
  if (!known_mech(q.mech)) return fail("unknown mechanism id");
  if (q.ncell < 0) return fail("negative cell count");
  if (!q.rpar || !q.ipar) return fail("null options pointer");
  if (!q.atol || !q.rtol) return fail("null tolerance array (atol / rtol: [ncell][ntol] each)");
  const int nv = kMech[q.mech].dims.nvar;
  if (q.ntol != 1 && q.ntol != nv) return fail("ntol = " + std::to_string(q.ntol) + ": a tolerance row holds 1 or NVAR = " + std::to_string(nv) + " entries");
  if (q.ipar[1] == 0 && q.ntol != nv) return fail("vector tolerances (ipar[1] = 0) need rows of NVAR = " + std::to_string(nv) + " entries, ntol = " + std::to_string(q.ntol));
  return 0;
}
// the arguments of the trace entries, checked before anything touches a device
int check_trace_args(const RosRequest& q) {
  if (q.cap < 0) return fail("negative trace capacity");
  if (!q.ntrace) return fail("null ntrace pointer");
  if (q.cap > 0 && (!q.trace_d || !q.trace_i)) return fail("trace capacity > 0 with a null trace_d or trace_i pointer");
  if (q.ipar[3] != 2) return fail("the step-control trace is built for Ros3 (ipar[3] = 2) only");
  return 0;
}
// arrays of a device entry that the kernel reads itself: memory the cells' device cannot reach is refused here, not met there
int check_reachable(std::initializer_list<const void*> arrays, int device, const char* refusal) {
  for (const void* p : arrays) {
    if (!p) continue;      // (hsteps with cap = 0)
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.type == hipMemoryTypeUnregistered || (attr.type == hipMemoryTypeDevice && attr.device != device))
      return fail(refusal);
  }
  return 0;
}

// What Rosenbrock_x's decode makes of a request's options.  Per-cell tolerances: the refusals -1 .. -4 depend on ipar / rpar alone and stay whole-call
// results decided here; -5 is then the kernel's, per cell, and the block's pair is a placeholder no kernel reads.
struct RosCall {
  int ierr = 1;                   // the decode's: 1, or the refusal -1 .. -5
  int method = kRos3;             // IPAR(4), 0 resolved to Ros4 (gas.f:1057)
  int max_steps = 0;
  bool vector = false;            // IPAR(2) = 0: every entry of a tolerance row is read; else entry 0 alone
  std::vector<double> block;      // the options block the kernel reads (kernel_args.hpp: RosOptSlot)
};
RosCall decode_call(const RosRequest& q) {
  RosCall c;
  RosResolved r;
  const double *atol = q.atol, *rtol = q.rtol;
  std::vector<double> one_a, one_r;
  if (q.per_cell) {
    one_a.assign((size_t)kMech[q.mech].dims.nvar, 1.0);
    one_r.assign((size_t)kMech[q.mech].dims.nvar, 1.0e-3);
    atol = one_a.data(); rtol = one_r.data();
    c.vector = q.ipar[1] == 0;
  }
  c.ierr = resolve_options(q.mech, q.ipar, q.rpar, atol, rtol, &r);
  if (c.ierr != 1) return c;
  c.method = q.ipar[3] == 0 ? (int)kRos4 : (int)q.ipar[3];
  c.max_steps = q.ipar[2] ? q.ipar[2] : g_max_steps;
  c.block = options_block(q.mech, r, atol, rtol);
  return c;
}

// The block of a call: its options, then the tail its family reads through the same pointer — the series' times, the dense sample times, or a replay's
// shared sequence with its count in the first half of one more word.  at = nullptr: nothing is written.  -> the words of the block and where the tail and
// the count word lie in it: the one convention for both paths
struct BlockLayout {
  size_t words = 0, tail = 0, count = 0;
};
BlockLayout put_block(double* at, const RosCall& call, const RosRequest& q) {
  const size_t nb = call.block.size();
  const double* from = q.series ? q.times : q.dense ? q.ts : q.hsteps;
  const size_t n = q.series ? (size_t)q.nleg + 1 : q.dense ? (size_t)q.ns : q.replay && !q.own_rows() ? (size_t)q.nsteps[0] : 0;      // (check_replay: 0 .. cap)
  const bool counted = q.replay && !q.own_rows();
  if (at) {
    std::memcpy(at, call.block.data(), nb * sizeof(double));
    if (n) std::memcpy(at + nb, from, n * sizeof(double));      // read here: the caller's array is free when the call returns
    if (counted) {
      at[nb + n] = 0.0;
      std::memcpy(at + nb + n, q.nsteps, sizeof(int32_t));
    }
  }
  return BlockLayout{nb + n + (counted ? 1 : 0), nb, nb + n};
}

// The kernel of a call: the VARIANT from the arguments (the replay, else dense output, else a series — with linear rates, with the flux of every leg or plain —, else the flux, else the trace, else a method other than Ros3, else the product unit's
// kernels), one guard, one slot of the mechanism's table.  A method other than Ros3 never runs as a quiet Ros3: what is not built is refused.
int launch(DeviceState& D, int mech, const KernelArgs& a, hipStream_t stream, int method = kRos3) {
  static const struct { const char *user, *refusal; } kText[kVariants] = {
      {}, {}, {},
      {"kernel for this Rosenbrock method (Ros2, Ros4, Rodas3, Rodas4)", "no kernel for this Rosenbrock method"},
      {"step-control trace", "no trace kernel for this Rosenbrock method"},
      {"series of Rosenbrock_x calls", "no series kernel for this Rosenbrock method"},
      {"reaction-flux entries", "no flux kernel for this Rosenbrock method"},
      {"dense-output entries", "no dense-output kernel for this Rosenbrock method"},
      {},      // (8, the operators: launch_ops, not an integration)
      {"replay entries", "no replay kernel for this mechanism"},
      {"series of Rosenbrock_x calls", "no series kernel with rate constants linear in time for this Rosenbrock method"},
      {"reaction-flux entries", "no series kernel with the reaction flux for this Rosenbrock method"}};
  const MechDesc& M = kMech[mech];
  const int variant = a.replay_n ? 9 : a.dense_nout ? 7 : a.times ? (a.lin_rates ? 10 : a.flux ? 11 : 5) : a.flux ? 6 : a.ntrace ? 4 : method != kRos3 ? 3 : 0;
  hipError_t e = hipErrorInvalidValue;
  if (variant) {
    if (M.user) return fail_user_slot(mech, kText[variant].user);
    const bool other = variant >= 5 && a.ntrace;      // (the trace is not an argument of a series or of the flux)
    if (method < kRos2 || method > kRodas4 || !M.unit.fn[variant][method] || !a.opt || a.dump || a.prof || other) return fail(kText[variant].refusal);
    e = M.unit.fn[variant][method](a, stream, &D.lds_configured[mech][variant][method]);
  } else {
    e = M.ros3(a, stream, &D.lds_configured[mech][0][0]);
  }
  if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

KernelArgs make_args(const MechState& S, int ncell, const double* var_in, const double* fix, const double* rconst, double tin,
                     double tout, double* var_out, int32_t* ierr, int32_t* stats, double* th) {
  const KernelBufs& k = S.k;
  KernelArgs a;
  a.var_in = var_in; a.fix = fix; a.rconst = rconst; a.var_out = var_out; a.ierr = ierr; a.stats = stats;
  a.texit_hexit = th; a.h_last = nullptr; a.hstart = nullptr; a.prof = nullptr; a.dump = nullptr; a.sing_rows = nullptr; a.n_temps = k.n_temps; a.max_steps = S.opt_max_steps ? S.opt_max_steps : g_max_steps; a.tin = tin; a.tout = tout; a.ncell = ncell;
  a.consts = k.consts.p; a.fun_fac = k.fun_fac.p; a.jac_fac = k.jac_fac.p; a.jvs_pos = k.jvs_pos.p;
  a.zero_pos = k.zero_pos.p; a.diag_pos = k.diag_pos.p;
  a.vdot = k.vdot.dev(); a.vdot_pass = k.vdot_pass.dev(); a.vdot_chain_mask = k.vdot_chain_mask.p; a.jvs = k.jvs.dev(); a.lu = k.lu.dev();
#ifdef MISTRA_DIAG_ENV      // diagnostic builds only (tools/diag_dense.sh env): never in the product library
  if (const char* cut = std::getenv("MISTRA_DIAG_LU_ROUNDS"))      // timing diagnostic (tools/profile_lu_rounds.py): results are garbage
    a.lu.nrounds = std::max(1, std::min(a.lu.nrounds, std::atoi(cut)));
#endif
  a.solve_head_fwd = k.solve_head_fwd.dev(); a.solve_head_bwd = k.solve_head_bwd.dev();
  a.tail = TailDev{k.tail_fwd.p, k.tail_bwd.p, {k.tail_fwd_addr[0].p, k.tail_fwd_addr[1].p}, {k.tail_bwd_addr[0].p, k.tail_bwd_addr[1].p}};
  a.lu_scale = ScaleDev{k.lu_scale.p, k.lu_scale_slots, k.lu_scale_slots + VM_LOOKAHEAD_ROWS};
  a.dense = DenseDev{k.dense_rows.p, k.schur_cells.p};
  a.trace_d = nullptr; a.trace_i = nullptr; a.ntrace = nullptr; a.ctrl = nullptr; a.trace_cap = 0;      // (the trace entries set them)
  a.tol_abs = nullptr; a.tol_rel = nullptr; a.tol_cell_stride = 0; a.tol_spec_stride = 0;      // (the cells entries set them)
  a.tol_cell_factor = 0.0; a.tol_cell_floor = 0.0;      // (policy_args sets them)
  a.times = nullptr; a.nleg = 0; a.carry_h = 0; a.leg_var = a.leg_ierr = a.leg_stats = a.leg_th = a.leg_h = 0; a.leg_rconst = a.leg_fix = 0;      // (the series entries set them)
  a.flux = nullptr;      // (the flux entries set it)
  a.dense_out = nullptr; a.dense_nout = nullptr; a.dense_ns = 0; a.dense_block = 0;      // (the dense-output entries set them)
  a.ops_vdot = nullptr; a.ops_jvs = nullptr; a.ops_x = nullptr; a.ops_rhs = nullptr; a.ops_shift = nullptr; a.ops_ising = nullptr;      // (the operator entries set them)
  a.ops_shift_stride = 0; a.ops_fun_rhs = 0; a.ops_nrhs = 0; a.ops_x_block = a.ops_rhs_block = 0;
  a.replay_h = nullptr; a.replay_n = nullptr; a.replay_h_stride = 0; a.replay_cap = 0; a.replay_err = nullptr;      // (the replay entries set them)
  a.lin_rates = 0;      // (the series entries with rate constants linear in time set it)
  a.leg_flux = 0;       // (the series entries with the reaction flux set it)
  a.opt = S.opt.p;      // set: the options instantiation of the kernel runs (ros3_kernel.hip: launch_ros3), also where the values equal INTEGRATE_x's
  return a;
}

// The integrator policy of the slot laid over the arguments of an entry that carries no options of its own (the integrate family, the column driver,
// the COMMON-block entry) -> the method to launch.  No policy: nothing changes, Ros3.  The entries whose options travel with the call and the Ros3
// diagnostics (first-step dump, phase timing) do not come here.
int policy_args(const MechState& S, KernelArgs* a) {
  if (!S.pol_method) return kRos3;
  if (!a->opt) a->opt = S.pol_opt.p;      // INTEGRATE_x's values: a policy runs the options instantiations
  a->tol_cell_factor = S.pol_factor; a->tol_cell_floor = S.pol_floor;
  return S.pol_method;
}

PackDev pack_dev(const MechState& S) { return S.pack.dev(S.tab.nreact, S.k.consts.p); }

// user_ok: the entry exists for a user slot (the integrate family); every other entry refuses one here, before it looks at a device
int check_call(int mech, int ncell, bool user_ok = false, const char* what = "such routine") {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (kMech[mech].user && !user_ok) return fail_user_slot(mech, what);
  if (ncell < 0) return fail("negative cell count");
  if (g_inited && !g_devs.empty() && kMech[mech].user && !g_devs[0].mech[mech].ready)
    return fail(std::string("user mechanism slot ") + std::to_string(mech - kBuiltinMechs) + ": " + kMech[mech].name + ".mech was not in the mechanism directory (" + mech_dir() +
                ") when mistra_chem_init ran");
  if (!g_inited || g_devs.empty() || !g_devs[0].mech[mech].ready) return fail("mistra_chem_init has not been called (or failed)");
  return 0;
}

// the groups of tables an entry needs are there
int require(const MechState& S, int mech, unsigned need) {
  const std::string m = kMech[mech].name;
  if ((need & kNeedPackTable) && !S.pack.ready) return fail("no hand-over table for the " + m + " mechanism");
  if ((need & kNeedMaps) && !S.pack.maps_ready) return fail("mistra_chem_set_species_maps has not been called for the " + m + " mechanism");
  if ((need & kNeedRates) && !S.rates.ready) return fail("no device rate table for the " + m + " mechanism");
  if ((need & kNeedKmt) && !S.kmt.ready) return fail("the " + m + " mechanism has no mass-transfer routine (fast_k_mt_a: aer, fast_k_mt_t: tot)");
  if ((need & kNeedLiq) && !S.liq.ready)
    return fail("the " + m + " mechanism has no liquid-phase routines (henry_a / equil_co_a: aer, henry_t / equil_co_t: tot)");
  if ((need & kNeedStc) && !S.stc.ready) return fail("the " + m + " mechanism has no st_coeff routine (st_coeff_a: aer, st_coeff_t: tot)");
  if ((need & kNeedVmean) && !S.vmean.ready) return fail("the " + m + " mechanism has no v_mean routine (v_mean_a: aer, v_mean_t: tot)");
  return 0;
}

struct Slot {
  DeviceState* D = nullptr;
  MechState* S = nullptr;
};

// The preamble of a device-pointer entry: the buffers decide the device.  The call runs on the slot `p` lives on — the first slot set up
// on that device — with the tables `need` names; the calling thread is switched to that device.
int on_device(int mech, int ncell, const void* p, const char* what, unsigned need, Slot* t) {
  if (int rc = check_call(mech, ncell, need == 0)) return rc;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) return fail(std::string(what) + " is not a device pointer");
  DeviceState* D = nullptr;
  for (auto& d : g_devs)
    if (d.id == attr.device) { D = &d; break; }
  if (!D) return fail("the buffers live on device " + std::to_string(attr.device) + ", which mistra_chem_init(_devices) did not set up");
  if (int rc = require(D->mech[mech], mech, need)) return rc;
  HIP_TRY(hipSetDevice(D->id));
  *t = Slot{D, &D->mech[mech]};
  return 0;
}

// The primary slot for a host-buffer entry (the caller holds g_mu), with the tables `need` names.  `mutates`: the entry changes the
// mechanism's staging, species maps or singular-row record, which a column step issued by mistra_chem_drive_begin may still be using —
// refused while such a step is open.
int step_is_open(int mech) {
  return fail(std::string("a column step of the ") + kMech[mech].name + " mechanism is open (mistra_chem_drive_begin): fetch it with mistra_chem_drive_end first");
}
int on_primary(int mech, unsigned need, bool mutates, Slot* t) {
  DeviceState& D = g_devs[0];
  MechState& S = D.mech[mech];
  if (mutates && S.pend.active) return step_is_open(mech);
  if (int rc = require(S, mech, need)) return rc;
  HIP_TRY(hipSetDevice(D.id));
  *t = Slot{&D, &S};
  return 0;
}

int init_locked(int n, const int* ids) {
  read_step_env();
  if (int rc = read_policy_env()) return rc;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) return fail("no HIP device available (this library has no CPU path)");
  if (n <= 0 || n > 64) return fail("device count out of range");      // (more slots than GPUs is legal: a device may be listed more than once)
  std::vector<int> want((size_t)n);
  for (int i = 0; i < n; i++) {
    want[(size_t)i] = ids ? ids[i] : i;
    if (want[(size_t)i] < 0 || want[(size_t)i] >= count) return fail("device index out of range");
    // (a device may be listed more than once: every listing is a slot of its own — tables, staging buffers, host thread —
    //  so two blocks of one batch overlap their copies with each other's kernel on that GPU; include/mistra_chem.h)
  }
  bool same = g_inited && g_devs.size() == want.size();
  for (size_t i = 0; same && i < want.size(); i++) same = g_devs[i].id == want[i];
  if (same) {
    HIP_TRY(hipSetDevice(g_devs[0].id));
    return 0;
  }
  release_all();
  g_devs.resize(want.size());
  for (size_t i = 0; i < want.size(); i++) {
    HIP_TRY(hipSetDevice(want[i]));
    g_devs[i].id = want[i];
    for (int mech = 0; mech < kNumMechs; mech++)
      if (int rc = setup_mech(g_devs[i], mech)) return rc;
  }
  HIP_TRY(hipSetDevice(g_devs[0].id));      // the calling thread ends up on the primary device
  g_inited = true;
  return 0;
}

// A host-buffer batch over the device slots (cell_split.hpp): block(slot, start, count) -> 0 or the refusal, whole on slot 0 where the batch is not
// split.  The calling thread ends up on the primary device.  -> 0, the unsplit block's refusal as it is, or the first failed slot's behind "device N: "
template <class F>
int on_cell_blocks(int ncell, F&& block) {
  std::vector<std::string> errs(g_devs.size());
  const std::vector<int> rcs = run_cell_blocks(ncell, (int)g_devs.size(), [&](int d, size_t start, int count) {
    const int rc = block(g_devs[(size_t)d], start, count);
    if (rc) errs[(size_t)d] = g_err;      // g_err is thread-local: carry the text to the caller's thread
    return rc;
  });
  (void)hipSetDevice(g_devs[0].id);
  if (rcs.size() == 1) return rcs[0];      // (this thread ran it: g_err is its text)
  for (size_t d = 0; d < rcs.size(); d++)
    if (rcs[d]) return fail("device " + std::to_string(g_devs[d].id) + ": " + errs[d]);
  return 0;
}

// The one binder: what a request adds to make_args' arguments.  `at` is the request with every array where the kernel reads it — the caller's device
// arrays (ros_device) or this slot's staging of its `nc` cells (ros_host_on); `block` the device address of the call's block (call = nullptr: the integrate
// family, which has none and keeps the options in force).  The only place these members are assigned outside make_args.
void bind_request(KernelArgs* a, const RosRequest& at, const RosCall* call, const double* block, const BlockLayout& L, size_t nc, double* h_last,
                  int32_t* sing_rows) {
  const MechDims& dims = kMech[at.mech].dims;
  const int64_t nv = (int64_t)nc * dims.nvar, nf = (int64_t)nc * dims.nfix, nr = (int64_t)nc * dims.nreact;
  a->hstart = at.hstart;
  a->h_last = h_last;
  a->sing_rows = sing_rows;      // stays on the device: fetched by mistra_chem_singular_rows, i.e. only when a cell reports Nsng > 0
  if (call) {
    a->opt = block;
    a->max_steps = call->max_steps;
  }
  if (at.per_cell) {      // device rows [nc][ntol]
    a->tol_abs = at.atol; a->tol_rel = at.rtol;
    a->tol_cell_stride = at.ntol;
    a->tol_spec_stride = call->vector ? 1 : 0;
  }
  if (at.trace) { a->trace_cap = at.cap; a->trace_d = at.trace_d; a->trace_i = at.trace_i; a->ntrace = at.ntrace; a->ctrl = at.ctrl; }
  a->flux = at.flux;
  if (at.dense) { a->times = block + L.tail; a->dense_out = at.ysample; a->dense_nout = at.nout; a->dense_ns = at.ns; a->dense_block = nv; }
  if (at.series) {
    a->times = block + L.tail; a->nleg = at.nleg; a->carry_h = at.carry_h ? 1 : 0;
    a->leg_var = nv; a->leg_ierr = (int64_t)nc; a->leg_stats = (int64_t)nc * 8; a->leg_th = (int64_t)nc * 2; a->leg_h = (int64_t)nc;
    a->leg_rconst = at.rconst_legs > 1 || at.lin ? nr : 0;      // the stride of the blocks the kernel reads, at the head of every leg
    a->leg_fix = at.fix_legs > 1 ? nf : 0;
    a->lin_rates = at.lin ? 1 : 0;      // (... of every evaluation: the node blocks, nleg + 1 of them)
    if (at.flux) a->leg_flux = nr;      // selects the series kernels with the flux (launch)
  }
  if (at.replay) {      // selects the replay kernel (launch); a shared sequence and its count lie in the block
    const bool own = at.own_rows();
    a->replay_cap = at.replay_cap;
    a->replay_h = own ? at.hsteps : block + L.tail;
    a->replay_n = own ? at.nsteps : reinterpret_cast<const int32_t*>(block + L.count);
    a->replay_h_stride = own ? (int64_t)at.replay_cap : 0;
    a->replay_err = at.replay_cap ? at.err : nullptr;
  }
}

// ---- staging of a host-buffer call as data: one entry per array that crosses PCIe for this slot's cells [start, start + nc) of the caller's `total`.
//      The caller's array is [blocks][total][bytes per cell], the slot's [blocks][nc][bytes per cell]; `shared`: one row for the whole batch (the block).
struct Staged {
  const void* up;      // the caller's array that goes up before the kernel, or null
  void* down;          // ... that is fetched behind it, or null
  void* dev;
  size_t bytes, blocks;
  bool shared;
};
struct StageList {
  size_t start, nc, total;
  std::vector<Staged> v;
  hipError_t err = hipSuccess;
  // `want`: the request has this array.  Reserves `room` elements of b (0: what the array needs behind `at`), points `slot` — the array's member of the
  // request the binder reads — at element `at` of it, and lists the copies.  Not wanted: slot = null, nothing else
  template <class T, class P>
  void add(DevBuf<T>& b, P& slot, size_t words, size_t blocks, const std::common_type_t<T>* up, std::common_type_t<T>* down, bool want = true, size_t at = 0, size_t room = 0, bool shared = false) {
    slot = nullptr;
    if (!want || err != hipSuccess) return;
    err = b.reserve(room ? room : at + blocks * (shared ? 1 : nc) * words);
    slot = b.p + at;
    if (up || down) v.push_back(Staged{up, down, b.p + at, words * sizeof(T), blocks, shared});
  }
  // one block: a plain copy; several blocks of a batch: the slot's cells of each, one strided copy
  hipError_t copy(const Staged& s, bool to_device) const {
    const size_t row = (s.shared ? 1 : nc) * s.bytes, off = s.shared ? 0 : start * s.bytes;
    if (!row) return hipSuccess;
    if (to_device) {
      const char* src = static_cast<const char*>(s.up) + off;
      return s.blocks == 1 ? hipMemcpy(s.dev, src, row, hipMemcpyHostToDevice) : hipMemcpy2D(s.dev, row, src, total * s.bytes, row, s.blocks, hipMemcpyHostToDevice);
    }
    char* dst = static_cast<char*>(s.down) + off;
    return s.blocks == 1 ? hipMemcpy(dst, s.dev, row, hipMemcpyDeviceToHost) : hipMemcpy2D(dst, total * s.bytes, s.dev, row, row, s.blocks, hipMemcpyDeviceToHost);
  }
};

// the kernel of a host-buffer call and the wait for it
int launch_and_wait(DeviceState& D, int mech, const KernelArgs& a, int method) {
  if (int rc = launch(D, mech, a, nullptr, method)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
#ifdef MISTRA_DIAG_ENV
// diagnostic builds only (-DMISTRA_DIAG_ENV, tools/diag_dense.sh env): MISTRA_CHEM_PROFILE=1 prints where wave 0 of the
// workgroups spent its cycles (mean over the cells of the call).  The product library does not read the environment here.
int launch_profiled(DeviceState& D, int mech, KernelArgs a, int method, size_t nc) {
  if (a.opt) return fail("the profiling kernel keeps INTEGRATE_x's values: clear the options (mistra_chem_set_options) first");
  DevBuf<unsigned long long> prof;
  HIP_TRY(prof.reserve(nc * kProfStride));
  HIP_TRY(hipMemset(prof.p, 0, nc * kProfStride * sizeof(unsigned long long)));      // (a workgroup of fewer than kProfWaves waves leaves the rest unwritten)
  a.prof = prof.p;
  if (int rc = launch_and_wait(D, mech, a, method)) return rc;
  std::vector<unsigned long long> h(nc * kProfStride);
  HIP_TRY(hipMemcpy(h.data(), prof.p, nc * kProfStride * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double sum[kProfStride] = {0};
  for (size_t c = 0; c < nc; c++)
    for (int k = 0; k < kProfStride; k++) sum[k] += (double)h[c * kProfStride + k];
  const char* names[kProfSlots] = {"fun", "jac", "prepare", "lu", "solve(rest)", "norm", "other", "total", "solve_head_fwd", "solve_tail", "solve_head_bwd", "lu_scale", "lu_dense", "jac_products", "jac_sums", "fun_products"};
  std::fprintf(stderr, "[mistra_chem profile] %s, %zu cells, mean shader-clock ticks per cell:", kMech[mech].name, nc);
  for (int k = 0; k < kProfSlots; k++) std::fprintf(stderr, " %s=%.0f (%.1f%%)", names[k], sum[k] / nc, 100.0 * sum[k] / sum[7]);
  std::fprintf(stderr, "\n");
  // the gather-sum machine per wave (kernel_args.hpp: kProfStride): mean ticks per call since wave 0 entered the evaluator.  The sums'
  // barrier opens when the last wave reaches the call, so `sums` = left - latest reach is the wave's own fill, rows and drain, and
  // `waits` = latest left - left is what the wave then idles at the next barrier behind the slowest one.
  const char* evaluator[2] = {"fun", "fun_jac"};
  for (int e = 0; e < 2; e++) {
    const double calls = sum[kProfSlots + 4 * kProfWaves + e];
    if (calls <= 0) continue;
    double reach[kProfWaves], left[kProfWaves], opens = 0, last = 0;
    for (int w = 0; w < kProfWaves; w++) {
      reach[w] = sum[kProfSlots + 4 * w + 2 * e] / calls;
      left[w] = sum[kProfSlots + 4 * w + 2 * e + 1] / calls;
      opens = std::max(opens, reach[w]);
      last = std::max(last, left[w]);
    }
    std::fprintf(stderr, "[mistra_chem profile] %s, sums per wave: %.1f calls per cell, ticks per call, barrier opens at %.0f:", evaluator[e], calls / nc, opens);
    for (int w = 0; w < kProfWaves; w++)
      if (left[w] > 0) std::fprintf(stderr, " w%d reach=%.0f left=%.0f sums=%.0f waits=%.0f |", w, reach[w], left[w], left[w] - opens, last - left[w]);
    std::fprintf(stderr, "\n");
  }
  prof.release();
  return 0;
}
#endif

// One device slot's share of a host-buffer call (ros_host): cells [start, start + nc) of the request's batch up, the kernel, the results down,
// synchronous on that device.  call = nullptr: the integrate family.  Every upload of the slot precedes its downloads and slots own disjoint cells, so
// var_in may alias var_out (one leg's block of it in a series).
int ros_host_on(DeviceState& D, const RosRequest& q, const RosCall* call, const std::vector<double>& blk, const BlockLayout& L, size_t start, size_t nc) {
  HIP_TRY(hipSetDevice(D.id));
  MechState& S = D.mech[q.mech];
  const MechDims& dims = kMech[q.mech].dims;
  const size_t nv = (size_t)dims.nvar, nf = (size_t)dims.nfix, nr = (size_t)dims.nreact, ne = q.env ? (size_t)S.rates.nenv : 0;
  const size_t nl = q.legs(), cap = (size_t)q.cap, rcap = (size_t)q.replay_cap, ntol = (size_t)q.ntol;
  const size_t nlr = q.lin ? nl + 1 : (size_t)q.rconst_legs;      // the node blocks: one more than there are legs
  const bool own = q.own_rows(), keep_err = q.err && rcap;
  const size_t o_err = own ? nc * rcap : 0, rp_room = o_err + (keep_err ? nc * rcap : 0);      // one arena: the cells' own rows | their Err rows
  RosRequest at = q;      // every array where this slot keeps its cells of it
  at.ts = at.times = nullptr;      // (in the block)
  const double* block = nullptr;
  int32_t* sing = nullptr;
  StageList st{start, nc, (size_t)q.ncell, {}};
  st.v.reserve(24);
  // Caller output arrays that go up are the ones the kernel writes in part: the trace logs, ctrl under per-cell tolerances (a cell refused with -5 writes
  // no row) and the replay's err rows come back as they were where it wrote nothing.  The flux and the samples are written whole: nothing goes up.
  st.add(S.s_var, at.var_in, nv, 1, q.var_in, q.series ? nullptr : q.var_out);      // (the single calls integrate in place)
  st.add(S.s_fix, at.fix, nf, (size_t)q.fix_legs, q.fix, nullptr);
  st.add(S.s_env, at.env, ne, 1, q.env, nullptr, q.env != nullptr);                 // (the caller has checked that the mechanism has a rate table)
  st.add(S.s_rct, at.rconst, nr, nlr, q.env ? nullptr : q.rconst, nullptr);
  st.add(S.call_opt, block, L.words, 1, blk.data(), nullptr, call != nullptr, 0, 0, true);
  st.add(S.s_ser_var, at.var_out, nv, nl, nullptr, q.var_out, q.series);
  if (!q.series) at.var_out = S.s_var.p;
  st.add(S.s_ierr, at.ierr, 1, nl, nullptr, q.ierr);
  st.add(S.s_stats, at.stats, 8, nl, nullptr, q.stats);
  st.add(S.s_sing, sing, 8, 1, nullptr, nullptr, q.record_sing);
  st.add(S.s_rp, at.hsteps, rcap, 1, q.hsteps, nullptr, own && rcap, 0, rp_room);
  st.add(S.s_ntr, at.nsteps, 1, 1, q.nsteps, nullptr, own);
  st.add(S.s_rp, at.err, rcap, 1, q.err, q.err, q.replay && keep_err, o_err, rp_room);
  st.add(S.s_tol, at.atol, ntol, 1, q.atol, nullptr, q.per_cell, 0, 2 * nc * ntol);
  st.add(S.s_tol, at.rtol, ntol, 1, q.rtol, nullptr, q.per_cell, nc * ntol, 2 * nc * ntol);
  st.add(S.s_ntr, at.ntrace, 1, 1, nullptr, q.ntrace, q.trace);
  st.add(S.s_trd, at.trace_d, cap * 4, 1, q.trace_d, q.trace_d, q.trace && cap);
  st.add(S.s_tri, at.trace_i, cap * 2, 1, q.trace_i, q.trace_i, q.trace && cap);
  st.add(S.s_ctl, at.ctrl, nv, 1, q.per_cell ? q.ctrl : nullptr, q.ctrl, q.trace && q.ctrl);
  st.add(S.s_flux, at.flux, nr, nl, nullptr, q.flux, q.flux != nullptr);
  st.add(S.s_dn_y, at.ysample, nv, (size_t)q.ns, nullptr, q.ysample, q.dense);
  st.add(S.s_dn_n, at.nout, 1, 1, nullptr, q.nout, q.dense);
  st.add(S.s_hst, at.hstart, 1, 1, q.hstart, nullptr, q.hstart != nullptr);
  st.add(S.s_th, at.th, 3, nl, nullptr, nullptr, q.th || q.replay);      // device: [legs][nc][2] (T, Hexit) then [legs][nc] (H); fetched below
  HIP_TRY(st.err);
  for (const Staged& s : st.v)
    if (s.up) HIP_TRY(st.copy(s, true));
  if (q.env) LAUNCH_TRY(launch_update_rconst(S.rates.dev(), at.env, S.s_rct.p, (int)nc, nullptr));
  const double t0 = q.series ? q.times[0] : q.tstart, t1 = q.series ? q.times[q.nleg] : q.tend;
  KernelArgs a = make_args(S, (int)nc, at.var_in, at.fix, at.rconst, t0, t1, at.var_out, at.ierr, at.stats, at.th);
  bind_request(&a, at, call, block, L, nc, at.th ? at.th + 2 * nl * nc : nullptr, sing);
  const int method = call ? call->method : policy_args(S, &a);
  if (q.record_sing) { S.sing_start = start; S.sing_count = nc; S.sing_one = false; }
#ifdef MISTRA_DIAG_ENV
  if (std::getenv("MISTRA_CHEM_PROFILE") && !q.series && !q.replay) {
    if (int rc = launch_profiled(D, q.mech, a, method, nc)) return rc;
  } else
#endif
  if (int rc = launch_and_wait(D, q.mech, a, method)) return rc;
  for (const Staged& s : st.v)
    if (s.down) HIP_TRY(st.copy(s, false));
  if (q.th) {      // the slot's [legs][nc][2] and [legs][nc]  ->  the caller's [legs][total][3]
    std::vector<double> h(nl * nc * 3);
    HIP_TRY(hipMemcpy(h.data(), at.th, nl * nc * 3 * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nl; k++)
      for (size_t c = 0; c < nc; c++) {
        double* o = q.th + (k * st.total + start + c) * 3;
        o[0] = h[(k * nc + c) * 2]; o[1] = h[(k * nc + c) * 2 + 1]; o[2] = h[2 * nl * nc + k * nc + c];
      }
  }
  return 0;
}

// ---- one column step on the device: x_drive for a batch of layers

// where the step's arrays live: caller buffers (mistra_chem_drive_device) or parts of the drive arena (mistra_chem_drive_begin)
struct ColumnDev {
  double *s1, *s3, *sl1, *sion1;
  const double* scal;
  double *env, *var, *fix, *rct;
  int32_t *ierr, *stats;
  double* th;
  double *bg, *bgs;             // budgets, each may be nullptr
  double *c_packed, *h_last;    // nullptr unless wanted
  int32_t* sing_rows;           // nullptr unless wanted
  // step reuse (mem != nullptr): the batch's layer numbers on the device, where their first steps are gathered to, the mechanism's step memory [mem_n]
  const int32_t* layer;
  double* hstart;
  double* mem;
  int mem_n;
};

// pack -> (C as packed) -> env from C -> Update_RCONST_x -> INTEGRATE_x -> budgets -> unpack, in order on `st`; under step reuse the integrator starts every
// layer at the step size the memory holds for it, and the memory is then rewritten from this step: cleared, and Hexit of the layers that succeeded stored
int column_step(DeviceState& D, int mech, int ncell, const ColumnDev& c, double tin, double dt, hipStream_t st) {
  const MechState& S = D.mech[mech];
  const PackDev P = pack_dev(S);
  LAUNCH_TRY(launch_pack(P, ncell, c.s1, c.s3, c.sl1, c.sion1, c.scal, c.var, c.fix, st));
  if (c.c_packed) {      // [ncell][NVAR + NFIX]
    const size_t nv = (size_t)kMech[mech].dims.nvar, nf = (size_t)kMech[mech].dims.nfix, nl = (size_t)ncell;
    HIP_TRY(hipMemcpy2DAsync(c.c_packed, (nv + nf) * sizeof(double), c.var, nv * sizeof(double), nv * sizeof(double), nl, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpy2DAsync(c.c_packed + nv, (nv + nf) * sizeof(double), c.fix, nf * sizeof(double), nf * sizeof(double), nl, hipMemcpyDeviceToDevice, st));
  }
  LAUNCH_TRY(launch_env_from_c(P, ncell, S.rates.nenv, c.var, c.fix, c.env, st));
  LAUNCH_TRY(launch_update_rconst(S.rates.dev(), c.env, c.rct, ncell, st));
  KernelArgs a = make_args(S, ncell, c.var, c.fix, c.rct, tin, tin + dt, c.var, c.ierr, c.stats, c.th);
  a.h_last = c.h_last;
  a.sing_rows = c.sing_rows;
  if (c.mem) {
    LAUNCH_TRY(launch_step_gather(c.mem, c.mem_n, c.layer, ncell, c.hstart, st));
    a.hstart = c.hstart;
  }
  if (int rc = launch(D, mech, a, st, policy_args(S, &a))) return rc;
  if (c.mem) {
    HIP_TRY(hipMemsetAsync(c.mem, 0, (size_t)c.mem_n * sizeof(double), st));
    LAUNCH_TRY(launch_step_store(c.mem, c.mem_n, c.layer, ncell, c.ierr, c.th, st));
  }
  if (c.bg || c.bgs) LAUNCH_TRY(launch_budgets(P, ncell, c.var, c.fix, c.rct, dt, c.bg, c.bgs, st));
  LAUNCH_TRY(launch_unpack(P, ncell, c.var, c.s1, c.s3, c.sl1, c.sion1, st));
  return 0;
}

DriveLayout drive_layout(const MechState& S, int mech, size_t nl, bool bg, bool bgs, bool c_packed, bool reuse) {
  const PackTable& T = S.pack.tab;
  DriveLayout L;
  L.nl = nl; L.j1 = (size_t)S.pack.j1; L.j5 = (size_t)S.pack.j5; L.nsl = (size_t)T.j2 * T.nkc; L.nsi = (size_t)T.j6 * T.nkc;
  L.nv = (size_t)kMech[mech].dims.nvar; L.nf = (size_t)kMech[mech].dims.nfix; L.nr = (size_t)kMech[mech].dims.nreact; L.ne = (size_t)S.rates.nenv;
  const size_t d8 = sizeof(double), nb = 2 * (size_t)kBudSlots;
  Layout B;
  L.s1 = B.take(nl * L.j1 * d8); L.s3 = B.take(nl * L.j5 * d8); L.sl1 = B.take(nl * L.nsl * d8); L.si = B.take(nl * L.nsi * d8);
  L.bg = B.take(bg ? nl * 2 * L.nr * d8 : 0); L.bgs = B.take(bgs ? nl * nb * d8 : 0);
  L.io_end = B.end;
  L.scal = B.take(nl * 6 * d8); L.env = B.take(nl * L.ne * d8); L.lyr = B.take(reuse ? nl * sizeof(int32_t) : 0);
  L.in_end = B.end;
  L.th = B.take(nl * 2 * d8); L.hl = B.take(nl * d8); L.ierr = B.take(nl * sizeof(int32_t)); L.stats = B.take(nl * 8 * sizeof(int32_t));
  L.cp = B.take(c_packed ? nl * (L.nv + L.nf) * d8 : 0);
  L.out_end = B.end;
  L.var = B.take(nl * L.nv * d8); L.fix = B.take(nl * L.nf * d8); L.rct = B.take(nl * L.nr * d8); L.hs = B.take(reuse ? nl * d8 : 0);
  L.end = B.end;
  return L;
}

// ---- the host-buffer forms of the liq_parm kernels: what a Fortran caller reaches (shim/mistra_kpp_liq.f90).  A call gathers its inputs into the
//      pinned mirror of g_liq (or, for caller memory that mistra_chem_pin_host registered, leaves them where they are), sends them up, runs the
//      kernel on the arena's stream and fetches its outputs; one stream synchronisation per call, no allocation once the arena has grown to the
//      column's size.
struct DevBlock {      // the arrays of one call as parts of g_liq
  struct Part {
    size_t off, bytes;
    const void* src;      // where its input comes from (nullptr: not an input)
    void* dst;            // where its output goes (nullptr: not an output)
  };
  Layout L;
  std::vector<Part> parts;
  size_t add(size_t bytes) {
    parts.push_back(Part{L.take(bytes), bytes, nullptr, nullptr});
    return parts.size() - 1;
  }
  hipError_t alloc() { return g_liq.ensure(L.end ? L.end : 256); }
  double* dptr(size_t i) const { return g_liq.d(parts[i].off); }
  void up(size_t i, const void* from) { parts[i].src = from; }
  void down(size_t i, void* to) { parts[i].dst = to; }
  hipStream_t stream() const { return g_liq.st; }
  // every transfer costs ~15 us of latency in the stream whatever its size: neighbouring staged parts travel as ONE copy (the padding between them with
  // them), parts inside a registered caller range go straight from / to the caller's memory
  hipError_t transfer(bool upward) {
    auto end = [&](size_t i) { return upward ? parts[i].src : static_cast<const void*>(parts[i].dst); };
    size_t i = 0;
    while (i < parts.size()) {
      const void* p = end(i);
      if (!p) { i++; continue; }
      if (g_pinned.contains(p, parts[i].bytes)) {
        hipError_t e = upward ? hipMemcpyAsync(g_liq.dev + parts[i].off, p, parts[i].bytes, hipMemcpyHostToDevice, g_liq.st)
                              : hipMemcpyAsync(parts[i].dst, g_liq.dev + parts[i].off, parts[i].bytes, hipMemcpyDeviceToHost, g_liq.st);
        if (e != hipSuccess) return e;
        i++;
        continue;
      }
      size_t j = i;      // the run of staged parts i..j-1
      while (j < parts.size() && end(j) && !g_pinned.contains(end(j), parts[j].bytes)) {
        if (upward) std::memcpy(g_liq.host + parts[j].off, parts[j].src, parts[j].bytes);
        j++;
      }
      const size_t lo = parts[i].off, hi = parts[j - 1].off + parts[j - 1].bytes;
      hipError_t e = upward ? hipMemcpyAsync(g_liq.dev + lo, g_liq.host + lo, hi - lo, hipMemcpyHostToDevice, g_liq.st)
                            : hipMemcpyAsync(g_liq.host + lo, g_liq.dev + lo, hi - lo, hipMemcpyDeviceToHost, g_liq.st);
      if (e != hipSuccess) return e;
      i = j;
    }
    return hipSuccess;
  }
  hipError_t send() { return transfer(true); }      // after the last up(), before the kernel
  hipError_t finish() {       // after the last down(): fetch, wait, hand the staged outputs to the caller
    if (hipError_t e = transfer(false)) return e;
    if (hipError_t e = hipStreamSynchronize(g_liq.st)) return e;
    for (const Part& q : parts)
      if (q.dst && !g_pinned.contains(q.dst, q.bytes)) std::memcpy(q.dst, g_liq.host + q.off, q.bytes);
    return hipSuccess;
  }
};

// the arguments of fast_k_mt against the mechanism's table (the kernel's loop limits: checked here, on the host)
int kmt_args(const MechState& S, const int32_t* kw, int nkw, int ka, int ifeed, int nkc_l, KmtDev* K) {
  const KmtTable& T = S.kmt.tab;
  if (nkw != T.nka || T.nka > kKmtMaxNka) return fail("kw does not have nka entries");
  if (ka < 0 || ka > T.nka || nkc_l < 1 || nkc_l > T.nkc) return fail("ka / nkc_l out of range");
  *K = S.kmt.dev(S.tab.nvar + S.tab.nfix, ka, ifeed, nkc_l);
  for (int i = 0; i < T.nka; i++) {
    if (kw[i] < 0 || kw[i] > T.nkt) return fail("kw out of range");
    K->kw[i] = kw[i];
  }
  return 0;
}

int equil_co_check(const MechState& S, int nkc, int j6) {
  const LiqTable& T = S.liq.tab;
  if (nkc < T.nkc_eq) return fail("nkc is smaller than the number of bins the routine sets");
  for (size_t i = 0; i < T.fkind.size(); i++)
    if (T.fkind[i] == 3 && T.farg[i] > j6) return fail("j6 is smaller than an activity-coefficient index the routine reads");
  return 0;
}

}  // namespace

static int lazy_init();

extern "C" {

const char* mistra_chem_last_error(void) { return g_err.c_str(); }

int mistra_chem_dims(int mech, int* nvar, int* nfix, int* nreact, int* lu_nonzero) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (nvar) *nvar = kMech[mech].dims.nvar;
  if (nfix) *nfix = kMech[mech].dims.nfix;
  if (nreact) *nreact = kMech[mech].dims.nreact;
  if (lu_nonzero) *lu_nonzero = kMech[mech].dims.lu_nonzero;
  return 0;
}

int mistra_chem_user_mechs(void) { return MISTRA_USER_MECHS; }

const char* mistra_chem_mech_name(int mech) { return known_mech(mech) ? kMech[mech].name : nullptr; }

int mistra_chem_init(int device) {
  std::lock_guard<std::mutex> lock(g_mu);
  g_err.clear();
  return init_locked(1, &device);
}

int mistra_chem_init_devices(int n_devices, const int* device_ids) {
  std::lock_guard<std::mutex> lock(g_mu);
  g_err.clear();
  return init_locked(n_devices, device_ids);
}

int mistra_chem_device_count(void) { return g_inited ? (int)g_devs.size() : 0; }

void mistra_chem_finalize(void) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (auto& o : g_opts) o = RosOptions{};
  for (int m = 0; m < kMaxMechs; m++) g_policy[m] = g_policy_env[m];      // (what the environment asked for stays)
  release_all();
}

static std::map<int, std::pair<int, int>>& cache_dims() { static std::map<int, std::pair<int, int>> d; return d; }      // (nnz, nvar) of the mechanisms compiled below
// The gather-sum programs of a mechanism as the schedule compiler builds them (tests/test_gsum_chain.py restates them on the host).  Needs
// no device: the mechanism's table is read from the mechanism directory and compiled here, once per mechanism and process.
int mistra_chem_gsum_program(int mech, int which, int64_t* info, uint32_t* wave_base, int32_t* rows, uint64_t* mask, int32_t* chained,
                             int32_t* pass_wave, uint32_t* recs, int64_t recs_cap) {
  if (!known_mech(mech)) return fail("mistra_chem_gsum_program: no such mechanism");
  if (which < 0 || which > 3 || !info) return fail("mistra_chem_gsum_program: which = 0 Vdot (full) | 1 JVS | 2 Vdot (lean rows) | 3 Vdot (chain passes), info is required");
  static std::mutex mu;
  static std::map<int, KernelSchedule> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(mech);
  if (it == cache.end()) {
    const MechDesc& M = kMech[mech];
    MechTables tab;
    std::string err;
    if (!tab.load(mech_dir() + "/" + M.name + ".mech", &err)) return fail(err);
    try {
      const DenseConfig dc = M.user ? DenseConfig{0, 0} : dense_config(tab);
      it = cache.emplace(mech, build_kernel_schedule(tab, M.nt, M.ab_base, M.max_temps, dc.nd, dc.kb, M.jb_base, M.gsum_chain)).first;
    } catch (const std::exception& ex) {
      return fail(std::string("schedule compiler: ") + ex.what());
    }
    cache_dims()[mech] = {tab.nnz, tab.nvar};
  }
  const KernelSchedule& K = it->second;
  const GsumChain& C = K.vdot_chain;
  const GsumProgram& P = which == 0 ? K.vdot : which == 1 ? K.jvs : which == 2 ? C.lean : C.pass;
  const VmLayout lay{cache_dims()[mech].first, cache_dims()[mech].second, 0};
  const int64_t vals[14] = {P.nt, P.nw, P.nq, (int64_t)P.recs.size(), C.on ? 1 : 0, (int64_t)C.pass_wave.size(), C.pole_rows_full, C.pole_rows_lean,
                            C.pole_cycles_full, C.pole_cycles_lean, 8 * (int64_t)lay.zero(), 8 * (int64_t)lay.trash(),
                            which == 1 ? (int64_t)K.jb_base_bytes : (int64_t)K.ab_base_bytes, 8 * (int64_t)lay.xs()};
  std::memcpy(info, vals, sizeof vals);
  for (int w = 0; w < P.nw; w++) {
    if (wave_base) wave_base[w] = P.wave_base[(size_t)w];
    if (rows) rows[w] = P.rows[(size_t)w];
    if (mask) mask[w] = C.mask[(size_t)w];
  }
  for (size_t i = 0; i < C.outputs.size(); i++)
    if (chained) chained[i] = C.outputs[i];
  for (size_t i = 0; i < C.pass_wave.size(); i++)
    if (pass_wave) pass_wave[i] = C.pass_wave[i];
  if (recs) {
    if (recs_cap < (int64_t)P.recs.size()) return fail("mistra_chem_gsum_program: recs_cap is below info[3]");
    std::memcpy(recs, P.recs.data(), P.recs.size() * sizeof(uint32_t));
  }
  return 0;
}

const char* mistra_chem_describe(int mech) {
  if (!known_mech(mech) || !g_inited || g_devs.empty() || !g_devs[0].mech[mech].ready) return "";
  return g_devs[0].mech[mech].text.c_str();
}

int mistra_chem_integrate_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                 double tin, double tout, double* d_var_out, int32_t* d_ierr, int32_t* d_stats,
                                 double* d_texit_hexit, void* hip_stream) {
  return mistra_chem_integrate_device_hstart(mech, ncell, d_var_in, d_fix, d_rconst, tin, tout, d_var_out, d_ierr, d_stats, d_texit_hexit,
                                             nullptr, hip_stream);
}

int mistra_chem_integrate_device_hstart(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                        double tin, double tout, double* d_var_out, int32_t* d_ierr, int32_t* d_stats,
                                        double* d_texit_hexit, const double* d_hstart, void* hip_stream) {
  if (ncell == 0) return check_call(mech, 0, true);      // (nothing to do, but an uninitialised library says so)
  if (!d_var_in || !d_fix || !d_rconst || !d_var_out || !d_ierr || !d_stats) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var_in, "d_var_in", 0, &t)) return rc;
  KernelArgs a = make_args(*t.S, ncell, d_var_in, d_fix, d_rconst, tin, tout, d_var_out, d_ierr, d_stats, d_texit_hexit);
  a.hstart = d_hstart;
  return launch(*t.D, mech, a, static_cast<hipStream_t>(hip_stream), policy_args(*t.S, &a));
}

int mistra_chem_table_stack_depth(const char* path, int stcoeff) {
  if (!path) return fail("null path"), -1;
  std::string err;
  int depth = 0;
  bool ok;
  if (stcoeff) {
    StcoeffTable T;
    ok = T.load(path, &err);
    for (int i = 0; ok && i < 4; i++) depth = T.v[i].depth > depth ? T.v[i].depth : depth;
  } else {
    RatesTable T;
    ok = T.load(path, &err);
    depth = T.depth;
  }
  if (!ok) return fail(err), -1;
  return depth;
}

int mistra_chem_rates_env_size(int mech) {
  if (!known_mech(mech) || !g_inited || g_devs.empty() || !g_devs[0].mech[mech].rates.ready) return 0;
  return g_devs[0].mech[mech].rates.nenv;
}

int mistra_chem_update_rconst_device(int mech, int ncell, const double* d_env, double* d_rconst, void* hip_stream) {
  if (int rc = builtin_only(mech, "rate table")) return rc;
  if (ncell == 0) return check_call(mech, 0);
  if (!d_env || !d_rconst) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_env, "d_env", kNeedRates, &t)) return rc;
  LAUNCH_TRY(launch_update_rconst(t.S->rates.dev(), d_env, d_rconst, ncell, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_update_rconst(int mech, int ncell, const double* env, double* rconst) {
  if (int rc = builtin_only(mech, "rate table")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, ncell)) return rc;
  if (ncell == 0) return 0;
  if (!env || !rconst) return fail("null host pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, kNeedRates, true, &t)) return rc;
  MechState& S = *t.S;
  const size_t nc = (size_t)ncell, ne = (size_t)S.rates.nenv, nr = (size_t)S.tab.nreact;
  HIP_TRY(S.s_env.reserve(nc * ne));
  HIP_TRY(S.s_rct.reserve(nc * nr));
  HIP_TRY(hipMemcpy(S.s_env.p, env, nc * ne * sizeof(double), hipMemcpyHostToDevice));
  LAUNCH_TRY(launch_update_rconst(S.rates.dev(), S.s_env.p, S.s_rct.p, ncell, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(rconst, S.s_rct.p, nc * nr * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ---- the hand-over halves of x_drive (pack.hip)

int mistra_chem_drive_dims(int mech, int* j2, int* j6, int* nkc, int* nbgs) {
  if (int rc = builtin_only(mech, "hand-over tables")) return rc;
  if (int rc = check_call(mech, 1)) return rc;
  const MechState& S = g_devs[0].mech[mech];
  if (int rc = require(S, mech, kNeedPackTable)) return rc;
  if (j2) *j2 = S.pack.tab.j2;
  if (j6) *j6 = S.pack.tab.j6;
  if (nkc) *nkc = S.pack.tab.nkc;
  if (nbgs) *nbgs = kBudSlots;
  return 0;
}

int mistra_chem_set_species_maps(int mech, int j1, const int32_t* gas_m2k, const int32_t* gas_k2m, int j5, const int32_t* rad_m2k,
                                 const int32_t* rad_k2m) {
  if (int rc = builtin_only(mech, "hand-over tables")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, 1)) return rc;
  if (j1 < 0 || j5 < 0 || (j1 > 0 && (!gas_m2k || !gas_k2m)) || (j5 > 0 && (!rad_m2k || !rad_k2m))) return fail("bad species maps");
  const int nvar = kMech[mech].dims.nvar;
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, kNeedPackTable, true, &t)) return rc;      // (the maps are the same on every slot)
  // what the kernels rely on: every map entry names a VARIABLE species, and no species is written twice by the pack (neither by two
  // map entries nor by a map entry and one of the driver's explicit liquid-phase assignments): the reference assigns in sequence
  // and the later one wins, the kernel assigns in parallel
  std::vector<char> seen((size_t)nvar, 0);
  for (int j = 0; j < j1 + j5; j++) {
    const int32_t* m = j < j1 ? gas_m2k + 2 * j : rad_m2k + 2 * (j - j1);
    const int c = m[0], src = m[1], lim = j < j1 ? j1 : j5;
    if (c < 1 || c > nvar || src < 1 || src > lim) return fail("species map entry out of range");
    if (seen[(size_t)c - 1]++) return fail("a species is mapped twice");
    const int back = j < j1 ? gas_k2m[src - 1] : rad_k2m[src - 1];
    if (back != c) return fail("gas_m2k / gas_k2m (rad_m2k / rad_k2m) are not inverse to each other");
  }
  for (auto& D : g_devs) {
    PackBufs& K = D.mech[mech].pack;
    for (int i = 0; i < K.tab.n_pack(); i++) {
      const int c0 = K.tab.pack[(size_t)4 * i];
      if (c0 < nvar && seen[(size_t)c0]) return fail("a species of the gas maps is also packed from sl1 / sion1");
    }
    HIP_TRY(hipSetDevice(D.id));
    if (int rc = K.set_maps(j1, gas_m2k, gas_k2m, j5, rad_m2k, rad_k2m)) return rc;
  }
  (void)hipSetDevice(g_devs[0].id);
  return 0;
}

int mistra_chem_pack_device(int mech, int ncell, const double* d_s1, const double* d_s3, double* d_sl1, double* d_sion1, const double* d_scal,
                            double* d_var, double* d_fix, void* hip_stream) {
  if (int rc = builtin_only(mech, "hand-over tables")) return rc;
  if (ncell == 0) return 0;
  if (!d_s1 || !d_s3 || !d_sl1 || !d_sion1 || !d_scal || !d_var || !d_fix) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", kNeedPack, &t)) return rc;
  LAUNCH_TRY(launch_pack(pack_dev(*t.S), ncell, d_s1, d_s3, d_sl1, d_sion1, d_scal, d_var, d_fix, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_unpack_device(int mech, int ncell, const double* d_var, double* d_s1, double* d_s3, double* d_sl1, double* d_sion1, void* hip_stream) {
  if (int rc = builtin_only(mech, "hand-over tables")) return rc;
  if (ncell == 0) return 0;
  if (!d_var || !d_s1 || !d_s3 || !d_sl1 || !d_sion1) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", kNeedPack, &t)) return rc;
  LAUNCH_TRY(launch_unpack(pack_dev(*t.S), ncell, d_var, d_s1, d_s3, d_sl1, d_sion1, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_budgets_device(int mech, int ncell, const double* d_var, const double* d_fix, const double* d_rconst, double dt, double* d_bg,
                               double* d_bgs, void* hip_stream) {
  if (int rc = builtin_only(mech, "hand-over tables")) return rc;
  if (ncell == 0) return 0;
  if (!d_var || !d_fix || !d_rconst) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", kNeedPack, &t)) return rc;
  LAUNCH_TRY(launch_budgets(pack_dev(*t.S), ncell, d_var, d_fix, d_rconst, dt, d_bg, d_bgs, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_rates_env_from_c_device(int mech, int ncell, const double* d_var, const double* d_fix, double* d_env, void* hip_stream) {
  if (int rc = builtin_only(mech, "hand-over tables")) return rc;
  if (ncell == 0) return 0;
  if (!d_var || !d_fix || !d_env) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", kNeedPack | kNeedRates, &t)) return rc;
  LAUNCH_TRY(launch_env_from_c(pack_dev(*t.S), ncell, t.S->rates.nenv, d_var, d_fix, d_env, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_drive_device(int mech, int ncell, double* d_s1, double* d_s3, double* d_sl1, double* d_sion1, const double* d_scal, double* d_env,
                             double* d_var, double* d_fix, double tin, double dt, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                             double* d_bg, double* d_bgs, void* hip_stream) {
  if (int rc = builtin_only(mech, "batched driver")) return rc;
  if (ncell == 0) return 0;
  if (!d_s1 || !d_s3 || !d_sl1 || !d_sion1 || !d_scal || !d_env || !d_var || !d_fix || !d_ierr || !d_stats) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", kNeedPack | kNeedRates, &t)) return rc;
  MechState& S = *t.S;
  HIP_TRY(S.d_rct.reserve((size_t)ncell * (size_t)S.tab.nreact));      // (grow-only: the first call of a size allocates, i.e. synchronises)
  const ColumnDev c{d_s1, d_s3, d_sl1, d_sion1, d_scal, d_env, d_var, d_fix, S.d_rct.p, d_ierr, d_stats, d_texit_hexit, d_bg, d_bgs, nullptr, nullptr, nullptr};
  return column_step(*t.D, mech, ncell, c, tin, dt, static_cast<hipStream_t>(hip_stream));
}

// x_drive for a batch of layers from the model's own arrays in HOST memory (include/mistra_chem.h).  The layers' slabs are gathered into the
// mechanism's pinned drive arena, go up in one copy, the column step runs on the arena's stream, everything the model gets back comes down
// in two copies (in/out and out-only: the in-only part between them stays up) and mistra_chem_drive_end scatters it into the model arrays.
// Primary device only: a column step is 148 layers.
int mistra_chem_drive_begin(int mech, int nlayer, const int32_t* layer, int n, double* s1, double* s3, double* sl1, double* sion1, const double* scal,
                            const double* env, double tin, double dt, int32_t* ierr, int32_t* stats, double* t_h, double* bg, int nrxn,
                            const int32_t* bg_level, double* bgs, double* c_packed) {
  if (int rc = builtin_only(mech, "batched driver")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, nlayer)) return rc;
  if (nlayer == 0) return 0;
  if (!layer || !s1 || !s3 || !sl1 || !sion1 || !scal || !env) return fail("null host pointer");
  if (bg && (!bg_level || nrxn < kMech[mech].dims.nreact)) return fail("bg needs bg_level and nrxn >= NREACT");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, kNeedPack | kNeedRates, true, &t)) return rc;
  MechState& S = *t.S;
  for (int i = 0; i < nlayer; i++) {
    if (layer[i] < 1 || layer[i] > n) return fail("layer index out of range");
    if (bg && (bg_level[i] < 0)) return fail("bg_level out of range");
  }
  const bool reuse = g_step_reuse[mech];
  const DriveLayout L = drive_layout(S, mech, (size_t)nlayer, bg != nullptr, bgs != nullptr, c_packed != nullptr, reuse);
  const size_t nl = L.nl, nb = 2 * (size_t)kBudSlots;
  HIP_TRY(S.drive.ensure(L.end));
  HIP_TRY(S.s_sing.reserve(nl * 8));
  const Staging& A = S.drive;
  if (reuse && S.step_n != n) {      // first step under reuse, a column of another height, or forgotten: nothing is remembered (the stream is idle: no step is open)
    HIP_TRY(S.step_mem.reserve((size_t)n));
    HIP_TRY(hipMemsetAsync(S.step_mem.p, 0, (size_t)n * sizeof(double), A.st));
    S.step_n = n;
  }
  // ---- gather the layers (the model arrays hold layer k at stride j1 / j5 / j2*nkc / j6*nkc; bg at stride 2*nrxn per level; bgs at 2*122 per layer)
  for (size_t i = 0; i < nl; i++) {
    const size_t k = (size_t)layer[i] - 1;
    std::memcpy(A.h(L.s1) + i * L.j1, s1 + k * L.j1, L.j1 * sizeof(double));
    std::memcpy(A.h(L.s3) + i * L.j5, s3 + k * L.j5, L.j5 * sizeof(double));
    std::memcpy(A.h(L.sl1) + i * L.nsl, sl1 + k * L.nsl, L.nsl * sizeof(double));
    std::memcpy(A.h(L.si) + i * L.nsi, sion1 + k * L.nsi, L.nsi * sizeof(double));
    if (bg) {
      if (bg_level[i] > 0) std::memcpy(A.h(L.bg) + i * 2 * L.nr, bg + ((size_t)bg_level[i] - 1) * 2 * (size_t)nrxn, 2 * L.nr * sizeof(double));
      else std::memset(A.h(L.bg) + i * 2 * L.nr, 0, 2 * L.nr * sizeof(double));
    }
    if (bgs) std::memcpy(A.h(L.bgs) + i * nb, bgs + k * nb, nb * sizeof(double));
  }
  std::memcpy(A.h(L.scal), scal, nl * 6 * sizeof(double));
  std::memcpy(A.h(L.env), env, nl * L.ne * sizeof(double));
  if (reuse) std::memcpy(A.h<int32_t>(L.lyr), layer, nl * sizeof(int32_t));      // (every entry checked above: 1..n)
  HIP_TRY(hipMemcpyAsync(A.dev, A.host, L.in_end, hipMemcpyHostToDevice, A.st));
  // KPP's dummy product species are not set by the drivers; the reference carries over what the previous LAYER left in COMMON /GDATA_x/
  // (INTEGRATION.md §4): a batch gives every layer zeros
  HIP_TRY(hipMemsetAsync(A.d(L.var), 0, nl * L.nv * sizeof(double), A.st));
  const ColumnDev c{A.d(L.s1), A.d(L.s3), A.d(L.sl1), A.d(L.si), A.d(L.scal), A.d(L.env), A.d(L.var), A.d(L.fix), A.d(L.rct),
                    A.d<int32_t>(L.ierr), A.d<int32_t>(L.stats), A.d(L.th), bg ? A.d(L.bg) : nullptr, bgs ? A.d(L.bgs) : nullptr,
                    c_packed ? A.d(L.cp) : nullptr, A.d(L.hl), S.s_sing.p,
                    reuse ? A.d<int32_t>(L.lyr) : nullptr, reuse ? A.d(L.hs) : nullptr, reuse ? S.step_mem.p : nullptr, reuse ? n : 0};
  S.sing_start = 0; S.sing_count = nl; S.sing_one = false;
  if (int rc = column_step(*t.D, mech, nlayer, c, tin, dt, A.st)) return rc;
  HIP_TRY(hipMemcpyAsync(A.host, A.dev, L.io_end, hipMemcpyDeviceToHost, A.st));
  HIP_TRY(hipMemcpyAsync(A.host + L.in_end, A.dev + L.in_end, L.out_end - L.in_end, hipMemcpyDeviceToHost, A.st));
  MechState::PendingDrive& Q = S.pend;
  Q.lay = L;
  Q.layer.assign(layer, layer + nl);
  if (bg) Q.level.assign(bg_level, bg_level + nl); else Q.level.clear();
  Q.s1 = s1; Q.s3 = s3; Q.sl1 = sl1; Q.sion1 = sion1; Q.bg = bg; Q.bgs = bgs; Q.t_h = t_h; Q.c_packed = c_packed; Q.ierr = ierr; Q.stats = stats; Q.nrxn = nrxn;
  Q.active = true;
  return 0;
}

int mistra_chem_drive_end(int mech) {
  if (int rc = builtin_only(mech, "batched driver")) return rc;
  if (int rc = check_call(mech, 1)) return rc;
  std::lock_guard<std::mutex> lock(g_mu);
  DeviceState& D = g_devs[0];
  MechState& S = D.mech[mech];
  MechState::PendingDrive& Q = S.pend;
  if (!Q.active) return fail("mistra_chem_drive_end: nothing issued for this mechanism");
  Q.active = false;
  HIP_TRY(hipSetDevice(D.id));
  HIP_TRY(hipStreamSynchronize(S.drive.st));
  const DriveLayout& L = Q.lay;
  const Staging& A = S.drive;
  const size_t nl = L.nl, nb = 2 * (size_t)kBudSlots;
  // ---- scatter
  const int32_t *h_ierr = A.h<int32_t>(L.ierr), *h_stats = A.h<int32_t>(L.stats);
  for (size_t i = 0; i < nl; i++) {
    const size_t k = (size_t)Q.layer[i] - 1;
    std::memcpy(Q.s1 + k * L.j1, A.h(L.s1) + i * L.j1, L.j1 * sizeof(double));
    std::memcpy(Q.s3 + k * L.j5, A.h(L.s3) + i * L.j5, L.j5 * sizeof(double));
    std::memcpy(Q.sl1 + k * L.nsl, A.h(L.sl1) + i * L.nsl, L.nsl * sizeof(double));
    std::memcpy(Q.sion1 + k * L.nsi, A.h(L.si) + i * L.nsi, L.nsi * sizeof(double));
    if (Q.bg && Q.level[i] > 0) std::memcpy(Q.bg + ((size_t)Q.level[i] - 1) * 2 * (size_t)Q.nrxn, A.h(L.bg) + i * 2 * L.nr, 2 * L.nr * sizeof(double));
    if (Q.bgs) std::memcpy(Q.bgs + k * nb, A.h(L.bgs) + i * nb, nb * sizeof(double));
    if (Q.ierr) Q.ierr[i] = h_ierr[i];
    if (Q.stats) std::memcpy(Q.stats + i * 8, h_stats + i * 8, 8 * sizeof(int32_t));
    if (Q.t_h) { Q.t_h[3 * i] = A.h(L.th)[2 * i]; Q.t_h[3 * i + 1] = A.h(L.th)[2 * i + 1]; Q.t_h[3 * i + 2] = A.h(L.hl)[i]; }
  }
  if (Q.c_packed) std::memcpy(Q.c_packed, A.h(L.cp), nl * (L.nv + L.nf) * sizeof(double));
  return 0;
}

int mistra_chem_drive(int mech, int nlayer, const int32_t* layer, int n, double* s1, double* s3, double* sl1, double* sion1, const double* scal,
                      const double* env, double tin, double dt, int32_t* ierr, int32_t* stats, double* t_h, double* bg, int nrxn,
                      const int32_t* bg_level, double* bgs, double* c_packed) {
  if (int rc = mistra_chem_drive_begin(mech, nlayer, layer, n, s1, s3, sl1, sion1, scal, env, tin, dt, ierr, stats, t_h, bg, nrxn, bg_level, bgs, c_packed)) return rc;
  if (nlayer == 0) return 0;
  return mistra_chem_drive_end(mech);
}

// ---- liq_parm: the device-pointer entries, then the host-buffer forms (DevBlock)

int mistra_chem_fast_k_mt_device(int mech, int nlayer, const double* d_ff, const double* d_rq, const int32_t* kw, int nkw, int ka, int ifeed,
                                 int nkc_l, const double* d_cw, const double* d_cm, const double* d_freep, const double* d_alpha,
                                 const double* d_vmean, double* d_xkmt, const double* d_t, const double* d_p, double* d_vt, void* hip_stream) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (nlayer == 0) return check_call(mech, 0);
  if (!d_ff || !d_rq || !kw || !d_cw || !d_cm || !d_freep || !d_alpha || !d_vmean || !d_xkmt) return fail("null pointer");
  if (d_vt && (!d_t || !d_p)) return fail("the sedimentation velocity needs the layers' temperature and pressure (d_t, d_p)");
  Slot t;
  if (int rc = on_device(mech, nlayer, d_xkmt, "d_xkmt", kNeedKmt, &t)) return rc;
  KmtDev K;
  if (int rc = kmt_args(*t.S, kw, nkw, ka, ifeed, nkc_l, &K)) return rc;
  LAUNCH_TRY(launch_fast_k_mt(K, nlayer, d_ff, d_rq, d_cw, d_cm, d_freep, d_alpha, d_vmean, d_xkmt, d_t, d_p, d_vt, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_henry_device(int mech, int nlayer, const double* d_tt, double* d_henry, void* hip_stream) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (nlayer == 0) return check_call(mech, 0);
  if (!d_tt || !d_henry) return fail("null pointer");
  Slot t;
  if (int rc = on_device(mech, nlayer, d_henry, "d_henry", kNeedLiq, &t)) return rc;
  LAUNCH_TRY(launch_henry(t.S->liq.dev(), nlayer, d_tt, d_henry, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_st_coeff_device(int mech, int nlayer, int lp_joyce14bc, int lp_buxmann15alph, const double* d_env, double* d_alpha, void* hip_stream) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (nlayer == 0) return check_call(mech, 0);
  if (!d_env || !d_alpha) return fail("null pointer");
  Slot t;
  if (int rc = on_device(mech, nlayer, d_alpha, "d_alpha", kNeedStc, &t)) return rc;
  const int v = (lp_joyce14bc ? 1 : 0) + (lp_buxmann15alph ? 2 : 0);
  LAUNCH_TRY(launch_update_rconst(t.S->stc.dev(v), d_env, d_alpha, nlayer, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_v_mean_device(int mech, int nlayer, const double* d_tt, double* d_vmean, void* hip_stream) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (nlayer == 0) return check_call(mech, 0);
  if (!d_tt || !d_vmean) return fail("null pointer");
  Slot t;
  if (int rc = on_device(mech, nlayer, d_vmean, "d_vmean", kNeedVmean, &t)) return rc;
  const VmeanBufs& V = t.S->vmean;
  LAUNCH_TRY(launch_v_mean(V.mass.p, V.tab.nspec, V.tab.coef, nlayer, d_tt, d_vmean, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_equil_co_device(int mech, int nlayer, int nkc, int j6, const double* d_tt, const double* d_conv2, const double* d_xgamma,
                                double* d_xkef, double* d_xkeb, void* hip_stream) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (nlayer == 0) return check_call(mech, 0);
  if (!d_tt || !d_conv2 || !d_xgamma || !d_xkef || !d_xkeb) return fail("null pointer");
  Slot t;
  if (int rc = on_device(mech, nlayer, d_xkef, "d_xkef", kNeedLiq, &t)) return rc;
  if (int rc = equil_co_check(*t.S, nkc, j6)) return rc;
  LAUNCH_TRY(launch_equil_co(t.S->liq.dev(), nlayer, nkc, j6, d_tt, d_conv2, d_xgamma, d_xkef, d_xkeb, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_pin_host(void* p, size_t bytes) {
  if (int rc = lazy_init()) return rc;
  if (!p || !bytes) return fail("mistra_chem_pin_host: null range");
  std::lock_guard<std::mutex> lock(g_mu);
  if (g_pinned.contains(p, bytes)) return 0;
  const char* c = static_cast<const char*>(p);
  for (const auto& r : g_pinned.r)
    if (c < r.first + r.second && r.first < c + bytes) return fail("mistra_chem_pin_host: the range overlaps one registered before");
  HIP_TRY(hipSetDevice(g_devs[0].id));
  HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
  g_pinned.r.emplace_back(c, bytes);
  return 0;
}

int mistra_chem_unpin_host(void* p) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (size_t i = 0; i < g_pinned.r.size(); i++)
    if (g_pinned.r[i].first == static_cast<const char*>(p)) {
      HIP_TRY(hipHostUnregister(p));
      g_pinned.r.erase(g_pinned.r.begin() + (long)i);
      return 0;
    }
  return fail("mistra_chem_unpin_host: not a registered range");
}

int mistra_chem_fast_k_mt(int mech, int nlayer, const double* ff, const double* rq, const int32_t* kw, int nkw, int ka, int ifeed, int nkc_l,
                          const double* cw, const double* cm, const double* freep, const double* alpha, const double* vmean, double* xkmt,
                          const double* t, const double* p, double* vt) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, nlayer)) return rc;
  if (nlayer == 0) return 0;
  if (!ff || !rq || !kw || !cw || !cm || !freep || !alpha || !vmean || !xkmt) return fail("null pointer");
  if (vt && (!t || !p)) return fail("the sedimentation velocity needs the layers' temperature and pressure (t, p)");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot s;
  if (int rc = on_primary(mech, kNeedKmt, false, &s)) return rc;
  KmtDev K;
  if (int rc = kmt_args(*s.S, kw, nkw, ka, ifeed, nkc_l, &K)) return rc;
  const KmtTable& T = s.S->kmt.tab;
  const size_t nl = (size_t)nlayer, grid = (size_t)T.nka * T.nkt, nspec = (size_t)(s.S->tab.nvar + s.S->tab.nfix), nkc = (size_t)T.nkc, d8 = sizeof(double);
  DevBlock B;
  const size_t i_ff = B.add(nl * grid * d8), i_rq = B.add(grid * d8), i_cw = B.add(nl * nkc * d8), i_cm = B.add(nl * nkc * d8), i_fp = B.add(nl * d8),
               i_al = B.add(nl * nspec * d8), i_vm = B.add(nl * nspec * d8), i_xk = B.add(nl * nkc * nspec * d8), i_t = B.add(nl * d8), i_p = B.add(nl * d8),
               i_vt = B.add(nl * nkc * d8);
  HIP_TRY(B.alloc());
  B.up(i_ff, ff); B.up(i_rq, rq); B.up(i_cw, cw); B.up(i_cm, cm); B.up(i_fp, freep); B.up(i_al, alpha); B.up(i_vm, vmean); B.up(i_xk, xkmt);
  if (vt) { B.up(i_t, t); B.up(i_p, p); B.up(i_vt, vt); }
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_fast_k_mt(K, nlayer, B.dptr(i_ff), B.dptr(i_rq), B.dptr(i_cw), B.dptr(i_cm), B.dptr(i_fp), B.dptr(i_al), B.dptr(i_vm), B.dptr(i_xk),
                              vt ? B.dptr(i_t) : nullptr, vt ? B.dptr(i_p) : nullptr, vt ? B.dptr(i_vt) : nullptr, B.stream()));
  B.down(i_xk, xkmt);
  if (vt) B.down(i_vt, vt);
  HIP_TRY(B.finish());
  return 0;
}

int mistra_chem_henry(int mech, int nlayer, const double* tt, double* henry) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, nlayer)) return rc;
  if (nlayer == 0) return 0;
  if (!tt || !henry) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot s;
  if (int rc = on_primary(mech, kNeedLiq, false, &s)) return rc;
  const size_t nl = (size_t)nlayer, nspec = (size_t)s.S->liq.tab.nspec;
  DevBlock B;
  const size_t i_t = B.add(nl * sizeof(double)), i_h = B.add(nl * nspec * sizeof(double));
  HIP_TRY(B.alloc());
  B.up(i_t, tt);
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_henry(s.S->liq.dev(), nlayer, B.dptr(i_t), B.dptr(i_h), B.stream()));
  B.down(i_h, henry);
  HIP_TRY(B.finish());
  return 0;
}

int mistra_chem_dry_rates(int gas, int nlayer, const double* tt, const double* freep, const double* rcd, const double* vmean4, double* xkmtd, double* xeq,
                          double* henry4) {
  if (int rc0 = lazy_init()) return rc0;
  if (nlayer == 0) return 0;
  if (nlayer < 0) return fail("nlayer < 0");
  if (!tt || !freep || !rcd || !xkmtd || !xeq || (gas ? !henry4 : !vmean4)) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  HIP_TRY(hipSetDevice(g_devs[0].id));
  const size_t nl = (size_t)nlayer, d8 = sizeof(double);
  DevBlock B;
  const size_t i_t = B.add(nl * d8), i_f = B.add(nl * d8), i_r = B.add(nl * 2 * d8), i_v = B.add(nl * 4 * d8), i_x = B.add(nl * 8 * d8), i_q = B.add(nl * d8),
               i_h = B.add(nl * 4 * d8);
  HIP_TRY(B.alloc());
  B.up(i_t, tt); B.up(i_f, freep); B.up(i_r, rcd);
  if (gas) B.up(i_h, henry4); else B.up(i_v, vmean4);
  const DryRatesArgs A{nlayer, gas ? 1 : 0, B.dptr(i_t), B.dptr(i_f), B.dptr(i_r), B.dptr(i_v), B.dptr(i_x), B.dptr(i_q), B.dptr(i_h)};
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_dry_rates(A, B.stream()));
  B.down(i_x, xkmtd); B.down(i_q, xeq);
  if (gas) B.down(i_h, henry4);
  HIP_TRY(B.finish());
  return 0;
}

int mistra_chem_cw_rc(int nlayer, int nkt, int nka, int dry, const double* ff, const double* rq, const double* e, const int32_t* kw, int ka, int ifeed,
                      const double* feu, const int32_t* cloud, const double* crys4, double* rc, double* cw, double* cm, double* conv2, int32_t* below) {
  if (int rc0 = lazy_init()) return rc0;
  if (nlayer == 0) return 0;
  if (nlayer < 0 || nkt < 1 || nka < 1 || nkt > 2048 || nka > 4096 || ka < 0 || ka > nka) return fail("cw_rc: bad dimensions (nkt <= 2048, nka <= 4096)");
  if (!ff || !rq || !kw || !rc || !cw || (!dry && (!e || !feu || !cloud || !crys4 || !cm || !conv2))) return fail("null pointer");
  for (int i = 0; i < nka; i++)
    if (kw[i] < 0 || kw[i] > nkt) return fail("kw out of range");      // the kernel's loop limits: checked here, on the host
  std::lock_guard<std::mutex> lock(g_mu);
  HIP_TRY(hipSetDevice(g_devs[0].id));
  const size_t nl = (size_t)nlayer, grid = (size_t)nka * nkt, nb = dry ? 2 : 4, d8 = sizeof(double);
  DevBlock B;
  const size_t i_ff = B.add(nl * grid * d8), i_rq = B.add(grid * d8), i_e = B.add((size_t)nkt * d8), i_kw = B.add((size_t)nka * 4), i_feu = B.add(nl * d8),
               i_cl = B.add(nl * 4 * 4), i_rc = B.add(nl * nb * d8), i_cw = B.add(nl * nb * d8), i_cm = B.add(nl * nb * d8), i_cv = B.add(nl * nb * d8),
               i_bl = B.add(nl * 4);
  HIP_TRY(B.alloc());
  B.up(i_ff, ff); B.up(i_rq, rq); B.up(i_kw, kw);
  if (!dry) { B.up(i_e, e); B.up(i_feu, feu); B.up(i_cl, cloud); }
  CwRcArgs A{};
  A.nlayer = nlayer; A.nkt = nkt; A.nka = nka; A.ka = ka; A.ial = ifeed == 2 ? 2 : 1; A.dry = dry ? 1 : 0;
  if (!dry) { A.xcryssulf = crys4[0]; A.xcrysss = crys4[1]; A.xdelisulf = crys4[2]; A.xdeliss = crys4[3]; }
  A.kw = reinterpret_cast<const int32_t*>(B.dptr(i_kw)); A.ff = B.dptr(i_ff); A.rq = B.dptr(i_rq); A.e = B.dptr(i_e); A.feu = B.dptr(i_feu);
  A.cloud = reinterpret_cast<const int32_t*>(B.dptr(i_cl)); A.rc = B.dptr(i_rc); A.cw = B.dptr(i_cw); A.cm = B.dptr(i_cm); A.conv2 = B.dptr(i_cv);
  A.below = reinterpret_cast<int32_t*>(B.dptr(i_bl));
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_cw_rc(A, B.stream()));
  B.down(i_rc, rc); B.down(i_cw, cw);
  if (!dry) { B.down(i_cm, cm); B.down(i_cv, conv2); if (below) B.down(i_bl, below); }
  HIP_TRY(B.finish());
  return 0;
}

int mistra_chem_st_coeff(int mech, int nlayer, int lp_joyce14bc, int lp_buxmann15alph, const double* env, double* alpha) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, nlayer)) return rc;
  if (nlayer == 0) return 0;
  if (!env || !alpha) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot s;
  if (int rc = on_primary(mech, kNeedStc, false, &s)) return rc;
  const int v = (lp_joyce14bc ? 1 : 0) + (lp_buxmann15alph ? 2 : 0);
  const size_t nl = (size_t)nlayer, nspec = (size_t)s.S->stc.tab.v[0].nreact, nenv = (size_t)s.S->stc.tab.v[0].nenv;
  DevBlock B;
  const size_t i_e = B.add(nl * nenv * sizeof(double)), i_a = B.add(nl * nspec * sizeof(double));
  HIP_TRY(B.alloc());
  B.up(i_e, env);
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_update_rconst(s.S->stc.dev(v), B.dptr(i_e), B.dptr(i_a), nlayer, B.stream()));
  B.down(i_a, alpha);
  HIP_TRY(B.finish());
  return 0;
}

int mistra_chem_v_mean(int mech, int nlayer, const double* tt, double* vmean) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, nlayer)) return rc;
  if (nlayer == 0) return 0;
  if (!tt || !vmean) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot s;
  if (int rc = on_primary(mech, kNeedVmean, false, &s)) return rc;
  const VmeanBufs& V = s.S->vmean;
  const size_t nl = (size_t)nlayer, nspec = (size_t)V.tab.nspec;
  DevBlock B;
  const size_t i_t = B.add(nl * sizeof(double)), i_v = B.add(nl * nspec * sizeof(double));
  HIP_TRY(B.alloc());
  B.up(i_t, tt);
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_v_mean(V.mass.p, V.tab.nspec, V.tab.coef, nlayer, B.dptr(i_t), B.dptr(i_v), B.stream()));
  B.down(i_v, vmean);
  HIP_TRY(B.finish());
  return 0;
}

int mistra_chem_equil_co(int mech, int nlayer, int nkc, int j6, const double* tt, const double* conv2, const double* xgamma, double* xkef, double* xkeb) {
  if (int rc = builtin_only(mech, "liquid-phase routines")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, nlayer)) return rc;
  if (nlayer == 0) return 0;
  if (!tt || !conv2 || !xgamma || !xkef || !xkeb || nkc < 1 || j6 < 1) return fail("null pointer or bad dimensions");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot s;
  if (int rc = on_primary(mech, kNeedLiq, false, &s)) return rc;
  if (int rc = equil_co_check(*s.S, nkc, j6)) return rc;
  const size_t nl = (size_t)nlayer, nspec = (size_t)s.S->liq.tab.nspec, d8 = sizeof(double);
  DevBlock B;
  const size_t i_t = B.add(nl * d8), i_c = B.add(nl * nkc * d8), i_g = B.add(nl * nkc * j6 * d8), i_f = B.add(nl * nkc * nspec * d8), i_b = B.add(nl * nkc * nspec * d8);
  HIP_TRY(B.alloc());
  B.up(i_t, tt); B.up(i_c, conv2); B.up(i_g, xgamma); B.up(i_f, xkef); B.up(i_b, xkeb);
  HIP_TRY(B.send());
  LAUNCH_TRY(launch_equil_co(s.S->liq.dev(), nlayer, nkc, j6, B.dptr(i_t), B.dptr(i_c), B.dptr(i_g), B.dptr(i_f), B.dptr(i_b), B.stream()));
  B.down(i_f, xkef); B.down(i_b, xkeb);
  HIP_TRY(B.finish());
  return 0;
}

// ---- OPT-IN step reuse of the batched driver

int mistra_chem_set_step_reuse(int mech, int on) {
  if (int rc = builtin_only(mech, "step reuse")) return rc;
  std::lock_guard<std::mutex> lock(g_mu);
  read_step_env();
  if (g_inited && !g_devs.empty() && g_devs[0].mech[mech].pend.active) return step_is_open(mech);
  const bool want = on != 0;
  if (want == g_step_reuse[mech]) return 0;
  g_step_reuse[mech] = want;
  for (auto& D : g_devs) D.mech[mech].step_n = 0;      // switched: nothing is remembered
  return 0;
}

int mistra_chem_get_step_reuse(int mech) {
  if (!known_mech(mech) || kMech[mech].user) return 0;
  std::lock_guard<std::mutex> lock(g_mu);
  read_step_env();
  return g_step_reuse[mech] ? 1 : 0;
}

int mistra_chem_get_step_memory(int mech, int n, double* h) {
  if (int rc = builtin_only(mech, "step reuse")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, n)) return rc;
  if (n == 0) return 0;
  if (!h) return fail("null host pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;      // (an open step is still rewriting it)
  const MechState& S = *t.S;
  if (S.step_n == 0) {
    std::memset(h, 0, (size_t)n * sizeof(double));
    return 0;
  }
  if (S.step_n != n) return fail("the step memory of the " + std::string(kMech[mech].name) + " mechanism holds " + std::to_string(S.step_n) + " layers, not " + std::to_string(n));
  HIP_TRY(hipMemcpy(h, S.step_mem.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int mistra_chem_set_step_memory(int mech, int n, const double* h) {
  if (int rc = builtin_only(mech, "step reuse")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, n)) return rc;
  if (n == 0) return fail("mistra_chem_set_step_memory: n must be the model's layer count");
  if (!h) return fail("null host pointer");
  for (int i = 0; i < n; i++)
    if (!(h[i] >= 0.0) || std::isinf(h[i])) return fail("mistra_chem_set_step_memory: step sizes are finite and >= 0 (0 = none)");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;
  MechState& S = *t.S;
  S.step_n = 0;
  HIP_TRY(S.step_mem.reserve((size_t)n));
  HIP_TRY(hipMemcpy(S.step_mem.p, h, (size_t)n * sizeof(double), hipMemcpyHostToDevice));      // (no step is open: the drive stream is idle)
  S.step_n = n;
  return 0;
}

int mistra_chem_debug_set_max_steps(int max_steps) {
  std::lock_guard<std::mutex> lock(g_mu);
  g_max_steps = max_steps > 0 ? max_steps : 100000;
  return 0;
}

int mistra_chem_check_options(int mech, const int32_t* ipar, const double* rpar, const double* atol, const double* rtol, double interval,
                              int32_t* ierr, double* resolved_r, int32_t* resolved_i) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (!ipar || !rpar || !atol || !rtol || !ierr) return fail("null pointer");
  *ierr = 0;
  RosResolved r;
  const int code = resolve_options(mech, ipar, rpar, atol, rtol, &r);
  if (code == 1)
    if (int rc = method_built(mech, ipar)) return rc;      // (*ierr stays 0: not a code of Rosenbrock_x's)
  *ierr = code;
  if (code != 1) return 0;
  const double span = std::fabs(interval);
  if (resolved_r) {
    const double hmax = std::min(r.hmax, span);                             // gas.f:987-989
    const double hstart = rpar[2] == 0.0 ? r.hstart : std::min(r.hstart, span);      // gas.f:997-999
    const double v[7] = {r.hmin, hmax, hstart, r.facmin, r.facmax, r.facrej, r.facsafe};
    std::memcpy(resolved_r, v, sizeof v);
  }
  if (resolved_i) { resolved_i[0] = r.max_steps; resolved_i[1] = r.autonomous; resolved_i[2] = r.vector; }
  return 0;
}

int mistra_chem_set_options(int mech, const int32_t* ipar, const double* rpar, const double* atol, const double* rtol, int32_t* ierr) {
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, 0, true)) return rc;
  if (ierr) *ierr = 0;
  if (ipar && (!rpar || !atol || !rtol)) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;      // (a column step in flight reads the block that would be freed here)
  RosOptions next;
  if (ipar) {
    const int code = resolve_options(mech, ipar, rpar, atol, rtol, &next.r);
    if (code != 1) {
      if (ierr) *ierr = code;
      return fail(options_refusal(mech, code));
    }
    if (int rc = method_built(mech, ipar)) return rc;
    if (ierr) *ierr = 1;
    next.set = true;
    std::memcpy(next.ipar, ipar, sizeof next.ipar);
    std::memcpy(next.rpar, rpar, sizeof next.rpar);
    next.block = options_block(mech, next.r, atol, rtol);
  }
  int rc = 0;
  for (auto& D : g_devs) {      // every slot: the device-buffer entries run where their buffers live
    MechState& S = D.mech[mech];
    if (hipSetDevice(D.id) != hipSuccess) { rc = fail("hipSetDevice failed"); break; }
    if (hipDeviceSynchronize() != hipSuccess) { rc = fail("hipDeviceSynchronize failed"); break; }      // (launches of the device-buffer entries that still read the old block)
    S.opt.release();
    S.opt_max_steps = 0;
    S.step_n = 0;      // other tolerances or step bounds: the step sizes remembered under the old ones are forgotten
    if (next.set) {
      if (hipError_t e = S.opt.upload(next.block)) { rc = fail(std::string("uploading the options: ") + hipGetErrorString(e)); break; }
      S.opt_max_steps = next.ipar[2];
    }
  }
  (void)hipSetDevice(g_devs[0].id);
  if (rc) {      // a failed upload leaves no slot with options the others do not have
    for (auto& D : g_devs) { D.mech[mech].opt.release(); D.mech[mech].opt_max_steps = 0; }
    g_opts[mech] = RosOptions{};
    return rc;
  }
  g_opts[mech] = next;
  return 0;
}

int mistra_chem_get_options(int mech, int32_t* is_set, int32_t* ipar, double* rpar, double* atol, double* rtol) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (!is_set) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  const RosOptions& o = g_opts[mech];
  *is_set = o.set ? 1 : 0;
  if (!o.set) return 0;
  const size_t nv = (size_t)kMech[mech].dims.nvar;
  if (ipar) std::memcpy(ipar, o.ipar, sizeof o.ipar);
  if (rpar) std::memcpy(rpar, o.rpar, sizeof o.rpar);
  if (atol) std::memcpy(atol, o.block.data() + kOptTol, nv * sizeof(double));
  if (rtol) std::memcpy(rtol, o.block.data() + kOptTol + nv, nv * sizeof(double));
  return 0;
}

// ---- OPT-IN integrator policy
int mistra_chem_check_policy(int mech, int method, double atol_factor, double atol_floor) {
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (int rc = read_policy_env()) return rc;      // (a value in the environment that cannot be read is reported by every policy entry)
  }
  return check_policy(mech, method, atol_factor, atol_floor);
}

// next.set = false: clear.  Every slot, walked and synchronised as mistra_chem_set_options walks them
static int install_policy(int mech, const Policy& next) {
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, 0, true)) return rc;
  std::lock_guard<std::mutex> lock(g_mu);
  if (int rc = read_policy_env()) return rc;
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;      // (a column step in flight reads the block that would be freed here)
  const std::vector<double> block = next.set ? base_options_block(mech) : std::vector<double>();
  int rc = 0;
  for (auto& D : g_devs) {
    MechState& S = D.mech[mech];
    if (hipSetDevice(D.id) != hipSuccess) { rc = fail("hipSetDevice failed"); break; }
    if (hipDeviceSynchronize() != hipSuccess) { rc = fail("hipDeviceSynchronize failed"); break; }      // (launches of the device-buffer entries that still read the old block)
    S.pol_opt.release();
    S.pol_method = 0; S.pol_factor = S.pol_floor = 0.0;
    S.step_n = 0;      // another method or AbsTol: the step sizes remembered under the old ones are forgotten
    if (next.set) {
      if (hipError_t e = S.pol_opt.upload(block)) { rc = fail(std::string("uploading the policy's options block: ") + hipGetErrorString(e)); break; }
      S.pol_method = next.method; S.pol_factor = next.factor; S.pol_floor = next.floor;
    }
  }
  (void)hipSetDevice(g_devs[0].id);
  if (rc) {      // a failed upload leaves no slot with a policy the others do not have
    for (auto& D : g_devs) { MechState& S = D.mech[mech]; S.pol_opt.release(); S.pol_method = 0; S.pol_factor = S.pol_floor = 0.0; }
    g_policy[mech] = Policy{};
    return rc;
  }
  g_policy[mech] = next;
  return 0;
}

int mistra_chem_set_policy(int mech, int method, double atol_factor, double atol_floor) {
  if (int rc = check_policy(mech, method, atol_factor, atol_floor)) return rc;      // (before a device is touched)
  Policy next;
  next.set = true; next.method = method; next.factor = atol_factor;
  next.floor = atol_factor != 0.0 ? atol_floor : 0.0;      // (not read without a factor)
  return install_policy(mech, next);
}

int mistra_chem_clear_policy(int mech) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  return install_policy(mech, Policy{});
}

int mistra_chem_get_policy(int mech, int32_t* is_set, int32_t* method, double* atol_factor, double* atol_floor) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (!is_set) return fail("null pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  if (int rc = read_policy_env()) return rc;
  const Policy& p = g_policy[mech];
  *is_set = p.set ? 1 : 0;
  if (!p.set) return 0;
  if (method) *method = p.method;
  if (atol_factor) *atol_factor = p.factor;
  if (atol_floor) *atol_floor = p.floor;
  return 0;
}

int mistra_chem_debug_first_step(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tin,
                                 double tout, double* dump) {
  return mistra_chem_debug_first_step_ex(mech, ncell, var_in, fix, rconst, tin, tout, nullptr, dump, nullptr, nullptr, nullptr);
}

int mistra_chem_debug_first_step_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tin,
                                    double tout, const double* hstart, double* dump, double* var_out, int32_t* ierr, int32_t* stats) {
  if (int rc = check_call(mech, ncell, true)) return rc;
  if (ncell == 0) return 0;
  if (!var_in || !fix || !rconst || !dump) return fail("null host pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;
  MechState& S = *t.S;
  if (S.opt.p) return fail("the first-step dump keeps INTEGRATE_x's values: clear the options (mistra_chem_set_options) first");
  const size_t nv = (size_t)kMech[mech].dims.nvar, nf = (size_t)kMech[mech].dims.nfix, nr = (size_t)kMech[mech].dims.nreact, nc = (size_t)ncell;
  const size_t per = 5 * nv + 2 * (size_t)kMech[mech].dims.lu_nonzero + 2;
  DevBuf<double> d_dump, d_hstart;
  HIP_TRY(S.s_var.reserve(nc * nv));
  HIP_TRY(S.s_fix.reserve(nc * nf));
  HIP_TRY(S.s_rct.reserve(nc * nr));
  HIP_TRY(S.s_ierr.reserve(nc));
  HIP_TRY(S.s_stats.reserve(nc * 8));
  HIP_TRY(d_dump.reserve(nc * per));
  HIP_TRY(hipMemset(d_dump.p, 0, nc * per * sizeof(double)));
  HIP_TRY(hipMemcpy(S.s_var.p, var_in, nc * nv * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.s_fix.p, fix, nc * nf * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.s_rct.p, rconst, nc * nr * sizeof(double), hipMemcpyHostToDevice));
  KernelArgs a = make_args(S, ncell, S.s_var.p, S.s_fix.p, S.s_rct.p, tin, tout, S.s_var.p, S.s_ierr.p, S.s_stats.p, nullptr);
  a.dump = d_dump.p;
  if (hstart) {
    HIP_TRY(d_hstart.reserve(nc));
    HIP_TRY(hipMemcpy(d_hstart.p, hstart, nc * sizeof(double), hipMemcpyHostToDevice));
    a.hstart = d_hstart.p;
  }
  if (int rc = launch(*t.D, mech, a, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(dump, d_dump.p, nc * per * sizeof(double), hipMemcpyDeviceToHost));
  // what the dump instantiation carried to the end of the integration (the same staging buffers the host-buffer entries use)
  if (var_out) HIP_TRY(hipMemcpy(var_out, S.s_var.p, nc * nv * sizeof(double), hipMemcpyDeviceToHost));
  if (ierr) HIP_TRY(hipMemcpy(ierr, S.s_ierr.p, nc * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (stats) HIP_TRY(hipMemcpy(stats, S.s_stats.p, nc * 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
  d_dump.release();
  d_hstart.release();
  return 0;
}

int mistra_chem_integrate(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tin,
                          double tout, double* var_out, int32_t* ierr, int32_t* stats) {
  return mistra_chem_integrate_ex(mech, ncell, var_in, fix, rconst, tin, tout, var_out, ierr, stats, nullptr);
}

// A Fortran caller has no init hook: the first call brings the library up on device MISTRA_CHEM_DEVICE (default 0), or on the
// first MISTRA_CHEM_DEVICES GPUs of the node when that is set.
static int lazy_init() {
  if (g_inited) return 0;
  if (const char* n = std::getenv("MISTRA_CHEM_DEVICES")) return mistra_chem_init_devices(std::atoi(n), nullptr);
  const char* dev = std::getenv("MISTRA_CHEM_DEVICE");
  return mistra_chem_init(dev ? std::atoi(dev) : 0);
}

// the two paths every Rosenbrock_x request takes (below, behind the families' checks): host buffers, device pointers
static int ros_host(const RosRequest& q);
static int ros_device(const RosRequest& q, void* hip_stream);

// the integrate family: the request without options of its own, under the options and the policy in force
static int integrate_host(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, const double* env, double tin,
                          double tout, double* var_out, int32_t* ierr, int32_t* stats, double* t_h, const double* hstart = nullptr) {
  RosRequest q = ros_request(mech, ncell, var_in, fix, rconst, tin, tout, nullptr, nullptr, nullptr, nullptr, var_out, ierr, stats, t_h, hstart);
  q.options = false; q.env = env; q.record_sing = true;
  return ros_host(q);
}

int mistra_chem_integrate_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tin,
                             double tout, double* var_out, int32_t* ierr, int32_t* stats, double* t_h) {
  return integrate_host(mech, ncell, var_in, fix, rconst, nullptr, tin, tout, var_out, ierr, stats, t_h);
}

int mistra_chem_integrate_env_ex(int mech, int ncell, const double* var_in, const double* fix, const double* env, double tin, double tout,
                                 double* var_out, int32_t* ierr, int32_t* stats, double* t_h) {
  if (int rc = builtin_only(mech, "rate table")) return rc;
  return integrate_host(mech, ncell, var_in, fix, nullptr, env, tin, tout, var_out, ierr, stats, t_h);
}

int mistra_chem_integrate_hstart_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, const double* env, double tin,
                                    double tout, double* var_out, int32_t* ierr, int32_t* stats, double* t_h, const double* hstart) {
  if ((rconst != nullptr) == (env != nullptr)) return fail("mistra_chem_integrate_hstart_ex: exactly one of rconst and env");
  return integrate_host(mech, ncell, var_in, fix, rconst, env, tin, tout, var_out, ierr, stats, t_h, hstart);
}

int mistra_chem_method_table(int method, int* S, double* A15, double* C15, double* M6, double* E6, double* gamma6, int32_t* newf6, double* elo) {
  if (method < 0 || method > 5) return fail("Rosenbrock_x has methods 1 .. 5 (Ros2, Ros3, Ros4, Rodas3, Rodas4; 0 selects Ros4)");
  const RosMethodTable t = ros_method_table(method == 0 ? (int)kRos4 : method);      // the tables the kernels are compiled with (ros_methods.hpp)
  const int nlow = t.S * (t.S - 1) / 2;
  if (S) *S = t.S;
  for (int i = 0; i < 15; i++) {
    if (A15) A15[i] = i < nlow ? t.A[i] : 0.0;
    if (C15) C15[i] = i < nlow ? t.C[i] : 0.0;
  }
  for (int i = 0; i < 6; i++) {
    if (M6) M6[i] = i < t.S ? t.M[i] : 0.0;
    if (E6) E6[i] = i < t.S ? t.E[i] : 0.0;
    if (gamma6) gamma6[i] = i < t.S ? t.Gamma[i] : 0.0;
    if (newf6) newf6[i] = i < t.S && t.NewF[i] ? 1 : 0;
  }
  if (elo) *elo = t.ELO;
  return 0;
}

// ---- Rosenbrock_x with the call's own options.  Every entry below, and every family further down, describes its call (ros_request and what the family
//      adds) and takes one of the two paths: ros_host with host buffers — these record the zero-pivot rows —, ros_device with device pointers.
static int single_host(RosRequest q) {
  q.record_sing = true;
  return ros_host(q);
}

int mistra_chem_rosenbrock_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                              const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr,
                              int32_t* stats, double* t_h) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h));
}

int mistra_chem_rosenbrock_trace_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                    const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr,
                                    int32_t* stats, double* t_h, int cap, double* trace_d, int32_t* trace_i, int32_t* ntrace, int32_t* ctrl) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h)
                         .traced(cap, trace_d, trace_i, ntrace, ctrl));
}

int mistra_chem_rosenbrock_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                  double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* d_var_out,
                                  int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart, void* hip_stream) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, atol, rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart),
                    hip_stream);
}

int mistra_chem_rosenbrock_trace_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                        double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                        double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                        void* hip_stream, int cap, double* d_trace_d, int32_t* d_trace_i, int32_t* d_ntrace, int32_t* d_ctrl) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, atol, rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .traced(cap, d_trace_d, d_trace_i, d_ntrace, d_ctrl),
                    hip_stream);
}

// ---- tolerances per cell: the rows in place of the pair
int mistra_chem_rosenbrock_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                    const double* atol, const double* rtol, int ntol, const double* rpar, const int32_t* ipar, double* var_out,
                                    int32_t* ierr, int32_t* stats, double* t_h) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h).cells(ntol));
}

int mistra_chem_rosenbrock_trace_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                          const double* atol, const double* rtol, int ntol, const double* rpar, const int32_t* ipar, double* var_out,
                                          int32_t* ierr, int32_t* stats, double* t_h, int cap, double* trace_d, int32_t* trace_i, int32_t* ntrace,
                                          int32_t* ctrl) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h)
                         .cells(ntol)
                         .traced(cap, trace_d, trace_i, ntrace, ctrl));
}

int mistra_chem_rosenbrock_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                        double tend, const double* d_atol, const double* d_rtol, int ntol, const double* rpar, const int32_t* ipar,
                                        double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                        void* hip_stream) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, d_atol, d_rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .cells(ntol),
                    hip_stream);
}

int mistra_chem_rosenbrock_trace_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                              double tend, const double* d_atol, const double* d_rtol, int ntol, const double* rpar, const int32_t* ipar,
                                              double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                              void* hip_stream, int cap, double* d_trace_d, int32_t* d_trace_i, int32_t* d_ntrace, int32_t* d_ctrl) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, d_atol, d_rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .cells(ntol)
                        .traced(cap, d_trace_d, d_trace_i, d_ntrace, d_ctrl),
                    hip_stream);
}

// ---- the operators: Fun_x, Jac_SP_x and solves with shift*I - Jac_SP_x at a state the caller gives (kernel VARIANT 8).  No integration
//      and nothing process-wide: neither the options in force, nor the integrator policy, nor step reuse.  Checked before anything touches a device, each
//      with its own text: the mechanism (no user slot) and the arguments.
int mistra_chem_jac_pattern(int mech, int32_t* crow, int32_t* icol, int32_t* diag) {
  if (int rc = builtin_only(mech, "operator entries")) return rc;
  MechTables T;      // read here: the pattern is the table's, the entry needs no device and no mistra_chem_init
  std::string err;
  if (!T.load(mech_dir() + "/" + kMech[mech].name + ".mech", &err)) return fail(err);
  if (T.nvar != kMech[mech].dims.nvar || T.nnz != kMech[mech].dims.lu_nonzero) return fail(std::string(kMech[mech].name) + ".mech does not belong to this library");
  for (int i = 0; crow && i <= T.nvar; i++) crow[i] = T.crow[(size_t)i] + 1;
  for (int i = 0; icol && i < T.nnz; i++) icol[i] = T.icol[(size_t)i] + 1;
  for (int i = 0; diag && i < T.nvar; i++) diag[i] = T.diag[(size_t)i] + 1;
  return 0;
}

static int check_ops(int mech, const void* vdot, const void* jvs, int nshift, const void* shift, int fun_rhs, int nrhs, const void* rhs, const void* x,
                     const void* ising, int ncell) {
  if (int rc = builtin_only(mech, "operator entries")) return rc;
  if (!x && !vdot && !jvs) return fail("mistra_chem_ops: nothing is asked for (vdot, jvs and x are all null)");
  if (nrhs < 0) return fail("mistra_chem_ops: negative nrhs");
  if (x && (fun_rhs ? 1 : 0) + nrhs < 1) return fail("mistra_chem_ops: a solve without a right-hand side (fun_rhs = 0 and nrhs = 0)");
  if (nrhs > MISTRA_OPS_MAX_RHS) return fail("mistra_chem_ops: nrhs is above MISTRA_OPS_MAX_RHS (" + std::to_string(MISTRA_OPS_MAX_RHS) + ")");
  if (x && nrhs > 0 && !rhs) return fail("mistra_chem_ops: null rhs pointer with nrhs > 0 (rhs: [nrhs][ncell][NVAR])");
  if (x && !ising) return fail("mistra_chem_ops: null ising pointer (ising: [ncell])");
  if (x && !shift) return fail("mistra_chem_ops: null shift pointer (shift: [nshift])");
  if (nshift != 1 && nshift != ncell) return fail("mistra_chem_ops: nshift is neither 1 (shared) nor ncell (one per cell)");
  return 0;
}

// the kernel's arguments of an operator call on device arrays; x null: no solve (rhs, shift, ising are not looked at)
static KernelArgs ops_args(const MechState& S, int ncell, const double* var, const double* fix, const double* rconst, double* vdot, double* jvs, int nshift,
                           const double* shift, int fun_rhs, int nrhs, const double* rhs, double* x, int32_t* ising, size_t block_cells, size_t nv) {
  KernelArgs a = make_args(S, ncell, var, fix, rconst, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr);
  a.opt = nullptr;      // (the options in force are not the operators' business)
  a.ops_vdot = vdot; a.ops_jvs = jvs;
  if (x) {
    a.ops_x = x; a.ops_rhs = nrhs > 0 ? rhs : nullptr; a.ops_shift = shift; a.ops_ising = ising;
    a.ops_shift_stride = nshift == 1 ? 0 : 1; a.ops_fun_rhs = fun_rhs ? 1 : 0; a.ops_nrhs = nrhs;
    a.ops_x_block = a.ops_rhs_block = (int64_t)(block_cells * nv);
  }
  return a;
}

static int launch_ops(DeviceState& D, int mech, const KernelArgs& a, hipStream_t stream) {
  const LaunchFn fn = kMech[mech].unit.fn[8][kRos3];
  if (!fn) return fail("no operator kernel for this mechanism");
  const hipError_t e = fn(a, stream, &D.lds_configured[mech][8][kRos3]);
  if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

// one device's share of mistra_chem_ops_ex: its cells up, the kernel, the rows down (synchronous on that device).  The slot's staging is the batched
// host-buffer entries'; the rows of rhs and x are blocks of the caller's [.][total][NVAR] arrays, moved as the dense-output samples are.
static int ops_host_on(DeviceState& D, int mech, int ncell, size_t start, size_t total, const double* var, const double* fix, const double* rconst, double* vdot,
                       double* jvs, int nshift, const double* shift, int fun_rhs, int nrhs, const double* rhs, double* x, int32_t* ising) {
  HIP_TRY(hipSetDevice(D.id));
  MechState& S = D.mech[mech];
  const size_t nv = (size_t)kMech[mech].dims.nvar, nf = (size_t)kMech[mech].dims.nfix, nr = (size_t)kMech[mech].dims.nreact, nz = (size_t)kMech[mech].dims.lu_nonzero;
  const size_t nc = (size_t)ncell, nrow = x ? (size_t)((fun_rhs ? 1 : 0) + nrhs) : 0, nin = x ? (size_t)nrhs : 0, nsh = x ? (nshift == 1 ? 1 : nc) : 0;
  HIP_TRY(S.s_var.reserve(nc * nv));
  HIP_TRY(S.s_fix.reserve(nc * nf));
  HIP_TRY(S.s_rct.reserve(nc * nr));
  HIP_TRY(S.s_ierr.reserve(nc));
  // one arena: vdot | jvs | shift | rhs | x
  const size_t o_vdot = 0, o_jvs = o_vdot + (vdot ? nc * nv : 0), o_shift = o_jvs + (jvs ? nc * nz : 0), o_rhs = o_shift + nsh, o_x = o_rhs + nin * nc * nv;
  HIP_TRY(S.s_ops.reserve(o_x + nrow * nc * nv + 1));
  double* const B = S.s_ops.p;
  HIP_TRY(hipMemcpy(S.s_var.p, var + start * nv, nc * nv * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.s_fix.p, fix + start * nf, nc * nf * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.s_rct.p, rconst + start * nr, nc * nr * sizeof(double), hipMemcpyHostToDevice));
  if (nsh) HIP_TRY(hipMemcpy(B + o_shift, shift + (nshift == 1 ? 0 : start), nsh * sizeof(double), hipMemcpyHostToDevice));
  if (nin) HIP_TRY(hipMemcpy2D(B + o_rhs, nc * nv * sizeof(double), rhs + start * nv, total * nv * sizeof(double), nc * nv * sizeof(double), nin, hipMemcpyHostToDevice));
  const KernelArgs a = ops_args(S, ncell, S.s_var.p, S.s_fix.p, S.s_rct.p, vdot ? B + o_vdot : nullptr, jvs ? B + o_jvs : nullptr, nshift, B + o_shift, fun_rhs, nrhs,
                                B + o_rhs, x ? B + o_x : nullptr, S.s_ierr.p, nc, nv);
  if (int rc = launch_ops(D, mech, a, nullptr)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (vdot) HIP_TRY(hipMemcpy(vdot + start * nv, B + o_vdot, nc * nv * sizeof(double), hipMemcpyDeviceToHost));
  if (jvs) HIP_TRY(hipMemcpy(jvs + start * nz, B + o_jvs, nc * nz * sizeof(double), hipMemcpyDeviceToHost));
  if (x) {
    HIP_TRY(hipMemcpy2D(x + start * nv, total * nv * sizeof(double), B + o_x, nc * nv * sizeof(double), nc * nv * sizeof(double), nrow, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ising + start, S.s_ierr.p, nc * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return 0;
}

int mistra_chem_ops_ex(int mech, int ncell, const double* var, const double* fix, const double* rconst, double* vdot, double* jvs, int nshift,
                       const double* shift, int fun_rhs, int nrhs, const double* rhs, double* x, int32_t* ising) {
  if (int rc = check_ops(mech, vdot, jvs, nshift, shift, fun_rhs, nrhs, rhs, x, ising, ncell)) return rc;
  if (x)
    for (int i = 0; i < nshift; i++)
      if (!std::isfinite(shift[i])) return fail("mistra_chem_ops_ex: shift[" + std::to_string(i) + "] is not finite");
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, ncell)) return rc;
  if (ncell == 0) return 0;
  if (!var || !fix || !rconst) return fail("null host pointer");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;      // (the slots' staging: refused while a column step is open)
  return on_cell_blocks(ncell, [=](DeviceState& D, size_t start, int count) {
    return ops_host_on(D, mech, count, start, (size_t)ncell, var, fix, rconst, vdot, jvs, nshift, shift, fun_rhs, nrhs, rhs, x, ising);
  });
}

int mistra_chem_ops_device(int mech, int ncell, const double* d_var, const double* d_fix, const double* d_rconst, double* d_vdot, double* d_jvs, int nshift,
                           const double* d_shift, int fun_rhs, int nrhs, const double* d_rhs, double* d_x, int32_t* d_ising, void* hip_stream) {
  if (int rc = check_ops(mech, d_vdot, d_jvs, nshift, d_shift, fun_rhs, nrhs, d_rhs, d_x, d_ising, ncell)) return rc;
  if (ncell == 0) return check_call(mech, 0);
  if (!d_var || !d_fix || !d_rconst) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", 0, &t)) return rc;
  std::lock_guard<std::mutex> lock(g_mu);
  const KernelArgs a = ops_args(*t.S, ncell, d_var, d_fix, d_rconst, d_vdot, d_jvs, nshift, d_shift, fun_rhs, nrhs, d_rhs, d_x, d_ising, (size_t)ncell,
                                (size_t)kMech[mech].dims.nvar);
  return launch_ops(*t.D, mech, a, static_cast<hipStream_t>(hip_stream));
}

// ---- the replay: Ros3 along a step sequence the caller prescribes, every step accepted, its Err handed back (kernel VARIANT 9).  The
//      options of the call give AbsTol, RelTol and Autonomous; the options in force, the integrator policy and step reuse are not involved.  Checked before
//      anything touches a device, each refusal by its text: the mechanism (no user slot), the table and the method.
// counts_on_host: nsteps is a host array (always but for the device entries' per-cell rows)
static int check_replay(const RosRequest& q, bool counts_on_host) {
  if (int rc = builtin_only(q.mech, "replay entries")) return rc;
  if (!q.rpar || !q.ipar) return fail("null options pointer");
  if (q.replay_cap < 0) return fail("replay: negative step capacity");
  if (q.hrows != 1 && q.hrows != q.ncell) return fail("replay: hrows = " + std::to_string(q.hrows) + " is neither 1 (one sequence shared by all cells) nor ncell (one per cell)");
  if (q.replay_cap > 0 && !q.hsteps) return fail("replay: step capacity > 0 with a null hsteps pointer (hsteps: [hrows][cap])");
  if (!q.nsteps) return fail("replay: null nsteps pointer (nsteps: [hrows])");
  if (counts_on_host)
    for (int r = 0; r < q.hrows; r++)
      if (q.nsteps[r] < 0 || q.nsteps[r] > q.replay_cap)
        return fail("replay: nsteps[" + std::to_string(r) + "] = " + std::to_string(q.nsteps[r]) + " lies outside 0 .. cap = " + std::to_string(q.replay_cap));
  if (q.ipar[3] != 2) return fail("the replay is built for Ros3 (ipar[3] = 2) only");
  return 0;
}

int mistra_chem_rosenbrock_replay_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                     const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, int cap, int hrows,
                                     const double* hsteps, const int32_t* nsteps, double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                     double* err_log) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h)
                         .replayed(cap, hrows, hsteps, nsteps, err_log));
}

int mistra_chem_rosenbrock_replay_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                           const double* atol, const double* rtol, int ntol, const double* rpar, const int32_t* ipar, int cap, int hrows,
                                           const double* hsteps, const int32_t* nsteps, double* var_out, int32_t* ierr, int32_t* stats, double* t_h,
                                           double* err_log) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h)
                         .cells(ntol)
                         .replayed(cap, hrows, hsteps, nsteps, err_log));
}

int mistra_chem_rosenbrock_replay_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                         double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, int cap, int hrows,
                                         const double* hsteps, const int32_t* nsteps, double* d_var_out, int32_t* d_ierr, int32_t* d_stats,
                                         double* d_texit_hexit, double* d_err_log, void* hip_stream) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, atol, rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit)
                        .replayed(cap, hrows, hsteps, nsteps, d_err_log),
                    hip_stream);
}

int mistra_chem_rosenbrock_replay_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                               double tend, const double* d_atol, const double* d_rtol, int ntol, const double* rpar, const int32_t* ipar,
                                               int cap, int hrows, const double* hsteps, const int32_t* nsteps, double* d_var_out, int32_t* d_ierr,
                                               int32_t* d_stats, double* d_texit_hexit, double* d_err_log, void* hip_stream) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, d_atol, d_rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit)
                        .cells(ntol)
                        .replayed(cap, hrows, hsteps, nsteps, d_err_log),
                    hip_stream);
}

// ---- the reaction flux: Rosenbrock_x as above, plus every reaction's rate integrated over the call (kernel VARIANT 6).  One
//      more output of the request.  Checked before anything touches a device: the mechanism (no user slot) and the flux pointer.
static int check_flux(int mech, const void* flux) {
  if (int rc = builtin_only(mech, "reaction-flux entries")) return rc;
  if (!flux) return fail("null flux pointer (flux: [ncell][NREACT])");
  return 0;
}

int mistra_chem_rosenbrock_flux_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                   const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr,
                                   int32_t* stats, double* t_h, double* flux) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h).with_flux(flux));
}

int mistra_chem_rosenbrock_flux_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                       double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                       double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                       void* hip_stream, double* d_flux) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, atol, rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .with_flux(d_flux),
                    hip_stream);
}

int mistra_chem_rosenbrock_flux_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart,
                                         double tend, const double* atol, const double* rtol, int ntol, const double* rpar, const int32_t* ipar,
                                         double* var_out, int32_t* ierr, int32_t* stats, double* t_h, double* flux) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h).cells(ntol).with_flux(flux));
}

int mistra_chem_rosenbrock_flux_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                             double tend, const double* d_atol, const double* d_rtol, int ntol, const double* rpar,
                                             const int32_t* ipar, double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                             const double* d_hstart, void* hip_stream, double* d_flux) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, d_atol, d_rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .cells(ntol)
                        .with_flux(d_flux),
                    hip_stream);
}

// ---- dense output: Rosenbrock_x as above, plus the state at ns sample times inside the call, by the cubic Hermite interpolant between the accepted states
//      (kernel VARIANT 7).  Two more outputs of the request.  Checked before anything touches a device, each refusal by its
//      text: the mechanism (no user slot), the pointers, the count and the times against the call's interval and direction (the kernel's: Tend >= Tstart).
static int check_dense(int mech, double tstart, double tend, int ns, const double* ts, const void* ysample, const void* nout) {
  if (int rc = builtin_only(mech, "dense-output entries")) return rc;
  if (ns < 1 || ns > MISTRA_DENSE_MAX_TIMES)
    return fail("dense output: ns = " + std::to_string(ns) + ": a call takes 1 .. MISTRA_DENSE_MAX_TIMES = " + std::to_string(MISTRA_DENSE_MAX_TIMES) + " sample times");
  if (!ts) return fail("dense output: null ts pointer (ts: [ns], a host array)");
  if (!ysample) return fail("dense output: null ysample pointer (ysample: [ns][ncell][NVAR])");
  if (!nout) return fail("dense output: null nout pointer (nout: [ncell])");
  const double dir = tend >= tstart ? 1.0 : -1.0;
  for (int k = 0; k < ns; k++)
    if (!std::isfinite(ts[k])) return fail("dense output: ts[" + std::to_string(k) + "] is not finite");
  for (int k = 1; k < ns; k++) {
    if (ts[k] == ts[k - 1]) return fail("dense output: ts[" + std::to_string(k) + "] repeats ts[" + std::to_string(k - 1) + "]: the sample times are strictly monotone");
    if (!(dir * (ts[k] - ts[k - 1]) > 0.0))
      return fail("dense output: the sample times change direction at ts[" + std::to_string(k) + "]: they run from Tstart towards Tend");
  }
  for (int k = 0; k < ns; k++) {
    if (!(dir * (ts[k] - tstart) > 0.0)) return fail("dense output: ts[" + std::to_string(k) + "] does not lie behind Tstart in the call's direction (Tstart itself is no sample)");
    if (!(dir * (tend - ts[k]) >= 0.0)) return fail("dense output: ts[" + std::to_string(k) + "] lies beyond Tend");
  }
  return 0;
}

int mistra_chem_rosenbrock_dense_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart, double tend,
                                    const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, double* var_out, int32_t* ierr,
                                    int32_t* stats, double* t_h, int ns, const double* ts, double* ysample, int32_t* nout) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h)
                         .sampled(ns, ts, ysample, nout));
}

int mistra_chem_rosenbrock_dense_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                        double tend, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                        double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, const double* d_hstart,
                                        void* hip_stream, int ns, const double* ts, double* d_ysample, int32_t* d_nout) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, atol, rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .sampled(ns, ts, d_ysample, d_nout),
                    hip_stream);
}

int mistra_chem_rosenbrock_dense_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, double tstart,
                                          double tend, const double* atol, const double* rtol, int ntol, const double* rpar, const int32_t* ipar,
                                          double* var_out, int32_t* ierr, int32_t* stats, double* t_h, int ns, const double* ts, double* ysample,
                                          int32_t* nout) {
  return single_host(ros_request(mech, ncell, var_in, fix, rconst, tstart, tend, atol, rtol, rpar, ipar, var_out, ierr, stats, t_h)
                         .cells(ntol)
                         .sampled(ns, ts, ysample, nout));
}

int mistra_chem_rosenbrock_dense_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, double tstart,
                                              double tend, const double* d_atol, const double* d_rtol, int ntol, const double* rpar,
                                              const int32_t* ipar, double* d_var_out, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                              const double* d_hstart, void* hip_stream, int ns, const double* ts, double* d_ysample, int32_t* d_nout) {
  return ros_device(ros_request(mech, ncell, d_var_in, d_fix, d_rconst, tstart, tend, d_atol, d_rtol, rpar, ipar, d_var_out, d_ierr, d_stats, d_texit_hexit, d_hstart)
                        .cells(ntol)
                        .sampled(ns, ts, d_ysample, d_nout),
                    hip_stream);
}

// ---- series: nleg calls of Rosenbrock_x over times[0 .. nleg] in one launch, the state on chip from leg to leg (kernel VARIANT 5).  One path for the
//      four entries, as above: the shared-pair forms pass ct = nullptr.  The options in force, the integrator policy and step reuse are not read; the
//      zero-pivot rows are not recorded (mistra_chem_singular_rows keeps describing the last call that is not a series).
//      flux_series (the entries with the reaction flux of every leg, below): null = the series as it is; set = kernel VARIANT 11 writes leg k's flux rows
//      at flux_series + k*ncell*NREACT, staged per device slot by the _ex forms as var_series is.

// what every series entry checks before anything touches a device, each refusal by its text
// (rconst_legs, fix_legs: the blocks of rconst and fix, 1 = shared by all legs or nleg = the leg's own; the entries without them pass 1, 1)
// (sflux: the entries with the reaction flux of every leg, which a user slot refuses as it refuses the flux entries; flux_series is theirs)
static int check_series(int mech, int nleg, const double* times, const void* var_series, int rconst_legs = 1, int fix_legs = 1, bool sflux = false,
                        const void* flux_series = nullptr) {
  if (int rc = builtin_only(mech, sflux ? "reaction-flux entries" : "series of Rosenbrock_x calls")) return rc;
  if (nleg < 1 || nleg > MISTRA_SERIES_MAX_LEGS)
    return fail("series: nleg = " + std::to_string(nleg) + ": a series has 1 .. MISTRA_SERIES_MAX_LEGS = " + std::to_string(MISTRA_SERIES_MAX_LEGS) + " legs");
  if (rconst_legs != 1 && rconst_legs != nleg)
    return fail("series: rconst_legs = " + std::to_string(rconst_legs) + ": rconst has 1 block (shared by all legs) or nleg = " + std::to_string(nleg) + " blocks");
  if (fix_legs != 1 && fix_legs != nleg)
    return fail("series: fix_legs = " + std::to_string(fix_legs) + ": fix has 1 block (shared by all legs) or nleg = " + std::to_string(nleg) + " blocks");
  if (!times) return fail("series: null times pointer (times: [nleg + 1], a host array)");
  if (!var_series) return fail("series: null var_series pointer (var_series: [nleg][ncell][NVAR])");
  if (sflux && !flux_series) return fail("series: null flux_series pointer (flux_series: [nleg][ncell][NREACT])");
  for (int k = 0; k <= nleg; k++)
    if (!std::isfinite(times[k])) return fail("series: times[" + std::to_string(k) + "] is not finite");
  for (int k = 1; k <= nleg; k++) {
    if (times[k] == times[k - 1]) return fail("series: times[" + std::to_string(k) + "] repeats times[" + std::to_string(k - 1) + "]: the times are strictly monotone");
    if ((times[k] > times[k - 1]) != (times[1] > times[0]))
      return fail("series: the times change direction at times[" + std::to_string(k) + "]: ascending or descending, one of them for the whole series");
  }
  return 0;
}

// the series with rate constants linear in time: the one argument of their own (the node blocks take the place of rconst and its count)
static int check_nodes(const double* rconst_nodes) {
  if (!rconst_nodes) return fail("series: null rconst_nodes pointer (rconst_nodes: [nleg + 1][ncell][NREACT], block k the rate constants at times[k])");
  return 0;
}

// ---- the two paths of every request.  What the families check before anything touches a device keeps each family's own order of refusals: the shared
//      paths run this first and repeat the generic tests behind it.
static int check_request(const RosRequest& q, bool device) {
  if (!q.options) return q.env && known_mech(q.mech) && kMech[q.mech].user ? fail_user_slot(q.mech, "rate table") : 0;      // (mistra_chem_integrate_hstart_ex with env)
  const bool null_options = !q.atol || !q.rtol || !q.rpar || !q.ipar;
  if (q.series) {
    if (int rc = check_series(q.mech, q.nleg, q.times, q.var_out, q.rconst_legs, q.fix_legs, q.wants_flux, q.flux)) return rc;
    if (q.lin)
      if (int rc = check_nodes(q.rconst)) return rc;
  } else if (q.replay) {
    if (int rc = check_replay(q, !device || !q.own_rows())) return rc;
    if (device && !q.own_rows() && q.nsteps[0] > MISTRA_REPLAY_MAX_SHARED)
      return fail("replay: nsteps[0] = " + std::to_string(q.nsteps[0]) + ": a shared sequence of the device entries holds at most MISTRA_REPLAY_MAX_SHARED = " +
                  std::to_string(MISTRA_REPLAY_MAX_SHARED) + " steps (it travels in the call's block); give every cell its row");
  } else if (q.trace) {
    if (int rc = builtin_only(q.mech, "step-control trace")) return rc;
    if (!q.per_cell && null_options) return fail("null options pointer");
  } else if (q.wants_flux) {
    if (int rc = check_flux(q.mech, q.flux)) return rc;
  } else if (q.dense) {
    if (int rc = check_dense(q.mech, q.tstart, q.tend, q.ns, q.ts, q.ysample, q.nout)) return rc;
  } else if (int rc = user_slot_method(q.mech, q.ipar)) {
    return rc;
  }
  if (q.per_cell)
    if (int rc = check_cell_tol(q)) return rc;
  if (q.trace)
    if (int rc = check_trace_args(q)) return rc;
  if ((q.series || q.replay) && null_options) return fail("null options pointer");      // (the single calls: behind check_call, in the paths)
  return user_slot_method(q.mech, q.ipar);
}

// Rosenbrock_x refused the options: it returns before it touches Y or the statistics (gas.f:936-1053).  A result, nothing is launched: every leg (one
// for the single calls) gets var = var_in, the code and zeros; no attempt was made and no sample reached, and the trace logs, ctrl and the replay's err
// stay as they are.  Two writers: the host call's, and the device call's in stream order.
static int refuse_host(const RosRequest& q, int code) {
  const size_t nv = (size_t)kMech[q.mech].dims.nvar, nr = (size_t)kMech[q.mech].dims.nreact, nc = (size_t)q.ncell, n = q.legs() * nc;
  for (size_t k = 0; k < q.legs(); k++)
    if (q.var_out + k * nc * nv != q.var_in) std::memmove(q.var_out + k * nc * nv, q.var_in, nc * nv * sizeof(double));
  if (q.ierr) std::fill(q.ierr, q.ierr + n, (int32_t)code);
  if (q.stats) std::fill(q.stats, q.stats + n * 8, 0);
  if (q.th) std::fill(q.th, q.th + n * 3, 0.0);
  if (q.trace) std::fill(q.ntrace, q.ntrace + nc, 0);
  if (q.flux) std::fill(q.flux, q.flux + n * nr, 0.0);
  if (q.dense) {
    std::fill(q.ysample, q.ysample + (size_t)q.ns * nc * nv, 0.0);
    std::fill(q.nout, q.nout + nc, 0);
  }
  return 0;
}
static int refuse_stream(const RosRequest& q, int code, hipStream_t st) {
  const size_t nv = (size_t)kMech[q.mech].dims.nvar, nr = (size_t)kMech[q.mech].dims.nreact, nc = (size_t)q.ncell, n = q.legs() * nc;
  for (size_t k = 0; k < q.legs(); k++)
    if (q.var_out + k * nc * nv != q.var_in) HIP_TRY(hipMemcpyAsync(q.var_out + k * nc * nv, q.var_in, nc * nv * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(q.ierr), code, n, st));
  HIP_TRY(hipMemsetAsync(q.stats, 0, n * 8 * sizeof(int32_t), st));
  if (q.th) HIP_TRY(hipMemsetAsync(q.th, 0, n * 2 * sizeof(double), st));
  if (q.trace) HIP_TRY(hipMemsetAsync(q.ntrace, 0, nc * sizeof(int32_t), st));
  if (q.flux) HIP_TRY(hipMemsetAsync(q.flux, 0, n * nr * sizeof(double), st));
  if (q.dense) {
    HIP_TRY(hipMemsetAsync(q.ysample, 0, (size_t)q.ns * nc * nv * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(q.nout, 0, nc * sizeof(int32_t), st));
  }
  return 0;
}

// Host buffers: the batch is split over the device slots (on_cell_blocks), each slot stages its cells, runs the kernel and fetches (ros_host_on).
static int ros_host(const RosRequest& q) {
  if (int rc = check_request(q, false)) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(q.mech, q.ncell, true)) return rc;
  if (q.options && (!q.atol || !q.rtol || !q.rpar || !q.ipar)) return fail("null options pointer");
  if (q.ncell == 0) return 0;
  if (!q.var_in || !q.fix || !q.var_out || (!q.rconst && !q.env)) return fail("null host pointer");
  std::lock_guard<std::mutex> lock(g_mu);      // (g_max_steps, the slots' staging)
  Slot t;
  if (int rc = on_primary(q.mech, q.env ? kNeedRates : 0, true, &t)) return rc;
  RosCall call;
  std::vector<double> blk;
  BlockLayout L;
  if (q.options) {
    call = decode_call(q);
    if (call.ierr != 1) return refuse_host(q, call.ierr);
    blk.resize(put_block(nullptr, call, q).words);
    L = put_block(blk.data(), call, q);      // one upload per slot, read by the kernel through the options pointer
  }
  if (q.record_sing)
    for (auto& d : g_devs) d.mech[q.mech].sing_count = 0;
  return on_cell_blocks(q.ncell, [&](DeviceState& D, size_t start, int count) {
    return ros_host_on(D, q, q.options ? &call : nullptr, blk, L, start, (size_t)count);
  });
}

// Device pointers: the buffers decide the device, the call is queued on the caller's stream and returns.  The kernel reads the caller's arrays in
// stream order, no copy but the call's block: a plain call's in the slot's call_ring, one with a tail in series_ring, whose blocks have the room.
static int ros_device(const RosRequest& q, void* hip_stream) {
  if (int rc = check_request(q, true)) return rc;
  if (q.ncell == 0) return check_call(q.mech, 0, true);
  if (!q.atol || !q.rtol || !q.rpar || !q.ipar) return fail("null options pointer");
  if (!q.var_in || !q.fix || !q.rconst || !q.var_out || !q.ierr || !q.stats) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(q.mech, q.ncell, q.var_in, "d_var_in", 0, &t)) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (q.per_cell)
    if (int rc = check_reachable({q.atol, q.rtol}, t.D->id, "d_atol / d_rtol are not device arrays on the cells' device")) return rc;
  if (q.own_rows())
    if (int rc = check_reachable({q.hsteps, q.nsteps}, t.D->id,
                                 "replay: hsteps / nsteps with hrows = ncell are not device arrays on the cells' device (a shared sequence, hrows = 1, is a host array)"))
      return rc;
  std::lock_guard<std::mutex> lock(g_mu);      // (g_max_steps, the slot's rings of blocks)
  const RosCall call = decode_call(q);
  if (call.ierr != 1) return refuse_stream(q, call.ierr, st);
  static_assert(MISTRA_DENSE_MAX_TIMES <= MISTRA_SERIES_MAX_LEGS + 1, "the sample times travel in a block of the series' ring");
  static_assert(MISTRA_REPLAY_MAX_SHARED + 1 <= MISTRA_SERIES_MAX_LEGS + 1, "a shared sequence and its count travel in a block of the series' ring");
  const bool tail = q.series || q.dense || q.replay;
  RosCallRing& R = tail ? t.S->series_ring : t.S->call_ring;
  int i;
  double *hb, *db;
  HIP_TRY(R.acquire(call.block.size() + (tail ? (size_t)MISTRA_SERIES_MAX_LEGS + 1 : 0), &i, &hb, &db));
  const BlockLayout L = put_block(hb, call, q);
  HIP_TRY(hipMemcpyAsync(db, hb, L.words * sizeof(double), hipMemcpyHostToDevice, st));
  const double t0 = q.series ? q.times[0] : q.tstart, t1 = q.series ? q.times[q.nleg] : q.tend;
  KernelArgs a = make_args(*t.S, q.ncell, q.var_in, q.fix, q.rconst, t0, t1, q.var_out, q.ierr, q.stats, q.th);
  bind_request(&a, q, &call, db, L, (size_t)q.ncell, nullptr, nullptr);
  const int rc = launch(*t.D, q.mech, a, st, call.method);
  R.mark(i, st);
  return rc;
}

static RosRequest series_request(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int rconst_legs, int fix_legs, int nleg,
                                 const double* times, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, int carry_h,
                                 const double* hstart, double* var_series, int32_t* ierr, int32_t* stats, double* th) {
  return ros_request(mech, ncell, var_in, fix, rconst, 0.0, 0.0, atol, rtol, rpar, ipar, var_series, ierr, stats, th, hstart).over(nleg, times, carry_h, rconst_legs, fix_legs);
}

int mistra_chem_rosenbrock_series_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int nleg, const double* times,
                                     const double* atol, const double* rtol, const double* rpar, const int32_t* ipar, int carry_h, const double* hstart,
                                     double* var_series, int32_t* ierr, int32_t* stats, double* t_h) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst, 1, 1, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats, t_h));
}

int mistra_chem_rosenbrock_series_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int nleg, const double* times,
                                           const double* atol, const double* rtol, int ntol, const double* rpar, const int32_t* ipar, int carry_h,
                                           const double* hstart, double* var_series, int32_t* ierr, int32_t* stats, double* t_h) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst, 1, 1, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats, t_h).cells(ntol));
}

int mistra_chem_rosenbrock_series_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, int nleg,
                                         const double* times, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                         double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, int carry_h,
                                         const double* d_hstart, void* hip_stream) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst, 1, 1, nleg, times, atol, rtol, rpar, ipar, carry_h, d_hstart, d_var_series, d_ierr, d_stats,
                                   d_texit_hexit),
                    hip_stream);
}

int mistra_chem_rosenbrock_series_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, int nleg,
                                               const double* times, const double* d_atol, const double* d_rtol, int ntol, const double* rpar,
                                               const int32_t* ipar, double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                               int carry_h, const double* d_hstart, void* hip_stream) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst, 1, 1, nleg, times, d_atol, d_rtol, rpar, ipar, carry_h, d_hstart, d_var_series, d_ierr,
                                   d_stats, d_texit_hexit)
                        .cells(ntol),
                    hip_stream);
}

// ---- the series with rate constants and FIX of the leg's own: the two counts the caller's
int mistra_chem_rosenbrock_series_rates_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int rconst_legs, int fix_legs,
                                           int nleg, const double* times, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                           int carry_h, const double* hstart, double* var_series, int32_t* ierr, int32_t* stats, double* t_h) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats,
                                 t_h));
}

int mistra_chem_rosenbrock_series_rates_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int rconst_legs,
                                                 int fix_legs, int nleg, const double* times, const double* atol, const double* rtol, int ntol,
                                                 const double* rpar, const int32_t* ipar, int carry_h, const double* hstart, double* var_series,
                                                 int32_t* ierr, int32_t* stats, double* t_h) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats,
                                 t_h)
                      .cells(ntol));
}

int mistra_chem_rosenbrock_series_rates_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, int rconst_legs,
                                               int fix_legs, int nleg, const double* times, const double* atol, const double* rtol, const double* rpar,
                                               const int32_t* ipar, double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                               int carry_h, const double* d_hstart, void* hip_stream) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, d_hstart, d_var_series,
                                   d_ierr, d_stats, d_texit_hexit),
                    hip_stream);
}

int mistra_chem_rosenbrock_series_rates_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                                     int rconst_legs, int fix_legs, int nleg, const double* times, const double* d_atol,
                                                     const double* d_rtol, int ntol, const double* rpar, const int32_t* ipar, double* d_var_series,
                                                     int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, int carry_h, const double* d_hstart,
                                                     void* hip_stream) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst, rconst_legs, fix_legs, nleg, times, d_atol, d_rtol, rpar, ipar, carry_h, d_hstart,
                                   d_var_series, d_ierr, d_stats, d_texit_hexit)
                        .cells(ntol),
                    hip_stream);
}

// ---- the series with rate constants linear in time over each leg (kernel VARIANT 10): rconst_nodes holds nleg + 1 blocks, block k
//      the rate constants AT times[k]; FIX stays piecewise constant (fix_legs = 1 or nleg)
int mistra_chem_rosenbrock_series_linrates_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst_nodes, int fix_legs, int nleg,
                                              const double* times, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                              int carry_h, const double* hstart, double* var_series, int32_t* ierr, int32_t* stats, double* t_h) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst_nodes, 1, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats, t_h)
                      .linear());
}

int mistra_chem_rosenbrock_series_linrates_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst_nodes, int fix_legs,
                                                    int nleg, const double* times, const double* atol, const double* rtol, int ntol, const double* rpar,
                                                    const int32_t* ipar, int carry_h, const double* hstart, double* var_series, int32_t* ierr,
                                                    int32_t* stats, double* t_h) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst_nodes, 1, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats, t_h)
                      .linear()
                      .cells(ntol));
}

int mistra_chem_rosenbrock_series_linrates_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst_nodes, int fix_legs,
                                                  int nleg, const double* times, const double* atol, const double* rtol, const double* rpar,
                                                  const int32_t* ipar, double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                                  int carry_h, const double* d_hstart, void* hip_stream) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst_nodes, 1, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, d_hstart, d_var_series,
                                   d_ierr, d_stats, d_texit_hexit)
                        .linear(),
                    hip_stream);
}

int mistra_chem_rosenbrock_series_linrates_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst_nodes,
                                                        int fix_legs, int nleg, const double* times, const double* d_atol, const double* d_rtol, int ntol,
                                                        const double* rpar, const int32_t* ipar, double* d_var_series, int32_t* d_ierr, int32_t* d_stats,
                                                        double* d_texit_hexit, int carry_h, const double* d_hstart, void* hip_stream) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst_nodes, 1, fix_legs, nleg, times, d_atol, d_rtol, rpar, ipar, carry_h, d_hstart, d_var_series,
                                   d_ierr, d_stats, d_texit_hexit)
                        .linear()
                        .cells(ntol),
                    hip_stream);
}

// ---- the series with the reaction flux of every leg (kernel VARIANT 11): the series with rates' arguments, flux_series
//      [nleg][ncell][NREACT] behind them, leg k's rows what mistra_chem_rosenbrock_flux_device returns for the call that leg k is
int mistra_chem_rosenbrock_series_flux_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int rconst_legs, int fix_legs,
                                          int nleg, const double* times, const double* atol, const double* rtol, const double* rpar, const int32_t* ipar,
                                          int carry_h, const double* hstart, double* var_series, int32_t* ierr, int32_t* stats, double* t_h,
                                          double* flux_series) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats,
                                 t_h)
                      .with_flux(flux_series));
}

int mistra_chem_rosenbrock_series_flux_cells_ex(int mech, int ncell, const double* var_in, const double* fix, const double* rconst, int rconst_legs,
                                                int fix_legs, int nleg, const double* times, const double* atol, const double* rtol, int ntol,
                                                const double* rpar, const int32_t* ipar, int carry_h, const double* hstart, double* var_series,
                                                int32_t* ierr, int32_t* stats, double* t_h, double* flux_series) {
  return ros_host(series_request(mech, ncell, var_in, fix, rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, hstart, var_series, ierr, stats,
                                 t_h)
                      .cells(ntol)
                      .with_flux(flux_series));
}

int mistra_chem_rosenbrock_series_flux_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst, int rconst_legs,
                                              int fix_legs, int nleg, const double* times, const double* atol, const double* rtol, const double* rpar,
                                              const int32_t* ipar, double* d_var_series, int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit,
                                              int carry_h, const double* d_hstart, void* hip_stream, double* d_flux_series) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst, rconst_legs, fix_legs, nleg, times, atol, rtol, rpar, ipar, carry_h, d_hstart, d_var_series,
                                   d_ierr, d_stats, d_texit_hexit)
                        .with_flux(d_flux_series),
                    hip_stream);
}

int mistra_chem_rosenbrock_series_flux_cells_device(int mech, int ncell, const double* d_var_in, const double* d_fix, const double* d_rconst,
                                                    int rconst_legs, int fix_legs, int nleg, const double* times, const double* d_atol,
                                                    const double* d_rtol, int ntol, const double* rpar, const int32_t* ipar, double* d_var_series,
                                                    int32_t* d_ierr, int32_t* d_stats, double* d_texit_hexit, int carry_h, const double* d_hstart,
                                                    void* hip_stream, double* d_flux_series) {
  return ros_device(series_request(mech, ncell, d_var_in, d_fix, d_rconst, rconst_legs, fix_legs, nleg, times, d_atol, d_rtol, rpar, ipar, carry_h, d_hstart,
                                   d_var_series, d_ierr, d_stats, d_texit_hexit)
                        .cells(ntol)
                        .with_flux(d_flux_series),
                    hip_stream);
}

int mistra_chem_cell_atol_device(int mech, int ncell, const double* d_var, double factor, double floor, double* d_atol, void* hip_stream) {
  if (!known_mech(mech)) return fail("unknown mechanism id");
  if (!(factor > 0.0) || !std::isfinite(factor)) return fail("cell_atol: factor must be finite and positive");
  if (!(floor > 0.0) || !std::isfinite(floor)) return fail("cell_atol: floor must be finite and positive");
  if (ncell == 0) return check_call(mech, 0, true);
  if (!d_var || !d_atol) return fail("null device pointer");
  Slot t;
  if (int rc = on_device(mech, ncell, d_var, "d_var", 0, &t)) return rc;
  LAUNCH_TRY(launch_cell_atol(kMech[mech].dims.nvar, ncell, d_var, factor, floor, d_atol, static_cast<hipStream_t>(hip_stream)));
  return 0;
}

int mistra_chem_integrate_common_status(int mech, void* gdata, double* tin, double* tout, int32_t* ierr_out, double* t_err,
                                        double* h_err, int32_t* nsng) {
  if (int rc = builtin_only(mech, "COMMON-block entry")) return rc;
  if (int rc = lazy_init()) return rc;
  if (int rc = check_call(mech, 1)) return rc;
  if (!gdata || !tin || !tout) return fail("null pointer");
  const int nv = kMech[mech].dims.nvar, nf = kMech[mech].dims.nfix, nr = kMech[mech].dims.nreact;
  double* c = static_cast<double*>(gdata);          // C(NSPEC) = VAR | FIX
  double* atol = c + nv + nf + nr + 2;              // after RCONST(NREACT), TIME, DT
  double* rtol = atol + nv;
  double* stepmin = rtol + nv;
  for (int i = 0; i < nv; i++) { rtol[i] = 1.0e-3; atol[i] = 1.0e-25; }   // INTEGRATE_x, gas.f:745-746
  // One call = one cell: what costs here is synchronisation, not bytes.  /GDATA_x/ holds C and RCONST back to back, so the inputs go
  // up in ONE copy from the pinned mirror of the mechanism's one-cell arena and everything the kernel writes comes back in ONE, on the
  // arena's stream with a single wait (seven blocking calls before: 340 us per gas call, of which the kernel is a fraction).
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;
  MechState& S = *t.S;
  if (g_opts[mech].set) {      // what the options in force make the integrator use instead
    std::memcpy(atol, g_opts[mech].block.data() + kOptTol, (size_t)nv * sizeof(double));
    std::memcpy(rtol, g_opts[mech].block.data() + kOptTol + nv, (size_t)nv * sizeof(double));
  }
  const size_t d8 = sizeof(double), n_in = (size_t)(nv + nf + nr) * d8;
  Layout B;
  const size_t o_in = B.take(n_in);      // C | RCONST
  const size_t o_var = B.take(nv * d8), o_th = B.take(2 * d8), o_hl = B.take(d8), o_ierr = B.take(4), o_stats = B.take(8 * 4), o_sing = B.take(8 * 4);
  HIP_TRY(S.one.ensure(B.end));
  const Staging& A = S.one;
  std::memcpy(A.h(o_in), c, n_in);
  HIP_TRY(hipMemcpyAsync(A.d(o_in), A.h(o_in), n_in, hipMemcpyHostToDevice, A.st));
  KernelArgs a = make_args(S, 1, A.d(o_in), A.d(o_in) + nv, A.d(o_in) + nv + nf, *tin, *tout, A.d(o_var), A.d<int32_t>(o_ierr), A.d<int32_t>(o_stats), A.d(o_th));
  a.h_last = A.d(o_hl);
  a.sing_rows = A.d<int32_t>(o_sing);
  if (int rc = launch(*t.D, mech, a, A.st, policy_args(S, &a))) return rc;
  HIP_TRY(hipMemcpyAsync(A.h(o_var), A.d(o_var), B.end - o_var, hipMemcpyDeviceToHost, A.st));
  HIP_TRY(hipStreamSynchronize(A.st));
  std::memcpy(c, A.h(o_var), (size_t)nv * d8);
  const int32_t ierr = *A.h<int32_t>(o_ierr);
  if (ierr_out) *ierr_out = ierr;
  if (nsng) *nsng = A.h<int32_t>(o_stats)[7];
  for (auto& d : g_devs) d.mech[mech].sing_count = 0;
  std::memcpy(S.one_sing, A.h<int32_t>(o_sing), sizeof S.one_sing);
  S.sing_one = true;
  if (t_err) *t_err = A.h(o_th)[0];       // T when the integrator returned
  if (h_err) *h_err = A.h(o_hl)[0];       // H when the integrator returned (what ros_ErrorMsg_x prints)
  *tin = A.h(o_th)[0];                    // TIN = RPAR(11), exit time
  *stepmin = A.h(o_th)[1];                // STEPMIN = RPAR(12), last step
  return 0;
}

int mistra_chem_singular_rows(int mech, int cell, int32_t* rows8) {
  if (int rc = check_call(mech, 1, true)) return rc;
  if (!rows8 || cell < 0) return fail("bad argument");
  std::lock_guard<std::mutex> lock(g_mu);
  Slot t;
  if (int rc = on_primary(mech, 0, true, &t)) return rc;      // (the rows of an open column step are not written yet)
  for (auto& D : g_devs) {
    MechState& S = D.mech[mech];
    if (S.sing_one && cell == 0 && &D == &g_devs[0]) {
      std::memcpy(rows8, S.one_sing, sizeof S.one_sing);
      return 0;
    }
    if (!S.sing_one && S.sing_count > 0 && (size_t)cell >= S.sing_start && (size_t)cell < S.sing_start + S.sing_count) {
      HIP_TRY(hipSetDevice(D.id));
      HIP_TRY(hipMemcpy(rows8, S.s_sing.p + ((size_t)cell - S.sing_start) * 8, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
      (void)hipSetDevice(g_devs[0].id);
      return 0;
    }
  }
  return fail("no host-buffer integration of this mechanism holds that cell");
}

int mistra_chem_integrate_common(int mech, void* gdata, double* tin, double* tout) {
  int32_t ierr = 1, nsng = 0;
  double t_err = 0.0, h_err = 0.0;
  const double tin_in = tin ? *tin : 0.0;
  if (int rc = mistra_chem_integrate_common_status(mech, gdata, tin, tout, &ierr, &t_err, &h_err, &nsng)) return rc;
  if (nsng > 0) {      // ros_PrepareMatrix_x's warning, one per failed decomposition (gas.f:1456)
    int32_t rows[8] = {0};
    (void)mistra_chem_singular_rows(mech, 0, rows);
    for (int i = 0; i < nsng; i++) std::printf(" Warning: LU Decomposition returned ising =  %d\n", rows[i < 8 ? i : 7]);
  }
  if (ierr < 0) {   // the reference prints and continues (ros_ErrorMsg_x gas.f:1474-1509, INTEGRATE_x gas.f:764-767);
                    // a Fortran caller gets the same lines from unit 6 through shim/mistra_kpp_shim.f90
    const char sfx = "gat"[mech];
    std::printf(" Forced exit from Rosenbrock_%c due to the following error:\n", sfx);
    if (const char* txt = ros_error_text(ierr)) std::printf(" %s\n", txt);
    else std::printf("       Unknown Error code: %4d\n", ierr);
    std::printf("        T=%15.7E and H=%15.7E\n", t_err, h_err);
    std::printf(" Rosenbrock: Unsucessful step at T= %g  (IERR= %d )\n", tin_in, ierr);
  }
  return 0;
}

}  // extern "C"
