// Build-time host program (mistra_amd/build.py): runs the schedule compiler on a user mechanism table and writes the traits header of its
// slot, the counterpart of the hand-written GasTraits / AerTraits / TotTraits of ros3_kernel.hpp.
//
//   user_traits_gen <table.mech> <slot 0|1> <out.hpp>      exit 0 and the header, or exit 1 and one line of text on stderr
//
// Counted from the table: NVAR NFIX NREACT NNZ NB NCONST NJNZ.  As the schedule compiler reports them: TAIL_REGS, SCALE_PASS, MAX_TEMPS (the
// partial-sum cells its solve programs use, plus kTempSlack: a table of the same sizes and other contents may need a few more).  A user slot
// never has the dense tail block (DENSE_ND = DENSE_KB = 0, whatever its NVAR).  The size class follows from NVAR alone:
//   NVAR <= 128         64 threads (one wave per cell), the look-ahead ring in its low placement, the register budget of the gas kernel
//   128 < NVAR <= 512   256 threads, two species per lane, the budget of the aer kernel; the rate constants live in LDS (RCT_LDS) only where the
//                       cell's LDS block then still fits twice into a CU
// anything else is refused, and so is a table whose LDS block exceeds the 160 KiB of a CU.
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mech_tables.hpp"
#include "schedule.hpp"

using namespace mistra;

namespace {

constexpr int kTempSlack = 2;
constexpr int kLdsBytes = 160 * 1024;

int round_up2(int x) { return (x + 1) & ~1; }

// ros3_kernel.hpp: LdsLayout<MT, NT> without the dense tail block, in doubles (ros_user_kernel.hip holds the two to each other)
struct Layout {
  int ab = 0, jb = 0, total = 0;
  bool merge = false;
};
Layout lds_layout(const MechTables& t, int njnz, int nt, int max_temps, bool rct_lds) {
  Layout L;
  const int x = round_up2(t.nnz + 2 * t.nvar + 4 + max_temps);
  L.ab = x + round_up2(t.nvar + t.nfix + t.nconst);
  const int ab_trash = t.nreact > t.nb ? t.nreact : t.nb;
  const int jvs_cells = (njnz + nt - 1) / nt * nt, spare = nt >= 128 ? 64 : 32;
  L.merge = jvs_cells + round_up2(ab_trash + spare) <= t.nnz;
  L.jb = L.merge ? jvs_cells : L.ab;
  const int a_cells = L.merge ? t.nreact : ab_trash;
  const int rct = L.ab + round_up2(a_cells + spare);
  const int red = rct + (L.merge && rct_lds ? round_up2(t.nreact) : 0);
  L.total = red + (nt == 64 ? 4 : 32) + 2;
  return L;
}

int refuse(const std::string& path, const std::string& why) {
  std::fprintf(stderr, "%s: %s\n", path.c_str(), why.c_str());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return refuse("user_traits_gen", "usage: user_traits_gen <table.mech> <slot 0|1> <out.hpp>");
  const std::string path = argv[1], out = argv[3];
  const int slot = std::atoi(argv[2]);
  if (slot < 0 || slot > 1) return refuse(path, "there are two user mechanism slots, 0 and 1");
  std::string name = path.substr(path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1);
  if (name.size() > 5 && name.compare(name.size() - 5, 5, ".mech") == 0) name.resize(name.size() - 5);
  for (char c : name)
    if (!(std::isalnum((unsigned char)c) || c == '_')) return refuse(path, "the table's name becomes the mechanism's name: letters, digits and _ only");
  if (name == "gas" || name == "aer" || name == "tot" || name == "user0" || name == "user1") return refuse(path, "the name " + name + " is taken");

  // the size class first, from the header alone
  int32_t hdr[12] = {0};
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return refuse(path, "cannot open the table");
  const bool got = std::fread(hdr, sizeof hdr, 1, f) == 1;
  std::fclose(f);
  if (!got || hdr[0] != 0x48434D4B || hdr[1] != 2) return refuse(path, "not a KMCH v2 mechanism table");
  const int nvar = hdr[2];
  // The lower limit is the kernel's, not a tuning choice: the solves' tail chain is one whole wave of rows (schedule.cpp: build_tail_solve refuses
  // "mechanism smaller than one wave") and the kernel forms its first row H = NVAR - 64 in unsigned arithmetic (ros3_kernel.hip: the tail's
  // xs_tail / r_tail addresses) — below 64 species that wraps around.  Do not lower it without a tail chain of fewer than 64 rows.
  if (nvar < 64 || nvar > 512)
    return refuse(path, "NVAR = " + std::to_string(nvar) + ": no size class for this mechanism (64 <= NVAR <= 128 runs with 64 threads, 128 < NVAR <= 512 with 256)");
  const int nt = nvar <= 128 ? 64 : 256;

  MechTables t;
  std::string err;
  if (!t.load(path, &err)) return refuse(path, err);
  int njnz = 0;
  for (int k = 0; k < t.nnz; k++) njnz += t.jv_ptr[(size_t)k + 1] > t.jv_ptr[(size_t)k];

  try {
    // pass 1: how many partial-sum cells the solve programs take (they do not depend on where the arrays lie)
    int room = (kLdsBytes / 8 - (t.nnz + 2 * t.nvar + 4)) & ~1;
    if (room > 4096) room = 4096;
    if (room < 4) return refuse(path, "mechanism too large: the matrix alone fills the 160 KiB LDS of a CU");
    const Layout L1 = lds_layout(t, njnz, nt, room, false);
    const KernelSchedule K1 = build_kernel_schedule(t, nt, 8u * (uint32_t)L1.ab, room, 0, 0, 8u * (uint32_t)L1.jb);
    const int max_temps = round_up2(K1.n_temps + kTempSlack);
    // the layout: the rate constants in LDS where two cells then still share a CU (the 256-thread class only)
    bool rct_lds = nt == 256 && lds_layout(t, njnz, nt, max_temps, true).merge && lds_layout(t, njnz, nt, max_temps, true).total * 8 * 2 <= kLdsBytes;
    const Layout L = lds_layout(t, njnz, nt, max_temps, rct_lds);
    if (L.total * 8 > kLdsBytes)
      return refuse(path, "the cell's LDS block is " + std::to_string(L.total * 8) + " bytes, a CU has " + std::to_string(kLdsBytes));
    // pass 2: the schedule as mistra_chem_init will compile it
    const KernelSchedule K = build_kernel_schedule(t, nt, 8u * (uint32_t)L.ab, max_temps, 0, 0, 8u * (uint32_t)L.jb);
    if (K.n_jnz != njnz || K.n_temps != K1.n_temps) return refuse(path, "the schedule compiler's two passes disagree");
    if (nt == 64 && K.tail.regs != 1) return refuse(path, "the one-wave class keeps one register of the tail chain");
    const bool scale_pass = K.lu_scale.nslots > 0;

    FILE* o = std::fopen(out.c_str(), "w");
    if (!o) return refuse(out, "cannot write the traits header");
    std::fprintf(o, "// GENERATED by user_traits_gen from %s.mech (mistra_amd/build.py): the traits of user mechanism slot %d.  Not committed.\n", name.c_str(), slot);
    std::fprintf(o, "#pragma once\nnamespace mistra {\n");
    std::fprintf(o,
                 "struct User%dTraits { static constexpr int NVAR = %d, NFIX = %d, NREACT = %d, NNZ = %d, NB = %d, NCONST = %d, NJNZ = %d, TAIL_REGS = %d, "
                 "MAX_TEMPS = %d, WAVES_PER_SIMD = %s, DENSE_ND = 0, DENSE_KB = 0; static constexpr bool RING_LOW = %s, SCALE_PASS = %s, RCT_LDS = %s, GSUM_CHAIN = false; };\n",
                 slot, t.nvar, t.nfix, t.nreact, t.nnz, t.nb, t.nconst, njnz, K.tail.regs, max_temps, nt == 64 ? "MISTRA_GAS_WPS" : "MISTRA_AER_WPS",
                 nt == 64 ? "true" : "false", scale_pass ? "true" : "false", rct_lds ? "true" : "false");
    std::fprintf(o, "constexpr int kUser%dNT = %d;\n", slot, nt);
    std::fprintf(o, "constexpr int kUser%dLdsTotal = %d, kUser%dLdsAB = %d, kUser%dLdsJB = %d, kUser%dTemps = %d;      // what the generator laid out and the compiler used\n",
                 slot, L.total, slot, L.ab, slot, L.jb, slot, K.n_temps);
    std::fprintf(o, "constexpr char kUser%dName[] = \"%s\";\n", slot, name.c_str());
    std::fprintf(o, "}  // namespace mistra\n");
    std::fclose(o);
  } catch (const std::exception& ex) {
    return refuse(path, std::string("schedule compiler: ") + ex.what());
  }
  return 0;
}
