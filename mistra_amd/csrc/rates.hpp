// Rate-constant tables (mistra_amd/mech/<mech>.rates, written by tools/extract_rates.py) and the device evaluator's entry.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

namespace mistra {

struct RatesDev {              // device copy of one mechanism's table
  const double* consts;        // literal pool
  const int32_t* offs;         // [nreact + 1] first word of each reaction's postfix program
  const int32_t* words;        // opcode | operand << 8   (0 const, 1 env slot, 2 + 3 - 4 * 5 / 6 neg 7 call function id)
  const int32_t* fslot;        // env slots of what the rate-law functions read from COMMON themselves, -1 = not in this mechanism
  int nreact, nenv;            // reactions; doubles per cell in the input vector ("env", layout: tools/extract_rates.py ENV)
};

// Operand-stack entries per thread of the device evaluator (update_rconst_kernel: one LDS column of this many doubles per thread).  The deepest
// program of the shipped tables needs 7 (rates) or 8 (st_coeff); the loaders refuse a table that needs more.
constexpr int kRatesStackDepth = 12;
// arguments each function id of a call word takes off the stack (the call switch of update_rconst_kernel)
constexpr int kRatesCallArgs[29] = {2, 4, 5, 5, 6, 7, 6, 6, 2, 6, 1, 0, 2, 2, 3, 5, 4, 1, 1, 3, 3, 2, 4, 5, 3, 4, 1, 4, 2};

struct RatesTable {
  int nreact = 0, nenv = 0;
  int depth = 0;               // deepest operand stack of any program (rates_stack_depth), set by load
  std::vector<double> consts;
  std::vector<int32_t> offs, words, fslot;
  bool load(const std::string& path, std::string* err);
};

// st_coeff_a / st_coeff_t (kpp.f90:857-1038 | 664-851) as four tables of the same format, one per setting of the namelist switches
// lpJoyce14bc + 2*lpBuxmann15alph (mistra_amd/mech/<mech>.stcoeff, tools/extract_stcoeff.py); outputs = NSPEC, env = 5 doubles per layer
struct StcoeffTable {
  RatesTable v[4];
  bool load(const std::string& path, std::string* err);
};

// deepest operand stack any program of T needs; -1 where a program is not one (words outside the table, an unknown word, a pop from an empty
// stack, not exactly one result left)
int rates_stack_depth(const RatesTable& T);

hipError_t launch_update_rconst(const RatesDev& R, const double* d_env, double* d_rconst, int ncell, hipStream_t stream);

}  // namespace mistra
