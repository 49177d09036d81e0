// TEST-ONLY: the tail chain's tables as the schedule compiler builds them (mistra_amd/csrc/schedule.hpp: TailSolve), for
// tests/test_tail_addr.py.  Not part of the product library.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../mistra_amd/csrc/mech_tables.hpp"
#include "../../mistra_amd/csrc/schedule.hpp"

using namespace mistra;

struct Probe {
  MechTables m;
  KernelSchedule s;
};

extern "C" {

void* tail_probe_create(const char* mech_path, int nt) {
  Probe* p = new Probe;
  std::string err;
  if (!p->m.load(mech_path, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); delete p; return nullptr; }
  try {
    // the tail tables depend on the mechanism's pattern and the 0.0 cell (nnz + nvar) alone: any LDS base and temp count will do,
    // and the dense block is configured as tests/emu/schedule_emu.cpp does
    const DenseConfig dc = nt >= 512 ? dense_config(p->m) : DenseConfig{0, 0};
    const VmLayout lay{p->m.nnz, p->m.nvar, 768};
    p->s = build_kernel_schedule(p->m, nt, 8u * (uint32_t)(lay.size() + 1000), 768, dc.nd, dc.kb);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "schedule: %s\n", ex.what());
    delete p;
    return nullptr;
  }
  return p;
}
void tail_probe_destroy(void* h) { delete (Probe*)h; }
int tail_probe_regs(void* h) { return ((Probe*)h)->s.tail.regs; }
int tail_probe_zero_cell(void* h) { const Probe* p = (Probe*)h; return VmLayout{p->m.nnz, p->m.nvar, 768}.zero(); }
// which: 0 = fwd, 1 = bwd (16-bit cells), 2 + r = fwd_addr[r], 4 + r = bwd_addr[r].  Copies up to cap words, returns the size.
long tail_probe_table(void* h, int which, unsigned* out, long cap) {
  const TailSolve& T = ((Probe*)h)->s.tail;
  const std::vector<uint32_t>& v = which == 0 ? T.fwd : which == 1 ? T.bwd : which < 4 ? T.fwd_addr[which - 2] : T.bwd_addr[which - 4];
  if (out) std::memcpy(out, v.data(), sizeof(uint32_t) * (size_t)std::min<long>(cap, (long)v.size()));
  return (long)v.size();
}

}  // extern "C"
