// A host-buffer batch across the device slots: contiguous blocks of cells, one host thread per slot (cells are independent, kpp.f90:4310-4470: nothing
// is exchanged, every slot uploads, integrates and downloads its own block).  No HIP in here: tests/probe/cell_split_probe.cpp runs it on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <thread>
#include <vector>

namespace mistra {

// whether a batch is split at all: one slot, or fewer than two cells per slot, runs whole on slot 0
inline bool cells_are_split(int ncell, int ndev) { return ndev > 1 && ncell >= 2 * ndev; }

// block d of ndev: cells [start, start + count), the first ncell % ndev blocks one cell longer
struct CellBlock {
  size_t start;
  int count;
};
inline CellBlock cell_block(int ncell, int ndev, int d) {
  const int per = ncell / ndev, rem = ncell % ndev;
  return {(size_t)d * per + (size_t)std::min(d, rem), per + (d < rem ? 1 : 0)};
}

// run(d, start, count) -> 0 or a failure, once per block: on the caller's thread where the batch is not split (one block, slot 0), else one thread per
// slot, joined before this returns.  -> what each block returned
template <class F>
std::vector<int> run_cell_blocks(int ncell, int ndev, F&& run) {
  if (!cells_are_split(ncell, ndev)) return {run(0, (size_t)0, ncell)};
  std::vector<int> rcs((size_t)ndev, 0);
  std::vector<std::thread> workers;
  for (int d = 0; d < ndev; d++) {
    const CellBlock b = cell_block(ncell, ndev, d);
    workers.emplace_back([&rcs, &run, b, d]() { rcs[(size_t)d] = run(d, b.start, b.count); });
  }
  for (auto& w : workers) w.join();
  return rcs;
}

}  // namespace mistra
