// TEST-ONLY, stand-alone: the cell split of the host-buffer entries (mistra_amd/csrc/cell_split.hpp) with a fake per-block callable, for
// 1 .. 4 device slots and 0 .. 9 cells.  The blocks are disjoint and contiguous, cover [0, ncell), equal the per / rem formula the entries used
// before the helper existed, and a block's failure comes back in its slot.  No HIP, no Python; meant to be built with the sanitizers and run directly:
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -o cell_split_probe tests/probe/cell_split_probe.cpp && ./cell_split_probe
// (tests/test_kernel_units.py builds it without them and runs it)
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "../../mistra_amd/csrc/cell_split.hpp"

#define CHECK(cond)                                                                                   \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      std::fprintf(stderr, "ndev %d ncell %d: %s (line %d)\n", ndev, ncell, #cond, __LINE__);         \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)

int main() {
  int cases = 0;
  for (int ndev = 1; ndev <= 4; ndev++)
    for (int ncell = 0; ncell <= 9; ncell++) {
      struct Seen {
        int d;
        size_t start;
        int count;
      };
      std::vector<Seen> seen;
      std::vector<int> owner((size_t)ncell, -1);
      std::mutex mu;
      bool overlap = false;
      const int fail_slot = ncell % ndev;      // the fake block of this slot fails with 7 + slot
      const std::vector<int> rcs = mistra::run_cell_blocks(ncell, ndev, [&](int d, size_t start, int count) {
        std::lock_guard<std::mutex> lock(mu);
        seen.push_back({d, start, count});
        for (size_t c = start; c < start + (size_t)count; c++) {
          if (c >= owner.size() || owner[c] != -1) overlap = true;
          else owner[c] = d;
        }
        return d == fail_slot ? 7 + d : 0;
      });
      const bool split = ndev > 1 && ncell >= 2 * ndev;      // the entries' short cut was `ndev == 1 || ncell < 2 * ndev`
      CHECK(mistra::cells_are_split(ncell, ndev) == split);
      CHECK(!overlap);
      for (int c = 0; c < ncell; c++) CHECK(owner[(size_t)c] != -1);
      CHECK(rcs.size() == (size_t)(split ? ndev : 1) && seen.size() == rcs.size());
      for (const Seen& s : seen) {
        if (!split) {
          CHECK(s.d == 0 && s.start == 0 && s.count == ncell);
          CHECK(rcs[0] == (fail_slot == 0 ? 7 : 0));
          continue;
        }
        const int per = ncell / ndev, rem = ncell % ndev;      // the formula as the entries had it
        CHECK(s.start == (size_t)s.d * per + (size_t)(s.d < rem ? s.d : rem));
        CHECK(s.count == per + (s.d < rem ? 1 : 0));
        CHECK(s.count >= 2);
        CHECK(rcs[(size_t)s.d] == (s.d == fail_slot ? 7 + s.d : 0));
        // contiguous in slot order: a block ends where the next begins, the last at ncell
        const mistra::CellBlock next = s.d + 1 < ndev ? mistra::cell_block(ncell, ndev, s.d + 1) : mistra::CellBlock{(size_t)ncell, 0};
        CHECK(s.start + (size_t)s.count == next.start);
        for (size_t c = s.start; c < s.start + (size_t)s.count; c++) CHECK(owner[c] == s.d);
      }
      cases++;
    }
  std::printf("cell split: %d cases ok\n", cases);
  return 0;
}
