// The chunked outside pass (outside_pass.h), what its host side plans from numbers alone: the requests of a call grouped by branch, how
// many tiles of outside vectors fit the scratch budget, and the stride of the per-(request, tile) records.  Host only and free of HIP:
// tests/outside_plan_check.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace hyhip {

// Requests (trials, derivatives) grouped by branch: branches in ascending node code, the requests of a branch in the caller's order.
struct BranchGroups {
  std::vector<int> order;   // [n] request indices, group after group
  std::vector<int> branch;  // [groups] node codes, strictly ascending
  std::vector<int> off;     // [groups + 1] group g is order[off[g] .. off[g + 1])
};
inline BranchGroups group_by_branch(const int64_t *nodes, int64_t n) {
  BranchGroups g;
  g.order.resize((size_t)n);
  std::iota(g.order.begin(), g.order.end(), 0);
  std::stable_sort(g.order.begin(), g.order.end(), [&](int x, int y) { return nodes[x] < nodes[y]; });
  for (int64_t k = 0; k < n; k++)
    if (k == 0 || nodes[g.order[(size_t)k]] != nodes[g.order[(size_t)k - 1]]) {
      g.branch.push_back((int)nodes[g.order[(size_t)k]]);
      g.off.push_back((int)k);
    }
  g.off.push_back((int)n);
  return g;
}

// Tiles of a chunk: as many as keep the V scratch ([B][tiles][tile_bytes]) within the budget, never less than one, never more than there are.
inline int chunk_tiles(double budget_bytes, int64_t B, size_t tile_bytes, int ntiles) {
  return (int)std::min<double>(ntiles, std::max(1., floor(budget_bytes / ((double)B * (double)tile_bytes))));
}

// Records per request: one per tile, padded so that combine_range reads whole 16-byte words.
inline int part_stride(int ntiles) { return (ntiles + 3) / 4 * 4 + 4; }

}  // namespace hyhip
