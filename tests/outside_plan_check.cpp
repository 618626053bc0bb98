// Host-only check of hyphy_amd/csrc/outside_plan.h (tests/test_outside_plan_cpu.py compiles and runs it): the grouping of a call's
// requests by branch, the tiles of a chunk under a scratch budget, and the stride of the per-tile records.  No GPU, no HIP header.
#include <stdio.h>

#include <random>

#include "../hyphy_amd/csrc/outside_plan.h"

namespace {
int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

void check_groups(const std::vector<int64_t> &nodes) {
  const int64_t n = (int64_t)nodes.size();
  const hyhip::BranchGroups g = hyhip::group_by_branch(nodes.data(), n);
  CHECK((int64_t)g.order.size() == n);
  std::vector<int> seen((size_t)n, 0);
  for (int k : g.order) {
    CHECK(k >= 0 && k < n);
    if (k >= 0 && k < n) seen[(size_t)k]++;
  }
  for (int c : seen) CHECK(c == 1);                                             // every request exactly once
  CHECK(g.off.size() == g.branch.size() + 1);
  CHECK(!g.off.empty() && g.off.front() == 0 && g.off.back() == n);
  CHECK((n == 0) == g.branch.empty());
  for (size_t b = 1; b < g.branch.size(); b++) CHECK(g.branch[b - 1] < g.branch[b]);  // strictly ascending
  for (size_t b = 0; b + 1 < g.off.size(); b++) {
    CHECK(g.off[b] < g.off[b + 1]);                                             // no empty group
    for (int k = g.off[b]; k < g.off[b + 1]; k++) {
      CHECK(nodes[(size_t)g.order[(size_t)k]] == g.branch[b]);
      if (k > g.off[b]) CHECK(g.order[(size_t)k - 1] < g.order[(size_t)k]);     // the caller's order within a branch
    }
  }
}

void groups() {
  std::mt19937_64 rng(20240611);
  check_groups({});
  check_groups({7});
  check_groups(std::vector<int64_t>(1000, 3));                                  // all equal
  std::vector<int64_t> v;
  for (int64_t k = 3000; k-- > 0;) v.push_back(k);                              // strictly descending
  check_groups(v);
  v.clear();
  for (int k = 0; k < 2999; k++) v.push_back((k % 3 == 0) ? 50 : (k % 3 == 1) ? 2 : 50 - k % 7);  // interleaved repeats
  check_groups(v);
  for (int round = 0; round < 200; round++) {
    const int64_t n = 1 + (int64_t)(rng() % (round < 150 ? 60 : 4000));
    const int64_t B = 1 + (int64_t)(rng() % (round % 2 ? 5 : 2000));
    v.assign((size_t)n, 0);
    for (int64_t &x : v) x = (int64_t)(rng() % (uint64_t)B);
    check_groups(v);
  }
  const int64_t nodes[] = {5, 1, 5, 0, 1, 5};                                   // one worked example
  const hyhip::BranchGroups g = hyhip::group_by_branch(nodes, 6);
  CHECK((g.branch == std::vector<int>{0, 1, 5}));
  CHECK((g.off == std::vector<int>{0, 1, 3, 6}));
  CHECK((g.order == std::vector<int>{3, 1, 4, 0, 2, 5}));
}

void chunks() {
  std::mt19937_64 rng(77);
  for (int round = 0; round < 2000; round++) {
    const int64_t B = 1 + (int64_t)(rng() % 700);
    const size_t tile_bytes = (size_t)(round % 2 ? 2048 : 128 * 16 * (1 + rng() % 4));
    const int ntiles = 1 + (int)(rng() % 5000);
    const double one = (double)B * (double)tile_bytes;
    CHECK(hyhip::chunk_tiles(0., B, tile_bytes, ntiles) == 1);
    CHECK(hyhip::chunk_tiles(one - 1., B, tile_bytes, ntiles) == 1);            // below one tile
    CHECK(hyhip::chunk_tiles(one, B, tile_bytes, ntiles) == 1);
    CHECK(hyhip::chunk_tiles(one * ntiles, B, tile_bytes, ntiles) == ntiles);   // holds them all
    CHECK(hyhip::chunk_tiles(one * ntiles * 3., B, tile_bytes, ntiles) == ntiles);
    CHECK(hyhip::chunk_tiles(1e300, B, tile_bytes, ntiles) == ntiles);
    if (ntiles > 1) CHECK(hyhip::chunk_tiles(one * ntiles - 1., B, tile_bytes, ntiles) == ntiles - 1);
    int before = 1;
    for (int k = 0; k <= 40; k++) {                                             // monotone in the budget, always within [1, ntiles]
      const int ct = hyhip::chunk_tiles(one * ntiles * 1.1 * k / 40., B, tile_bytes, ntiles);
      CHECK(ct >= 1 && ct <= ntiles && ct >= before);
      before = ct;
    }
  }
  // the shapes the GPU tests chunk: 62 branches, 33 states (48 padded) under 1 MB; 4 states under 0.1 MB
  CHECK(hyhip::chunk_tiles(1048576., 62, (size_t)16 * 48 * 8, 5) == 2);
  CHECK(hyhip::chunk_tiles(104857.6, 62, (size_t)256 * 8, 4) == 1);
  CHECK(hyhip::chunk_tiles(1048576., 30, (size_t)16 * 48 * 8, 5) == 5);
}

void strides() {
  for (int ntiles = 0; ntiles < 5000; ntiles++) {
    const int s = hyhip::part_stride(ntiles);
    CHECK(s % 4 == 0 && s >= ntiles + 4 && s < ntiles + 8);
  }
}
}  // namespace

int main() {
  groups();
  chunks();
  strides();
  if (g_failed) {
    fprintf(stderr, "outside_plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("outside_plan_check: ok\n");
  return 0;
}
