// Nearest-neighbour interchanges (nni.hip), what their host side plans from the tree alone: whether a pair (x, y) of node codes is a
// move, the list of every move, and the per-request tables phase 2 reads.  Host only and free of HIP.
// A move (x, y): c = parent(x) is an internal node other than the root, y is a sibling of c (parent(y) == parent(c) == p, y != c);
// the neighbour tree is the one in which x and y exchange parents.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace hyhip {

// children per internal node, ascending node codes (parents [L + I]: internal index of the parent, the root last with -1)
inline std::vector<std::vector<int>> nni_children(int64_t L, int64_t I, const int64_t *parents) {
  std::vector<std::vector<int>> ch((size_t)I);
  for (int64_t c = 0; c < L + I - 1; c++) ch[(size_t)parents[c]].push_back((int)c);
  return ch;
}

// THE rule, once: nullptr when (x, y) is a move, else what is wrong with it.  The planner lists by it, hyphy_hip_check_nni and
// hyphy_hip_nni_scores refuse by it (nni_moves_error).
inline const char *nni_move_error(int64_t L, int64_t I, const int64_t *parents, int64_t x, int64_t y) {
  const int64_t root = L + I - 1;
  if (x < 0 || x >= root) return "x is not the code of a branch (the root has none)";
  if (y < 0 || y >= root) return "y is not the code of a branch (the root has none)";
  const int64_t c = L + parents[x];
  if (c == root) return "the parent of x is the root";
  if (y == c) return "y is the parent of x";
  if (parents[y] != parents[c]) return "y is not a sibling of the parent of x";
  return nullptr;
}

// "" when every pair of moves [n][2] is a move, else the first that is not: "move t (x, y): what is wrong with it"
inline std::string nni_moves_error(int64_t L, int64_t I, const int64_t *parents, int64_t n, const int64_t *moves) {
  for (int64_t t = 0; t < n; t++)
    if (const char *why = nni_move_error(L, I, parents, moves[2 * t], moves[2 * t + 1]))
      return "move " + std::to_string(t) + " (" + std::to_string(moves[2 * t]) + ", " + std::to_string(moves[2 * t + 1]) + "): " + why;
  return "";
}

// Every move in ascending (c, y, x), as pairs x, y.  The loops only propose — for every internal node c, the root included, every
// child of its parent (c itself included; below the root: the root's children) against every child x of c — and keep what
// nni_move_error admits: a pair the rule admits has y among the children of parent(parent(x)), so nothing is left out.
inline std::vector<int64_t> plan_nni_moves(int64_t L, int64_t I, const int64_t *parents) {
  const std::vector<std::vector<int>> ch = nni_children(L, I, parents);
  std::vector<int64_t> out;
  for (int64_t ci = 0; ci < I; ci++)
    for (int y : ch[(size_t)(parents[L + ci] >= 0 ? parents[L + ci] : ci)])
      for (int x : ch[(size_t)ci])
        if (!nni_move_error(L, I, parents, x, y)) out.push_back(x), out.push_back(y);
  return out;
}

// Per request t three entries of four words (the program's child entry: 1, node code, internal index or -1, 0):
//   3t      the entry of x
//   3t + 1  the entry of y
//   3t + 2  p's internal index or -1 when p is the root, first word of the request's list in `others`, the other children of c
//           (all but x), the other children of p (all but c and y)
// `others`: node codes, the other children of c and then those of p, request after request.
struct NniTables {
  std::vector<int32_t> entries;  // [n][3][4]
  std::vector<int32_t> others;
  std::vector<int64_t> branch;   // [n] c
};
inline NniTables plan_nni_tables(int64_t L, int64_t I, const int64_t *parents, const std::vector<std::vector<int>> &children, int64_t n,
                                 const int64_t *moves) {
  NniTables t;
  t.entries.resize((size_t)n * 12);
  t.branch.resize((size_t)n);
  for (int64_t k = 0; k < n; k++) {
    const int64_t x = moves[2 * k], y = moves[2 * k + 1], ci = parents[x], pi = parents[L + ci];
    int32_t *e = &t.entries[(size_t)k * 12];
    e[0] = 1, e[1] = (int32_t)x, e[2] = x >= L ? (int32_t)(x - L) : -1, e[3] = 0;
    e[4] = 1, e[5] = (int32_t)y, e[6] = y >= L ? (int32_t)(y - L) : -1, e[7] = 0;
    e[8] = pi == I - 1 ? -1 : (int32_t)pi, e[9] = (int32_t)t.others.size(), e[10] = 0, e[11] = 0;
    for (int k2 : children[(size_t)ci])
      if (k2 != x) t.others.push_back(k2), e[10]++;
    for (int k2 : children[(size_t)pi])
      if (k2 != L + ci && k2 != y) t.others.push_back(k2), e[11]++;
    t.branch[(size_t)k] = L + ci;
  }
  return t;
}

}  // namespace hyhip
