// The host-only plan of subtree repeats (repeats_plan.h): no partition, no device call, no switch, no output.
#include <functional>
#include <unordered_map>

#include "repeats_plan.h"

namespace hyhip {

namespace {

// class ids of the pairs (a[s], b[s]) in order of first occurrence
int pair_classes(const std::vector<int> &a, const std::vector<int> &b, std::vector<int> &out) {
  std::unordered_map<uint64_t, int> seen;
  seen.reserve(a.size() / 2 + 16);
  out.resize(a.size());
  int n = 0;
  for (size_t s = 0; s < a.size(); s++) {
    const uint64_t key = ((uint64_t)(uint32_t)a[s] << 32) | (uint32_t)b[s];
    auto it = seen.find(key);
    if (it == seen.end()) it = seen.emplace(key, n++).first;
    out[s] = it->second;
  }
  return n;
}

// ... of a single column
int column_classes(const std::vector<int> &a, std::vector<int> &out) {
  std::unordered_map<int, int> seen;
  out.resize(a.size());
  int n = 0;
  for (size_t s = 0; s < a.size(); s++) {
    auto it = seen.find(a[s]);
    if (it == seen.end()) it = seen.emplace(a[s], n++).first;
    out[s] = it->second;
  }
  return n;
}

// class of every (internal node, pattern) bottom-up — the id of the tuple of the children's classes (a leaf: its code, ambiguity codes
// included) in order of first occurrence — and the number of classes per node
void count_classes(const std::vector<std::vector<int>> &children, int L, int I, const std::vector<int16_t> &codes, size_t SP,
                   std::vector<std::vector<int>> &cls, std::vector<int> &U) {
  cls.assign(I, std::vector<int>());
  U.assign(I, 0);
  std::vector<int> col(SP), tmp;
  for (int n = 0; n < I; n++) {
    std::vector<int> run;
    bool first = true;
    for (int c : children[n]) {
      const std::vector<int> *cc;
      if (c < L) {
        for (size_t j = 0; j < SP; j++) col[j] = (int)codes[(size_t)c * SP + j];
        cc = &col;
      } else {
        cc = &cls[c - L];
      }
      if (first) {
        run = *cc;
        first = false;
      } else {
        pair_classes(run, *cc, tmp);
        run.swap(tmp);
      }
    }
    U[n] = column_classes(run, cls[n]);
  }
}

// the compressed set: internal nodes (never the root) with at most theta x patterns classes on every shard, all of whose internal
// children are compressed too
std::vector<char> compressed_set(const std::vector<std::vector<int>> &children, int L, int I, const std::vector<std::vector<int>> &U,
                                 const std::vector<int> &S_pad, double theta) {
  std::vector<char> comp(I, 0);
  for (int n = 0; n < I - 1; n++) {
    bool ok = true;
    for (size_t k = 0; k < U.size(); k++)
      if ((double)U[k][n] > theta * S_pad[k] || U[k][n] > 32000) ok = false;
    for (int c : children[n])
      if (c >= L && !comp[c - L]) ok = false;
    if ((int)children[n].size() > kRepMaxInputs - 8) ok = false;  // (a star: its children's indices would not fit the wave's LDS list)
    comp[n] = ok ? 1 : 0;
  }
  return comp;
}

// ---- admission: the rules that need no class computation ----
std::string admission(const RepPlanInput &in, const RepOptions &opt) {
  if (opt.mode == 0) return "switched off (HYPHY_HIP_REPEATS=0)";
  if (in.S_pad.empty()) return "no shards";
  if (opt.mode < 0 && opt.per_pattern_forced) return "a diagnostic switch forces a per-pattern kernel, instantiation or cut";
  for (int t : in.T)
    if (t != 1) return "a shard runs more than one tile per workgroup";
  // (tiny shards: the workgroup-per-tile kernel keeps the whole tree)
  if (!in.nuc && opt.variant != 1 && opt.mode != 2) return "the shard is small enough for the workgroup-per-tile kernel";
  // 4 states: only on request (HYPHY_HIP_REPEATS=1 / 2).  Measured, it loses: a class row is 36 bytes gathered past the L2 per pattern
  // and generalised leaf, where prune_nuc2_kernel computes a whole node from registers for 16 multiply-adds — gtr_32x50k 35.0 us plain
  // against 16.5 (walks) + 26.0 (trunk of 5 nodes) compressed, gtr_32x1m 123.8 against 14.5 + 238.9
  if (in.nuc && opt.mode < 0) return "4 states compress on request only (HYPHY_HIP_REPEATS=1 / 2)";
  if (in.I < 2) return "fewer than two internal nodes";
  // (before any work: a partition of a few tiles — FEL makes one per site — has nothing to compress, and the class arrays of a
  //  very large one are host memory this analysis should not take: 4 bytes per internal node and pattern)
  // (4 states: a small shard is one launch with exponentials and combine folded in)
  if (opt.mode != 2 && (in.nuc ? in.S_pad[0] < 8192 : in.ntiles[0] < 8)) return "too few patterns on the first shard";
  double cells = 0.;
  for (int sp : in.S_pad) cells += (double)in.I * sp;
  // (2.5e8 cells = 1 GB of transient host memory and a few seconds of hashing inside hyphy_hip_create, before it is known
  //  whether compression pays — 128 taxa x 100 000 codons is 1.3e7; beyond the bound the partition runs plain)
  if (cells > 2.5e8) return "more than 2.5e8 (internal node, pattern) cells: the class computation is not attempted";
  return "";
}

// ---- does it pay?  the edge products of the two forms on the first shard ----
bool pays_mfma(const RepPlanInput &in, const std::vector<char> &comp, const std::vector<int> &U0, double min_gain) {
  double full = 0., rep = 0.;
  for (int n = 0; n < in.I - 1; n++) {
    full += in.S_pad[0];
    rep += comp[n] ? (U0[n] + 15) / 16 * 16 : in.S_pad[0];
  }
  return rep <= (1.0 - min_gain) * full;
}
bool pays_nuc(const RepPlanInput &in, const std::vector<char> &comp, const std::vector<int> &U0) {
  double full = 0., repd = 0.;
  for (int n = 0; n < in.I - 1; n++) {
    full += in.S_pad[0];
    const bool root = comp[n] && !comp[(*in.parents)[in.L + n]];
    repd += comp[n] ? (root ? (double)U0[n] : 0.) : (double)in.S_pad[0];  // (nodes inside a walk cost next to nothing here)
  }
  return repd <= 0.5 * full;
}

// ---- paths (MFMA form) ----
// rho: a path goes on into the heaviest compressed child while that child keeps at least rho of the node's classes.  0: paths
// run to the bottom of the subtree — no table reads a table, one launch, more products (3.4 x those of one table per node at
// 128 x 100 k).  Larger values trade products for hand-offs; a hand-off is a launch boundary (rep_build_items: one launch per
// level).  Where the lower phase is bound by its walks' lengths (a shard of a few hundred tiles: 1.5 walks per wave) rho = 0 wins
// (headline pruning launches 74.5 us, 79.0 at 0.3, 77.0 at 0.6, 83.2 at 2); where it is bound by throughput (128 x 100 k: 6 250
// tiles, eight rounds of walks) the saved products win: 663.6 us at 0, 584.2 at 0.15, 537.7 at 0.3, 549.6 at 0.45, 552.2 at 2.
// In between (64 taxa): 1 250 tiles 110.0 us at 0 against 119.1 at 0.3; 2 500 tiles 173.8 against 169.3 — the default changes at
// 2 048.  (Before the per-level launches, with the ticket protocol: 785 us at 0.6 against 726 at 0.)  HYPHY_HIP_REP_RHO overrides.
// (r06, row-split walks in both phases, pruning launches at 128 x 100 k: 625 us at 0, 537 at 0.15, 501 at 0.3, 489 at 0.5, 485 at 0.6,
//  504 at 0.7, 508 at 1 and 2: the default there moved from 0.3 to 0.5)
struct Paths {
  std::vector<int> heavy;                  // the compressed child a node's path continues into
  std::vector<char> continued;             // the node is inside its parent's path (no table of its own)
  std::vector<char> absorbed;              // a side path's top walked inline by the path it hangs off
  std::vector<std::vector<int>> inline_at; // per path node: the side tops walked inline in front of it
  std::vector<int> chain_of(int top) const {  // bottom first
    std::vector<int> down;
    for (int x = top; x >= 0; x = heavy[x]) down.push_back(x);
    return std::vector<int>(down.rbegin(), down.rend());
  }
};
Paths select_paths(const RepPlanInput &in, const std::vector<char> &comp, const std::vector<int> &U0, double rho, bool inline_chains) {
  const int L = in.L, I = in.I;
  const std::vector<std::vector<int>> &children = *in.children;
  Paths ps;
  ps.heavy.assign(I, -1);
  ps.continued.assign(I, 0);
  ps.absorbed.assign(I, 0);
  ps.inline_at.assign(I, std::vector<int>());
  std::vector<int> path_inputs(I, 0), path_len(I, 0);
  for (int n = 0; n < I; n++) {
    if (!comp[n]) continue;
    int best = -1;
    for (int c : children[n])
      if (c >= L && (best < 0 || U0[c - L] > U0[best])) best = c - L;
    // (a path's inputs are staged in LDS by index: long caterpillars / wide multifurcations are cut into several paths)
    const int own_inputs = (int)children[n].size();
    path_inputs[n] = own_inputs;
    path_len[n] = 1;
    if (best >= 0 && (double)U0[best] >= rho * (double)U0[n] && path_inputs[best] + own_inputs - 1 <= kRepMaxInputs - 8 &&
        path_len[best] < 32 && own_inputs <= kRepMaxInputs / 2) {
      ps.heavy[n] = best;
      ps.continued[best] = 1;
      path_inputs[n] = path_inputs[best] + own_inputs - 1;
      path_len[n] = path_len[best] + 1;
    }
  }
  // Side chains walked inline (latency mode, rho = 0).  A side path whose nodes read leaves only — a cherry, a short caterpillar —
  // hanging off another path is not worth a table of its own: its table would be one more hand-off in the dependency chain of the
  // path that reads it (publish, drain, counter, poll, gather: ~8 us with the item's fixed costs) to save a few products.  Such a
  // chain is walked INSIDE the item of the path it hangs off: the running product is parked in the wave's LDS tile, the chain
  // is walked from ones, and its edge product is multiplied back in (one parking slot: inlined chains do not nest).
  if (!inline_chains) return ps;
  std::vector<char> leafy(I, 0);  // a path top whose whole path reads ordinary leaves / leaf tables only
  for (int n = 0; n < I; n++)
    if (comp[n] && !ps.continued[n]) {
      bool ok = true;
      for (int x : ps.chain_of(n))
        for (int c : children[x])
          if (c >= L && c - L != ps.heavy[x]) ok = false;
      leafy[n] = ok ? 1 : 0;
    }
  // (the path a chain hangs off decides, within what its LDS index list holds)
  for (int n = 0; n < I; n++)
    if (comp[n] && !ps.continued[n]) {
      int n_inputs = 0, n_entries = 0;
      for (int x : ps.chain_of(n)) n_inputs += (int)children[x].size() - (ps.heavy[x] >= 0 ? 1 : 0), n_entries++;
      for (int x : ps.chain_of(n))
        for (int c : children[x]) {
          if (c < L || c - L == ps.heavy[x] || !comp[c - L] || !leafy[c - L]) continue;
          const std::vector<int> side = ps.chain_of(c - L);
          int side_inputs = 0;
          for (int y : side) side_inputs += (int)children[y].size();
          if (n_inputs + side_inputs > kRepMaxInputs - 8 || n_entries + (int)side.size() > 40) continue;
          n_inputs += side_inputs - 1;  // (the chain's table would have been one input)
          n_entries += (int)side.size();
          ps.absorbed[c - L] = 1;
          ps.inline_at[x].push_back(c - L);
        }
    }
  return ps;
}

// ---- descriptors, MFMA form: leaves with ambiguity codes first (level 0), then the paths, inputs before the paths that read them ----
void build_descriptors_mfma(const RepPlanInput &in, const Paths &ps, RepPlan &plan) {
  const int L = in.L, I = in.I;
  plan.rep_nodes.clear();
  plan.rep_desc_of.assign((size_t)L + I, -1);
  for (int l = 0; l < L; l++)
    if ((*in.leaf_has_ambig)[l]) {
      RepNode rn;
      rn.node = l;
      rn.level = 0;
      plan.rep_desc_of[l] = (int)plan.rep_nodes.size();
      plan.rep_nodes.push_back(rn);
    }
  for (int n = 0; n < I; n++)
    if (plan.comp[n] && !ps.continued[n] && !ps.absorbed[n]) {  // a path's top (ascending: every input's top comes first)
      RepNode rn;
      rn.node = L + n;
      rn.level = 0;
      auto add_node = [&](int x, int skip_child, int flags) {
        rn.path.push_back(L + x);
        rn.flags.push_back(flags);
        rn.kids.push_back(std::vector<int>());
        rn.kid_desc.push_back(std::vector<int>());
        for (int c : (*in.children)[x]) {
          if (c == skip_child) continue;  // (comes through the registers / was walked inline just before)
          if (c >= L && ps.absorbed[c - L]) continue;
          rn.kids.back().push_back(c);
          const int d = plan.rep_desc_of[c];
          rn.kid_desc.back().push_back(d);
          if (d >= 0) rn.level = std::max(rn.level, plan.rep_nodes[d].level + 1);
        }
      };
      const std::vector<int> main_path = ps.chain_of(n);
      for (size_t k = 0; k < main_path.size(); k++) {
        const int x = main_path[k];
        for (int c : ps.inline_at[x]) {
          const std::vector<int> side = ps.chain_of(c);
          for (size_t j = 0; j < side.size(); j++)
            add_node(side[j], j > 0 ? L + side[j - 1] : -1, (j == 0 ? 1 : 0) | (j + 1 == side.size() ? 2 : 0));
        }
        add_node(x, k > 0 ? L + main_path[k - 1] : -1, 0);
      }
      plan.rep_desc_of[L + n] = (int)plan.rep_nodes.size();
      plan.rep_nodes.push_back(rn);
    }
}

// ---- descriptors, 4 states (class_table_nuc_kernel): one per compressed subtree ROOT, walked whole on an LDS stack ----
// internal children (internal indices) of every node in visiting order — heaviest stack need first — and, in `need`, the stack slots
// a subtree's walk takes under that order
std::vector<std::vector<int>> nuc_visit_order(const RepPlanInput &in, std::vector<int> &need) {
  need.assign(in.I, 1);
  std::vector<std::vector<int>> order(in.I);
  for (int n = 0; n < in.I; n++) {
    for (int c : (*in.children)[n])
      if (c >= in.L) order[n].push_back(c - in.L);
    std::stable_sort(order[n].begin(), order[n].end(), [&](int x, int y) { return need[x] > need[y]; });
    for (size_t j = 0; j < order[n].size(); j++) need[n] = std::max(need[n], (int)j + need[order[n][j]]);
  }
  return order;
}
void build_descriptors_nuc(const RepPlanInput &in, const std::vector<std::vector<int>> &order, RepPlan &plan) {
  const int L = in.L, I = in.I;
  plan.rep_nodes.clear();
  plan.rep_desc_of.assign((size_t)L + I, -1);
  for (int n = 0; n < I; n++) {
    if (!plan.comp[n] || plan.comp[(*in.parents)[L + n]]) continue;  // roots only
    RepNode rn;
    rn.node = L + n;
    rn.level = 0;
    // post-order over the subtree, heaviest child first
    std::vector<std::pair<int, size_t>> stack(1, std::make_pair(n, (size_t)0));
    while (!stack.empty()) {
      std::pair<int, size_t> &t = stack.back();
      if (t.second < order[t.first].size()) {
        const int c = order[t.first][t.second++];
        stack.push_back(std::make_pair(c, (size_t)0));
      } else {
        const int x = t.first;
        rn.path.push_back(L + x);
        rn.flags.push_back((int)order[x].size());  // (4 states: finished children this node takes off the stack)
        rn.kids.push_back(std::vector<int>());
        rn.kid_desc.push_back(std::vector<int>());
        for (int c : (*in.children)[x])
          if (c < L) {
            rn.kids.back().push_back(c);
            rn.kid_desc.back().push_back(-1);
          }
        stack.pop_back();
      }
    }
    plan.rep_desc_of[L + n] = (int)plan.rep_nodes.size();
    plan.rep_nodes.push_back(rn);
  }
}

// ---- the trunk view: the nodes that are not compressed over generalised leaves (ordinary leaves below them, compressed roots) ----
// `leaf_has_ambig` given (4 states): ambiguity codes stay with the trunk kernel's own resolution-vector path; nullptr (MFMA form):
// they live in class tables, and no leaf of the view takes that path
RepView build_trunk_view(const std::vector<std::vector<int>> &children, const std::vector<int64_t> &parents, int L, const std::vector<char> &comp,
                         const std::vector<char> *leaf_has_ambig, std::vector<int> &leaf_nodes) {
  const int I = (int)comp.size();
  RepView v;
  std::vector<int> vint(I, -1);  // view-internal index of a trunk node
  for (int n = 0; n < I; n++)
    if (!comp[n]) vint[n] = v.I++;
  leaf_nodes.clear();
  std::vector<int> vleaf((size_t)L + I, -1);
  for (int n = 0; n < I; n++)
    if (!comp[n])
      for (int c : children[n])
        if (c < L || comp[c - L]) {
          vleaf[c] = (int)leaf_nodes.size();
          leaf_nodes.push_back(c);
        }
  v.L = (int)leaf_nodes.size();
  v.parents.assign((size_t)v.L + v.I, -1);
  v.children.assign(v.I, std::vector<int>());
  v.slot.assign((size_t)v.L + v.I, 0);
  v.leaf_has_ambig.assign(v.L, 0);
  for (int n = 0; n < I; n++) {
    if (comp[n]) continue;
    v.slot[v.L + vint[n]] = L + n;
    const int64_t par = parents[L + n];
    v.parents[v.L + vint[n]] = par < 0 ? -1 : vint[par];
    for (int c : children[n]) {
      if (c < L || comp[c - L]) {
        v.children[vint[n]].push_back(vleaf[c]);
        v.parents[vleaf[c]] = vint[n];
        v.slot[vleaf[c]] = c;
        if (c < L && leaf_has_ambig) v.leaf_has_ambig[vleaf[c]] = (*leaf_has_ambig)[c];
      } else {
        v.children[vint[n]].push_back(v.L + vint[c - L]);
      }
    }
    std::sort(v.children[vint[n]].begin(), v.children[vint[n]].end());
  }
  return v;
}

// ---- per-shard tables ----
// table d's rows behind those of the tables before it; returns the representative pattern of every row (padding rows repeat class 0)
std::vector<int> add_table(RepShardTables &t, int d, int U, const std::vector<int> &cl) {
  RepTable &tb = t.tabs[d];
  tb.U = U;
  tb.rows = (U + 15) / 16 * 16;
  tb.row0 = t.rows;
  t.rows += tb.rows;
  std::vector<int> first_pat(tb.rows, -1);
  for (size_t j = 0; j < cl.size(); j++)
    if (first_pat[cl[j]] < 0) first_pat[cl[j]] = (int)j;
  for (int u = U; u < tb.rows; u++) first_pat[u] = first_pat[0];
  return first_pat;
}
bool addressable(RepShardTables &t) {
  if (t.maps.size() > 0x7fffffffull || t.rows > 0x7fffffffll) t.declined = "a shard's index maps or table rows exceed 2^31 entries";
  return t.declined.empty();
}
// the trunk's leaf table (state codes / class ids; tile-major [tile][view leaf][16] or row-major [view leaf][pattern]) and where each
// view leaf gathers from
void leaf_table(const RepPlan &plan, size_t k, const std::vector<int16_t> &codes, size_t SP, int L, const std::vector<std::vector<int>> &leaf_cls,
                bool tile_major, RepShardTables &t) {
  const size_t VL = (size_t)plan.view.L;
  t.ct.assign(VL * SP, 0);
  t.lt.resize(VL);
  for (size_t vl = 0; vl < VL; vl++) {
    const int c = plan.leaf_nodes[vl], d = plan.rep_desc_of[c];
    t.lt[vl] = d >= 0 ? make_int2((int)t.tabs[d].row0, (int)t.tabs[d].row0) : make_int2(-1, c);
    const int *cl = d < 0 ? nullptr : (c < L ? leaf_cls[c].data() : plan.cls[k][c - L].data());
    const int16_t *code = codes.data() + (size_t)c * SP;
    for (size_t j = 0; j < SP; j++)
      t.ct[tile_major ? ((j >> 4) * VL + vl) * 16 + (j & 15) : vl * SP + j] = (int16_t)(cl ? cl[j] : (int)code[j]);
  }
}

RepShardTables shard_tables_mfma(const RepPlanInput &in, const RepPlan &plan, size_t k, const std::vector<int16_t> &codes) {
  const int L = in.L, ND = (int)plan.rep_nodes.size();
  const size_t SP = (size_t)in.S_pad[k];
  RepShardTables t;
  t.tabs.assign(ND, RepTable());
  std::vector<std::vector<int>> leaf_cls(L);  // classes of the leaves that own a table
  for (int d = 0; d < ND; d++) {
    const RepNode &rn = plan.rep_nodes[d];
    RepTable &tb = t.tabs[d];
    if (rn.node < L) {  // the code of every class
      std::vector<int> col(SP);
      for (size_t j = 0; j < SP; j++) col[j] = (int)codes[(size_t)rn.node * SP + j];
      const int U = column_classes(col, leaf_cls[rn.node]);
      const std::vector<int> first_pat = add_table(t, d, U, leaf_cls[rn.node]);
      tb.map0.push_back((int64_t)t.maps.size());
      for (int u = 0; u < tb.rows; u++) t.maps.push_back((int32_t)codes[(size_t)rn.node * SP + first_pat[u]]);
      continue;
    }
    const std::vector<int> first_pat = add_table(t, d, plan.U[k][rn.node - L], plan.cls[k][rn.node - L]);
    for (size_t x = 0; x < rn.path.size(); x++)
      for (size_t j = 0; j < rn.kids[x].size(); j++) {
        tb.map0.push_back((int64_t)t.maps.size());
        const int c = rn.kids[x][j], cd = rn.kid_desc[x][j];
        for (int u = 0; u < tb.rows; u++) {
          const int pat = first_pat[u];  // (a class of the top node fixes the class of everything below it)
          int32_t idx;
          if (cd < 0) idx = (int32_t)codes[(size_t)c * SP + pat];  // ordinary leaf: its state
          else if (c < L) idx = (int32_t)leaf_cls[c][pat];         // leaf with a table: class of its code
          else idx = (int32_t)plan.cls[k][c - L][pat];             // compressed child: its class
          t.maps.push_back(idx);
        }
      }
  }
  if (!addressable(t)) return t;
  t.desc.assign((size_t)2 * ND, make_int4(0, 0, 0, 0));
  for (int d = 0; d < ND; d++) {
    const RepNode &rn = plan.rep_nodes[d];
    const RepTable &tb = t.tabs[d];
    const int kind = rn.node < L ? 1 : 0;
    const int node0 = (int)t.desc.size();
    t.desc[2 * d] = make_int4((int)tb.row0, tb.U, (int)rn.path.size() | (kind << 16), node0);
    int n_in = 0;
    for (const std::vector<int> &kk : rn.kids) n_in += (int)kk.size();
    t.desc[2 * d + 1] = make_int4(tb.map0.empty() ? 0 : (int)tb.map0[0], tb.rows / 16, rn.level, kind ? rn.node : n_in);
    t.desc.resize(t.desc.size() + rn.path.size());
    size_t mi = 0;
    for (size_t x = 0; x < rn.path.size(); x++) {
      t.desc[node0 + x] = make_int4(rn.path[x], (int)rn.kids[x].size(), (int)t.desc.size(), rn.flags[x]);
      for (size_t j = 0; j < rn.kids[x].size(); j++, mi++) {
        const int cd = rn.kid_desc[x][j];
        t.desc.push_back(make_int4(cd >= 0 ? (int)t.tabs[cd].row0 : -1, rn.kids[x][j], (int)tb.map0[mi],
                                   cd >= 0 ? (cd | ((t.tabs[cd].rows / 16) << 16)) : -1));
      }
    }
  }
  leaf_table(plan, k, codes, SP, L, leaf_cls, true, t);
  return t;
}

RepShardTables shard_tables_nuc(const RepPlanInput &in, const RepPlan &plan, size_t k, const std::vector<int16_t> &codes) {
  const int L = in.L, ND = (int)plan.rep_nodes.size();
  const size_t SP = (size_t)in.S_pad[k];
  RepShardTables t;
  t.tabs.assign(ND, RepTable());
  t.desc.assign((size_t)2 * ND, make_int4(0, 0, 0, 0));
  for (int d = 0; d < ND; d++) {
    const RepNode &rn = plan.rep_nodes[d];
    RepTable &tb = t.tabs[d];
    const std::vector<int> first_pat = add_table(t, d, plan.U[k][rn.node - L], plan.cls[k][rn.node - L]);
    const int64_t map0 = (int64_t)t.maps.size();
    int n_in = 0;
    for (size_t x = 0; x < rn.path.size(); x++)
      for (int c : rn.kids[x]) {
        for (int u = 0; u < tb.rows; u++) t.maps.push_back((int32_t)codes[(size_t)c * SP + first_pat[u]]);
        n_in++;
      }
    tb.map0.push_back(map0);
    const int node0 = (int)t.desc.size();
    t.desc[2 * d] = make_int4((int)tb.row0, tb.U, (int)rn.path.size(), node0);
    t.desc[2 * d + 1] = make_int4((int)map0, tb.rows, 0, n_in);
    t.desc.resize(t.desc.size() + rn.path.size());
    for (size_t x = 0; x < rn.path.size(); x++) {
      t.desc[node0 + x] = make_int4(rn.path[x], (int)rn.kids[x].size(), (int)t.desc.size(), rn.flags[x]);
      for (int c : rn.kids[x]) t.desc.push_back(make_int4(-1, c, 0, -1));
    }
  }
  if (!addressable(t)) return t;
  leaf_table(plan, k, codes, SP, L, std::vector<std::vector<int>>(), false, t);
  return t;
}

}  // namespace

RepShardTables plan_shard_tables(const RepPlanInput &in, const RepPlan &plan, size_t k, const std::vector<int16_t> &codes_k) {
  return in.nuc ? shard_tables_nuc(in, plan, k, codes_k) : shard_tables_mfma(in, plan, k, codes_k);
}

WalkPlan plan_trunk_walk(const RepView &v) {
  WalkPlan wp;
  std::vector<int> weight(v.I, 1);
  for (int i = 0; i < v.I; i++)  // (children before parents)
    for (int c : v.children[i])
      if (c >= v.L) weight[i] += weight[c - v.L];
  std::vector<WalkPlan::Node> &nodes = wp.nodes;
  std::vector<int> &inputs = wp.inputs;
  int depth = 0;
  auto leaf_inputs = [&](int i, int &n_in, int &in0) {
    n_in = 0, in0 = (int)inputs.size();
    for (int c : v.children[i])
      if (c < v.L) inputs.push_back(c), n_in++;
  };
  std::function<void(int)> emit = [&](int i) {
    std::vector<int> kids;
    for (int c : v.children[i])
      if (c >= v.L) kids.push_back(c - v.L);
    std::stable_sort(kids.begin(), kids.end(), [&](int x, int y) { return weight[x] > weight[y]; });
    for (size_t j = 0; j < kids.size(); j++) {
      const size_t first = nodes.size();
      if (j > 0) wp.max_depth = std::max(wp.max_depth, ++depth);
      emit(kids[j]);
      if (j > 0) {
        nodes[first].flags |= 1;
        nodes.back().flags |= 2;
        depth--;
      }
    }
    int n_in, in0;
    leaf_inputs(i, n_in, in0);
    nodes.push_back(WalkPlan::Node{i, n_in, in0, 0});
  };
  auto emit_chain = [&](const std::vector<int> &subs, bool root_leaves, std::vector<int> &range) {
    range.push_back((int)nodes.size());
    for (size_t j = 0; j < subs.size(); j++) {
      const size_t first = nodes.size();
      if (j > 0) wp.max_depth = std::max(wp.max_depth, ++depth);
      emit(subs[j]);
      if (j > 0) {
        nodes[first].flags |= 1;
        nodes.back().flags |= 2;
        depth--;
      }
    }
    int n_in = 0, in0 = (int)inputs.size();
    if (root_leaves) leaf_inputs(v.I - 1, n_in, in0);
    nodes.push_back(WalkPlan::Node{-1, n_in, in0, 0});
    range.push_back((int)nodes.size());
  };
  std::vector<int> subs;
  for (int c : v.children[v.I - 1])
    if (c >= v.L) subs.push_back(c - v.L);
  std::stable_sort(subs.begin(), subs.end(), [&](int x, int y) { return weight[x] > weight[y]; });
  emit_chain(subs, true, wp.one_range);
  if (subs.size() >= 2) {
    std::vector<int> c0, c1;
    int w0 = 0, w1 = 0;
    for (int sb : subs)
      if (w0 <= w1) c0.push_back(sb), w0 += weight[sb];
      else c1.push_back(sb), w1 += weight[sb];
    if (std::min(w0, w1) >= 2 && 4 * std::min(w0, w1) >= std::max(w0, w1)) {  // (a second chain of a node or two is not worth its workgroup)
      emit_chain(c0, true, wp.two_range);
      emit_chain(c1, false, wp.two_range);
      wp.two = true;
    }
  }
  return wp;
}

// The walk's program as trunk_walk_kernel reads it: [0] header, one-chain form (1 + 1 words), two-chain form (1 + 2 words), node words
// (matrix slot or -1, inputs, first input word, flags), input words (view leaf, and the shard's two leaf-table words for it)
std::vector<int4> encode_walk_program(const WalkPlan &wp, const RepView &v, const std::vector<int2> &lt) {
  const std::vector<WalkPlan::Node> &nodes = wp.nodes;
  const std::vector<int> &one_range = wp.one_range, &two_range = wp.two_range;
  const int form1 = 1, form2 = wp.two ? 3 : 0, node_base = wp.two ? 6 : 3, in_base = node_base + (int)nodes.size();
  std::vector<int4> prog((size_t)in_base + wp.inputs.size());
  prog[0] = make_int4(form1, form2, wp.max_depth, (int)prog.size());
  prog[form1] = make_int4(1, 0, 0, 0);
  prog[form1 + 1] = make_int4(node_base + one_range[0], one_range[1] - one_range[0], 0, 0);
  if (wp.two) {
    prog[form2] = make_int4(2, 0, 0, 0);
    const int n0 = two_range[1] - two_range[0], n1 = two_range[3] - two_range[2];
    // (.z: wave priority — the longer chain's instructions first wherever the two share a SIMD: 59.5 against 60.4 us of pruning
    //  launches at the headline; the same by walk length in the lower phase: no difference, not kept)
    prog[form2 + 1] = make_int4(node_base + two_range[0], n0, n0 > n1 ? 3 : 0, 0);
    prog[form2 + 2] = make_int4(node_base + two_range[2], n1, n1 > n0 ? 3 : 0, 0);
  }
  for (size_t k = 0; k < nodes.size(); k++)
    prog[node_base + k] = make_int4(nodes[k].node < 0 ? -1 : v.slot[v.L + nodes[k].node], nodes[k].n_in, in_base + nodes[k].in0, nodes[k].flags);
  for (size_t k = 0; k < wp.inputs.size(); k++) prog[in_base + k] = make_int4(wp.inputs[k], lt[wp.inputs[k]].x, lt[wp.inputs[k]].y, 0);
  return prog;
}

// Everything that is the same on every shard: the compressed set, the descriptors, the trunk view, the walk.
RepPlan plan_repeat_set(const RepPlanInput &in, const RepOptions &opt, const std::vector<std::vector<int16_t>> &codes) {
  RepPlan plan;
  plan.declined = admission(in, opt);
  if (!plan.declined.empty()) return plan;
  const int L = in.L, I = in.I;
  const size_t nsh = in.S_pad.size();
  const bool forced = opt.mode == 2;
  // theta: the share of the patterns below which a node's classes are worth a table.  0.3-0.4 is the flat optimum of the headline
  // alignment (0.2: 100 us of pruning launches, 0.3: 89, 0.4: 89, 0.5: 101, 0.7: 106): above it the walks of the lower phase get long
  // and few, below it the trunk keeps nodes that repeat heavily.  4 states: 0.9 (a walk costs 16 multiply-adds per node: everything
  // that repeats at all is worth a table)
  plan.theta = in.nuc && !opt.theta_given ? 0.9 : opt.theta;
  plan.cls.resize(nsh);
  plan.U.assign(nsh, std::vector<int>(I, 0));
  for (size_t k = 0; k < nsh; k++) count_classes(*in.children, L, I, codes[k], (size_t)in.S_pad[k], plan.cls[k], plan.U[k]);
  // the same set on every shard (one schedule serves them all)
  plan.comp = compressed_set(*in.children, L, I, plan.U, in.S_pad, plan.theta);
  for (size_t k = 0; k < nsh; k++)  // (only the classes of compressed nodes are read again: tables, maps, the trunk's leaf table)
    for (int n = 0; n < I; n++)
      if (!plan.comp[n]) std::vector<int>().swap(plan.cls[k][n]);
  if (in.nuc) {
    std::vector<int> need;
    const std::vector<std::vector<int>> order = nuc_visit_order(in, need);
    for (int n = I - 1; n >= 0; n--) {  // (parents first: a subtree too deep for the stack hands the role of root to its children)
      const int64_t par = (*in.parents)[L + n];
      if (plan.comp[n] && (par < 0 || !plan.comp[par]) && need[n] > kNucStack) plan.comp[n] = 0;
    }
    if (!forced && !pays_nuc(in, plan.comp, plan.U[0])) { plan.declined = "the walks would cost more than half of the plain form"; return plan; }
    build_descriptors_nuc(in, order, plan);
  } else {
    if (!forced && !pays_mfma(in, plan.comp, plan.U[0], opt.min_gain))
      { plan.declined = "the class tables save less than HYPHY_HIP_REP_MIN_GAIN of the edge products"; return plan; }
    plan.rho = std::isnan(opt.rho) ? (in.ntiles[0] >= 2048 ? 0.5 : 0.) : opt.rho;
    const bool inline_chains = opt.inline_chains >= 0 ? opt.inline_chains != 0 : plan.rho == 0.;
    build_descriptors_mfma(in, select_paths(in, plan.comp, plan.U[0], plan.rho, inline_chains), plan);
  }
  if (plan.rep_nodes.empty()) { plan.declined = "no node repeats enough to be compressed"; return plan; }
  if (plan.rep_nodes.size() > 65535) { plan.declined = "more than 65535 class tables"; return plan; }
  plan.view = build_trunk_view(*in.children, *in.parents, L, plan.comp, in.nuc ? in.leaf_has_ambig : nullptr, plan.leaf_nodes);
  if (plan.view.L > 65535 || plan.view.L < 1) { plan.declined = "the trunk has more than 65535 generalised leaves"; return plan; }
  if (!in.nuc && in.NW >= 2 && plan.view.L <= 1024) {
    plan.walk = plan_trunk_walk(plan.view);
    plan.has_walk = plan.walk.max_depth <= kWalkDepth && plan.walk.nodes.size() < 4096 && !plan.walk.inputs.empty();
  }
  return plan;
}

}  // namespace hyhip

// ---- host-only inspection entries (include/hyphy_hip.h) and their marshalling ----
using namespace hyhip;

namespace {
// the caller's tree (flat_parents[n] = internal index of n's parent, children before parents, the root last) as the planner takes it
bool tree_from_flat(int64_t L, int64_t I, const int64_t *flat_parents, std::vector<int64_t> &parents, std::vector<std::vector<int>> &children) {
  parents.assign((size_t)(L + I), -1);
  children.assign((size_t)I, std::vector<int>());
  for (int64_t n = 0; n < L + I - 1; n++) {
    const int64_t par = flat_parents[n];
    if (par < 0 || par >= I || (n >= L && par <= n - L)) return false;
    parents[(size_t)n] = par;
    children[(size_t)par].push_back((int)n);
  }
  return true;
}
template <typename T>
void put_list(std::vector<int64_t> &o, const std::vector<T> &v) {
  o.push_back((int64_t)v.size());
  for (const T &x : v) o.push_back((int64_t)x);
}
void put_words(std::vector<int64_t> &o, const std::vector<int4> &v) {
  o.push_back((int64_t)v.size());
  for (const int4 &w : v) o.push_back(w.x), o.push_back(w.y), o.push_back(w.z), o.push_back(w.w);
}
}  // namespace

extern "C" {

/* Host-only (no device needed): what hyphy_hip_create decides about subtree repeats from the topology and the leaf table alone.
 * classes_out[I]: classes of every internal node over the S patterns as given (no padding, one shard); compressed_out[I]: 1 where
 * the node's subtree is evaluated per class (theta <= 0: the library's default).  Returns the edge products a full pass executes
 * with one table per compressed node (sum of their classes + S per trunk edge), < 0 on bad arguments. */
/* Host-only: the walk program of a trunk given as a tree over generalised leaves (node codes 0 .. L - 1: leaves, L + i: internal node
 * i, children before parents, the root last; parents[c] = node code of c's parent, the root's entry is ignored).
 * out: [nodes, inputs, stack depth, two chains?, first / end node of the one-chain form, of chain 0, of chain 1], then per node
 * (internal index or -1, leaf children, first input, flags), then the inputs (leaf codes).  Returns the words written, < 0: cap too small. */
int64_t hyphy_hip_plan_trunk_walk(int64_t L, int64_t I, const int64_t *parents, int64_t *out, int64_t cap) {
  if (L < 1 || I < 1 || !parents || !out) return -1;
  RepView v;
  v.L = (int)L, v.I = (int)I;
  v.children.assign((size_t)I, std::vector<int>());
  for (int64_t c = 0; c < L + I - 1; c++) {
    if (parents[c] < L || parents[c] >= L + I) return -1;
    v.children[(size_t)(parents[c] - L)].push_back((int)c);
  }
  const WalkPlan wp = plan_trunk_walk(v);
  const int64_t need = 10 + 4 * (int64_t)wp.nodes.size() + (int64_t)wp.inputs.size();
  if (need > cap) return -need;
  int64_t *o = out;
  *o++ = (int64_t)wp.nodes.size(), *o++ = (int64_t)wp.inputs.size(), *o++ = wp.max_depth, *o++ = wp.two ? 1 : 0;
  *o++ = wp.one_range[0], *o++ = wp.one_range[1];
  for (int k = 0; k < 4; k++) *o++ = wp.two ? wp.two_range[(size_t)k] : 0;
  for (const auto &n : wp.nodes) *o++ = n.node, *o++ = n.n_in, *o++ = n.in0, *o++ = n.flags;
  for (int x : wp.inputs) *o++ = x;
  return need;
}

int64_t hyphy_hip_plan_repeats(int64_t L, int64_t I, const int64_t *flat_parents, int64_t S, const int64_t *leaf_codes, double theta,
                               int64_t *classes_out, int64_t *compressed_out) {
  if (L < 2 || I < 1 || S < 1 || !flat_parents || !leaf_codes) return -1;
  std::vector<int64_t> parents;
  std::vector<std::vector<int>> children;
  if (!tree_from_flat(L, I, flat_parents, parents, children)) return -1;
  std::vector<int16_t> codes((size_t)L * S);
  for (int64_t k = 0; k < L * S; k++) {
    if (leaf_codes[k] > 32767 || leaf_codes[k] < -32768) return -1;
    codes[(size_t)k] = (int16_t)leaf_codes[k];
  }
  std::vector<std::vector<int>> cls;
  std::vector<std::vector<int>> U(1);
  count_classes(children, (int)L, (int)I, codes, (size_t)S, cls, U[0]);
  const std::vector<char> comp = compressed_set(children, (int)L, (int)I, U, std::vector<int>(1, (int)S), theta > 0. ? theta : 0.35);
  int64_t work = 0;
  for (int64_t n = 0; n < I; n++) {
    if (classes_out) classes_out[n] = U[0][(size_t)n];
    if (compressed_out) compressed_out[n] = comp[(size_t)n];
    if (n < I - 1) work += comp[(size_t)n] ? U[0][(size_t)n] : S;
  }
  return work;
}

int64_t hyphy_hip_plan_repeat_layout(int64_t L, int64_t I, const int64_t *flat_parents, int64_t D, int64_t C, int64_t n_shards,
                                     const int64_t *S_pad, const int64_t *leaf_codes, int64_t mode, double theta, double rho, double min_gain,
                                     int64_t inline_chains, int64_t variant, int64_t *out, int64_t cap, char *reason, int64_t reason_cap) {
  if (L < 2 || I < 1 || D < 2 || C < 1 || n_shards < 1 || !flat_parents || !S_pad || !leaf_codes) return -1;
  RepPlanInput in;
  std::vector<int64_t> parents;
  std::vector<std::vector<int>> children;
  if (!tree_from_flat(L, I, flat_parents, parents, children)) return -1;
  in.L = (int)L, in.I = (int)I, in.parents = &parents, in.children = &children;
  in.nuc = D == 4, in.NW = (int)((D + 15) / 16), in.C = (int)C;
  std::vector<char> ambig((size_t)L, 0);
  in.leaf_has_ambig = &ambig;
  std::vector<std::vector<int16_t>> codes((size_t)n_shards);
  const int64_t *src = leaf_codes;
  for (int64_t k = 0; k < n_shards; k++) {
    const int64_t SP = S_pad[k];
    if (SP < 1 || SP > 0x7fffffff || (!in.nuc && SP % 16)) return -1;
    in.S_pad.push_back((int)SP), in.ntiles.push_back(in.nuc ? 0 : (int)(SP / 16)), in.T.push_back(1);
    codes[(size_t)k].resize((size_t)(L * SP));
    for (int64_t j = 0; j < L * SP; j++) {
      if (src[j] > 32767 || src[j] < -32768) return -1;
      codes[(size_t)k][(size_t)j] = (int16_t)src[j];
      if (src[j] < 0) ambig[(size_t)(j / SP)] = 1;
    }
    src += L * SP;
  }
  RepOptions opt;
  opt.mode = (int)mode;
  opt.theta_given = theta > 0.;
  if (opt.theta_given) opt.theta = theta;
  opt.rho = rho < 0. ? NAN : rho;
  if (min_gain >= 0.) opt.min_gain = min_gain;
  opt.inline_chains = (int)inline_chains;
  opt.variant = (int)variant;
  auto decline = [&](const std::string &why) -> int64_t {
    if (reason && reason_cap > 0) snprintf(reason, (size_t)reason_cap, "%s", why.c_str());
    return 0;
  };
  const RepPlan plan = plan_repeat_set(in, opt, codes);
  if (!plan.declined.empty()) return decline(plan.declined);
  const RepView &v = plan.view;
  std::vector<int64_t> o;
  o.push_back((int64_t)plan.rep_nodes.size()), o.push_back(v.L), o.push_back(v.I), o.push_back(n_shards), o.push_back(plan.has_walk ? 1 : 0);
  put_list(o, plan.comp);
  put_list(o, plan.rep_desc_of);
  for (const RepNode &rn : plan.rep_nodes) {
    o.push_back(rn.node), o.push_back(rn.level);
    put_list(o, rn.path);
    put_list(o, rn.flags);
    for (size_t x = 0; x < rn.path.size(); x++) put_list(o, rn.kids[x]), put_list(o, rn.kid_desc[x]);
  }
  put_list(o, v.parents);
  put_list(o, v.slot);
  put_list(o, v.leaf_has_ambig);
  put_list(o, plan.leaf_nodes);
  for (const std::vector<int> &ch : v.children) put_list(o, ch);
  for (int64_t k = 0; k < n_shards; k++) {
    const RepShardTables t = plan_shard_tables(in, plan, (size_t)k, codes[(size_t)k]);
    if (!t.declined.empty()) return decline(t.declined);
    o.push_back(t.rows);
    for (const RepTable &tb : t.tabs) {
      o.push_back(tb.U), o.push_back(tb.rows), o.push_back(tb.row0);
      put_list(o, tb.map0);
    }
    put_list(o, t.maps);
    put_words(o, t.desc);
    put_list(o, t.ct);
    o.push_back((int64_t)t.lt.size());
    for (const int2 &w : t.lt) o.push_back(w.x), o.push_back(w.y);
    put_words(o, plan.has_walk ? encode_walk_program(plan.walk, v, t.lt) : std::vector<int4>());
  }
  if ((int64_t)o.size() > cap || !out) return -(int64_t)o.size();
  std::copy(o.begin(), o.end(), out);
  return (int64_t)o.size();
}

}  // extern "C"
