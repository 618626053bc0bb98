// Subtree repeats, the host-only plan (repeats_plan.hip): everything hyphy_hip_create decides about the class-compressed form from the
// topology and the leaf tables alone — admission, classes, the compressed set, paths and inlined side chains, descriptors, the trunk
// view, every shard's tables / index maps / descriptor words / leaf table, and the trunk walk's program.  Plain data in, plain data
// out: no partition, no device call, no switch, no output.  rep_setup (repeats.hip) fills RepOptions from the switches, uploads what
// the plan holds and seeds the trunk's mode; hyphy_hip_plan_repeat_layout returns the same words to CPU tests.
#pragma once
#include "partition.h"

namespace hyhip {

constexpr int kRepMaxInputs = 64;  // inputs of a path whose class indices are staged in LDS (longer paths: cut by the host)
constexpr int kNucStack = 8;       // 4 states: finished subtrees a walk holds in LDS (class_table_nuc_kernel)
constexpr int kWalkDepth = 3;      // waiting products of the trunk walk's register stack (trunk_walk_kernel)

using RepView = hyphy_hip_partition::View;
using RepNode = hyphy_hip_partition::RepNode;

// What the switches say, read once at create by rep_setup (hyphy_hip_plan_repeat_layout takes the same values as arguments).
struct RepOptions {
  int mode = -1;                    // REPEATS: -1 not given, 0 never, 1 always, 2 always and past the size rules
  bool per_pattern_forced = false;  // a diagnostic that forces a per-pattern kernel, instantiation or cut is set
  double theta = 0.35;              // REP_THETA
  bool theta_given = false;
  double rho = NAN;                 // REP_RHO; NaN: not given (0 below 2 048 tiles on the first shard, 0.5 from there)
  double min_gain = 0.15;           // REP_MIN_GAIN
  int inline_chains = -1;           // REP_INLINE: -1 not given (inline where rho is 0), 0, 1
  int trunk_kernel = -1;            // TRUNK_KERNEL: -1 not given
  int trunk_walk = -1;              // TRUNK_WALK at create: -1 not given, 1 the walk without asking the tuner, 0 any other value
  bool tune = true;                 // TUNE
  int variant = 0, n_slots = 0, n_slots_wave = 3;  // what the partition's own view starts from
};

struct RepPlanInput {
  int L = 0, I = 0;
  const std::vector<int64_t> *parents = nullptr;            // [L + I] internal index of the parent, the root's < 0
  const std::vector<std::vector<int>> *children = nullptr;  // per internal node, ascending node codes
  const std::vector<char> *leaf_has_ambig = nullptr;        // [L]
  bool nuc = false;
  int NW = 0, C = 1;
  std::vector<int> S_pad, ntiles, T;                        // per shard
};

// The trunk as one post-order walk per tile (trunk_walk_kernel): heaviest internal child first — its chain stays in the running
// product —, every other internal child a chain of its own behind a push (flag 1 on its first walked node, 2 on the child itself).
// Two forms: ONE workgroup per tile walks everything; TWO split the subtrees below the root (longest-processing-time-first); each
// chain ends with a node -1: the root's own leaf children (first chain only) and the hand-over / epilogue.
struct WalkPlan {
  struct Node { int node, n_in, in0, flags; };  // node: view-internal index (-1: the chain's end at the root); in0: first entry of `inputs`
  std::vector<Node> nodes;
  std::vector<int> inputs;                      // view leaves
  std::vector<int> one_range, two_range;        // [first, end) node ranges: the one-chain form; the two chains
  int max_depth = 0;
  bool two = false;
};
WalkPlan plan_trunk_walk(const RepView &v);

struct RepPlan {
  std::string declined;                    // non-empty: why the partition runs plain (nothing below is meaningful then)
  double theta = 0., rho = 0.;             // as used
  std::vector<char> comp;                  // [I] the node's subtree is evaluated per class
  std::vector<RepNode> rep_nodes;          // descriptors, children before parents
  std::vector<int> rep_desc_of;            // [L + I] descriptor of a node's table, -1: none
  RepView view;                            // the trunk over generalised leaves
  std::vector<int> leaf_nodes;             // node code (partition's tree) of every view leaf
  bool has_walk = false;                   // the trunk walk has a program for this trunk
  WalkPlan walk;
  // classes [shard][internal node][pattern] (compressed nodes only) and their counts [shard][internal node]: what the shard tables read
  std::vector<std::vector<std::vector<int>>> cls;
  std::vector<std::vector<int>> U;
};
// `codes[k]`: shard k's leaf table [L][S_pad] in device pattern order (padding patterns included: they are patterns like any other)
RepPlan plan_repeat_set(const RepPlanInput &in, const RepOptions &opt, const std::vector<std::vector<int16_t>> &codes);

// One shard's words exactly as uploaded.  Planned one shard at a time: `maps` and `ct` of a large shard are hundreds of MB.
struct RepShardTables {
  std::string declined;        // non-empty: the shard's tables cannot be addressed (nothing is allocated for it)
  std::vector<RepTable> tabs;  // per descriptor
  int64_t rows = 0;            // table rows over all descriptors
  std::vector<int32_t> maps;   // Shard::rep_map
  std::vector<int4> desc;      // Shard::rep_desc
  std::vector<int16_t> ct;     // Shard::rep_codes_tile
  std::vector<int2> lt;        // Shard::rep_leaf
};
RepShardTables plan_shard_tables(const RepPlanInput &in, const RepPlan &plan, size_t k, const std::vector<int16_t> &codes_k);
std::vector<int4> encode_walk_program(const WalkPlan &wp, const RepView &v, const std::vector<int2> &lt);

}  // namespace hyhip
