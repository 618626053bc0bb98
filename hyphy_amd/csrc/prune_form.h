// Which instantiation of the pruning kernels serves a launch, with what grid, block and LDS: decided from plain numbers, on the host,
// in ONE place.  prune.hip's launchers launch what select_*_form returns, and what the evaluation stages ask before they wire a fused
// combine or fold the exponentials in (prune_fuses_reduce, prune_nuc_fuses_reduce, ...) are fields of the same answer: a stage that
// wired a combine the launched kernel does not carry would leave the host spinning on a record nobody writes.  Host only, free of HIP,
// reads no environment (the caller passes the switches in the key): tests/prune_form_check.cpp walks the whole key space.
#pragma once
#include <stddef.h>

#include <tuple>

#ifndef HYPHY_OCC3
#define HYPHY_OCC3 2  // waves per SIMD the production wave-per-tile instantiations are compiled for
#endif

namespace hyhip {

// wave: prune_wave_kernel<NW, NP, CLDS, TRACE, LB, OCC, PRE, REP>; team: prune_mfma_kernel<NW, T, CLDS, TRACE, ABL, CHAIN, FUSE, REP>;
// nuc: prune_nuc_kernel<PIN, REP>; nuc2: prune_nuc2_kernel<NP, PIN, FOLD, LP>.  none: no instantiation serves the launch.
enum class PruneFamily { none, wave, team, nuc, nuc2 };
struct PruneInst {  // one instantiation; fields its family does not own stay at their defaults
  PruneFamily family = PruneFamily::none;
  int NW = 0, T = 0, NP = 0, OCC = 0, ABL = 0;
  bool CLDS = false, TRACE = false, LB = false, PRE = false, CHAIN = false, FUSE = false, REP = false, PIN = false, FOLD = false, LP = false;
  bool operator==(const PruneInst &o) const {
    return std::tie(family, NW, T, NP, OCC, ABL, CLDS, TRACE, LB, PRE, CHAIN, FUSE, REP, PIN, FOLD, LP) ==
           std::tie(o.family, o.NW, o.T, o.NP, o.OCC, o.ABL, o.CLDS, o.TRACE, o.LB, o.PRE, o.CHAIN, o.FUSE, o.REP, o.PIN, o.FOLD, o.LP);
  }
};
constexpr PruneInst wave_inst(int NW, bool CLDS, int NP, bool TRACE, bool LB, int OCC, bool PRE, bool REP) {
  return PruneInst{PruneFamily::wave, NW, 1, NP, OCC, 0, CLDS, TRACE, LB, PRE, false, false, REP};
}
constexpr PruneInst team_inst(int NW, bool CLDS, int T, bool TRACE, int ABL, bool CHAIN, bool FUSE, bool REP) {
  return PruneInst{PruneFamily::team, NW, T, 0, 0, ABL, CLDS, TRACE, false, false, CHAIN, FUSE, REP};
}
constexpr PruneInst nuc_inst(bool PIN, bool REP) { return PruneInst{PruneFamily::nuc, 0, 0, 0, 0, 0, false, false, false, false, false, false, REP, PIN}; }
constexpr PruneInst nuc2_inst(int NP, bool PIN, bool FOLD, bool LP) {
  return PruneInst{PruneFamily::nuc2, 0, 0, NP, 0, 0, false, false, false, false, false, false, false, PIN, FOLD, LP};
}

// The compiled instantiations, in the argument order of the four functions above: prune.hip builds its launch table from this list
// and from nothing else, the host check reads it as values.
#define HYPHY_EACH_NW_CLDS(X, ...)                                                                               \
  X(1, false, __VA_ARGS__), X(1, true, __VA_ARGS__), X(2, false, __VA_ARGS__), X(2, true, __VA_ARGS__), X(3, false, __VA_ARGS__), \
  X(3, true, __VA_ARGS__), X(4, false, __VA_ARGS__), X(4, true, __VA_ARGS__)
#define HYPHY_PRUNE_FORMS(W, M, N1, N2)                                                                          \
  /* wave, two per SIMD, 0 / 1 / 2 parking slots: ordinary trees, then the trunk of a class-compressed partition */ \
  HYPHY_EACH_NW_CLDS(W, 0, false, false, HYPHY_OCC3, true, false), HYPHY_EACH_NW_CLDS(W, 1, false, false, HYPHY_OCC3, true, false), \
  HYPHY_EACH_NW_CLDS(W, 2, false, false, HYPHY_OCC3, true, false), HYPHY_EACH_NW_CLDS(W, 0, false, false, HYPHY_OCC3, true, true), \
  HYPHY_EACH_NW_CLDS(W, 1, false, false, HYPHY_OCC3, true, true), HYPHY_EACH_NW_CLDS(W, 2, false, false, HYPHY_OCC3, true, true), \
  /* wave, tracing builds (HYPHY_HIP_TIMELINE) */                                                                \
  W(4, true, 1, true, false, HYPHY_OCC3, true, false), W(4, true, 2, true, false, HYPHY_OCC3, true, false),      \
  W(4, true, 1, true, false, HYPHY_OCC3, true, true), W(4, true, 2, true, false, HYPHY_OCC3, true, true),        \
  /* wave, three per SIMD: the node finalised last in LDS, no parking slot; without / with the deposit prefetch */ \
  W(4, true, 0, false, true, 3, false, false), W(4, true, 0, false, true, 3, true, false),                       \
  W(4, true, 0, false, true, 3, false, true), W(4, true, 0, false, true, 3, true, true),                         \
  /* team, level schedules with T = 1 .. 4 tiles per workgroup; tracing builds; chain schedules */               \
  HYPHY_EACH_NW_CLDS(M, 1, false, 0, false, false, false), HYPHY_EACH_NW_CLDS(M, 2, false, 0, false, false, false), \
  HYPHY_EACH_NW_CLDS(M, 3, false, 0, false, false, false), HYPHY_EACH_NW_CLDS(M, 4, false, 0, false, false, false), \
  HYPHY_EACH_NW_CLDS(M, 1, true, 0, false, false, false), HYPHY_EACH_NW_CLDS(M, 1, false, 0, true, false, false), \
  /* team, the fused final combine; the trunk of a class-compressed partition (level and chain schedules each) */ \
  M(4, true, 1, false, 0, false, true, false), M(4, true, 1, false, 0, true, true, false),                       \
  M(4, true, 1, false, 0, false, false, true), M(4, true, 1, false, 0, true, false, true),                       \
  /* team, diagnostic ablation builds (HYPHY_HIP_ABLATE, results invalid) */                                     \
  M(4, true, 1, false, 1, false, false, false), M(4, true, 1, false, 2, false, false, false),                    \
  M(4, true, 1, false, 4, false, false, false), M(4, true, 1, false, 16, false, false, false),                   \
  M(4, true, 1, false, 62, false, false, false), M(4, true, 1, false, 63, false, false, false),                  \
  M(4, true, 1, false, 127, false, false, false),                                                                \
  /* 4 states */                                                                                                 \
  N1(false, false), N1(true, false), N1(false, true),                                                            \
  N2(1, false, false, false), N2(1, true, false, false), N2(2, false, false, false), N2(2, true, false, false),  \
  N2(1, false, true, false), N2(1, true, true, false),                                                           \
  N2(1, false, false, true), N2(1, true, false, true), N2(1, false, true, true), N2(1, true, true, true)
constexpr PruneInst kPruneInsts[] = {HYPHY_PRUNE_FORMS(wave_inst, team_inst, nuc_inst, nuc2_inst)};
constexpr bool is_ablation_build(int v) { return v == 1 || v == 2 || v == 4 || v == 16 || v == 62 || v == 63 || v == 127; }

// ---- 20 to 64 states.  What the decision reads of a PruneArgs and of the environment (prune.hip: prune_key) ----
struct PruneKey {
  int NW = 4, T = 1, variant = 0, wave_variant = 0, n_slots = 2, chain = 0, ablate = 0, ntiles = 0, n_cat = 0, n_prog = 0, L = 0;
  bool codes_in_lds = false, leaf_tab = false, timeline = false, target = false;  // (trunk leaf table, trace buffer, fused-combine target present)
  bool xcd_pad = true;                                                           // HYPHY_HIP_XCD_PAD
};
struct PruneForm {
  PruneInst inst;
  int grid[3] = {0, 0, 0}, block = 0;
  size_t lds = 0;  // dynamic LDS bytes
  int n_wg = 0;    // workgroups that write a partial sum (entries of wg_sum), whatever the grid is padded to
  int disp_T = 0, park = -1;  // PruneDispatch, what hyphy_hip_last_prune_form reports
  const char *label = "";
  bool on_chain = false;
  bool can_fuse = false;    // a fused-combine target would be served: inst.FUSE = target && can_fuse (4 states: inst.LP)
  bool leaf_pairs = false;  // 4 states: the schedule must carry leaf groups of two
};

inline PruneForm select_prune_form(const PruneKey &k) {
  PruneForm f;
  const int NW = (k.NW >= 1 && k.NW <= 3) ? k.NW : 4;
  const bool CLDS = k.codes_in_lds, full = NW == 4 && CLDS;  // (the special builds exist at 49-64 states with the leaf codes in LDS only)
  const int gy = k.n_cat > 0 ? k.n_cat : 1, gz = k.n_prog > 0 ? k.n_prog : 1;
  // Chain grids (tiles, classes, sources): workgroup b runs on XCD b mod 8 and the grid is linearised x-fastest, so with the
  // tile dimension padded to a multiple of 8 (the surplus workgroups retire at once) every chain of a tile — and so every
  // join of its trunk — sits on ONE XCD: deposits and arrival counters are then L2 hits instead of trips to memory.
  const int gx = (k.chain && k.T == 1 && k.xcd_pad && !k.timeline) ? ((k.ntiles + 7) & ~7) : k.ntiles / k.T;
  f.n_wg = k.ntiles / k.T, f.disp_T = 1;
  if (k.variant == 1 && k.T == 1) {  // wave-per-tile kernel: one wave per workgroup
    if (k.chain) f.grid[0] = gx, f.grid[1] = gy, f.grid[2] = gz;   // chains: source-major
    else f.grid[0] = gz, f.grid[1] = gy, f.grid[2] = k.ntiles;     // fragments: tile-major
    f.block = 64, f.lds = CLDS ? (size_t)k.L * 16 * sizeof(short) : 0;
    const bool REP = k.leaf_tab;  // the trunk of a class-compressed partition
    if (k.timeline && full) {     // tracing build
      f.inst = wave_inst(4, true, k.n_slots <= 3 ? 1 : 2, true, false, HYPHY_OCC3, true, REP);
      f.label = REP ? "occ2 trace trunk" : "occ2 trace";
    } else if (full && (k.wave_variant == 2 || k.wave_variant == 3) && k.n_slots <= 2) {
      // three waves per SIMD (the tuner's second stage): finalised node in LDS instead of 32 registers, no parking slot; 2 without,
      // 3 with the deposit prefetch
      f.inst = wave_inst(4, true, 0, false, true, 3, k.wave_variant == 3, REP);
      f.label = k.wave_variant == 2 ? (REP ? "occ3 trunk" : "occ3") : (REP ? "occ3+pre trunk" : "occ3+pre");
    } else {  // production: two waves per SIMD, 0 / 1 / 2 parking slots in LDS (the schedule was compiled for k.n_slots - 2 of them)
      f.inst = wave_inst(NW, CLDS, k.n_slots <= 2 ? 0 : (k.n_slots == 3 ? 1 : 2), false, false, HYPHY_OCC3, true, REP);
      f.label = REP ? "occ2 trunk" : "occ2";
    }
    f.park = f.inst.NP;
    // (no wave instantiation carries the fused combine: at 231 VGPRs the combine's registers push 15 spill instructions into the
    //  main loop — what the fusion saves on a small shard, the spills cost)
    return f;
  }
  f.grid[0] = k.chain ? gx : k.ntiles / k.T, f.grid[1] = gy, f.grid[2] = gz;
  f.block = 64 * NW, f.lds = CLDS ? (size_t)k.L * k.T * 16 * sizeof(short) : 0;
  // the fused final combine (PruneArgs::red_out): 49-64 states with the leaf codes in LDS, one tile per workgroup, production builds
  const bool fuse = full && k.T == 1 && !k.timeline && !k.ablate;
  if (k.leaf_tab) {  // the trunk under the row-split kernel: one form; a skipped launch would leave the trunk stale, so the caller reports it
    if (!(full && k.T == 1)) return f;
    f.inst = team_inst(4, true, 1, false, 0, k.chain != 0, false, true);
    f.label = "trunk", f.on_chain = k.chain != 0;
  } else if (k.variant == 2 && k.chain && k.T == 1) {  // row-split workgroups on a chain schedule
    f.inst = team_inst(NW, CLDS, 1, false, 0, true, k.target && fuse, false);
    f.on_chain = true, f.can_fuse = fuse;
  } else if (k.timeline) {  // tracing build of the kernel, T = 1 only
    f.inst = team_inst(NW, CLDS, 1, true, 0, false, false, false);
    f.label = "trace";
  } else {
    f.disp_T = k.T <= 3 ? k.T : 4;
    f.inst = team_inst(NW, CLDS, f.disp_T, false, (full && k.T == 1 && is_ablation_build(k.ablate)) ? k.ablate : 0, false, k.target && fuse && k.variant == 0, false);
    f.can_fuse = fuse && k.variant == 0;
  }
  return f;
}

// ---- 4 states: prune_nuc_kernel (leaf matrices from memory) and prune_nuc2_kernel (leaf matrices and parking slots in LDS) ----
constexpr int kNucParkSlots = 4;           // LDS parking slots of the 4-state kernels (nodes whose parent is not the next entry)
constexpr size_t kNucLdsCap = 112 * 1024;  // dynamic LDS a prune_nuc2_kernel launch may ask for (NP = 2: 74 KiB of parking + up to 32 KiB of leaf matrices)
struct NucKey {
  int L = 0, S_pad = 0, n_ops = 0, root_inode = 0;
  bool PT = false, leaf_tab = false, pinned = false;  // transposed matrices present, trunk leaf table present, a node's states pinned
  bool folded = false;                                // the evaluation's matrix exponentials ride along
  int nuc = -1, nuc_lp = -1, cus = 256;               // HYPHY_HIP_NUC (0: prune_nuc_kernel, 1 / 2: patterns per thread), HYPHY_HIP_NUC_LP (-1: by size)
};
inline PruneForm select_nuc_form(const NucKey &k) {  // grid (n_wg, 1, 1): one workgroup of 256 threads per entry of wg_sum
  PruneForm f;
  f.block = 256, f.grid[1] = f.grid[2] = 1;
  f.leaf_pairs = k.nuc != 0 && k.L <= 256;  // (prune_nuc2_kernel: the leaf matrices, 128 bytes each, fit LDS)
  if (k.leaf_tab || !f.leaf_pairs || !k.PT) {
    // the trunk of a class-compressed partition (no pinned states in that mode), or a tree too large for the LDS tables
    f.inst = k.leaf_tab ? nuc_inst(false, true) : nuc_inst(k.pinned, false);
    f.grid[0] = f.n_wg = (k.S_pad + 255) / 256;
    return f;
  }
  // (measured: one pattern per thread and four workgroups per CU beat two patterns and two workgroups at every size)
  const int np = (k.nuc == 2 && k.S_pad % 512 == 0) ? 2 : 1;
  const auto lds = [&](bool lp) {
    return (size_t)(lp ? k.L + k.root_inode : k.L) * 16 * sizeof(double) + (size_t)kNucParkSlots * np * 256 * (4 * sizeof(double) + sizeof(int)) +
           (lp ? (size_t)(k.n_ops + 4) * 4 * sizeof(int) : 0);
  };
  // schedule words + every branch's matrix from LDS (LP): shards of at most two workgroups per CU.  The LP builds are the ones
  // that carry the fused final combine (NucArgs::red_out).
  const bool lp = np == 1 && (k.nuc_lp >= 0 ? k.nuc_lp != 0 : k.S_pad / 256 <= 2 * k.cus) && lds(true) <= kNucLdsCap;
  // (np == 2 has no folded build: the exponentials would be dropped.  nuc_may_fold refuses HYPHY_HIP_NUC=2, so no caller asks.)
  f.inst = nuc2_inst(np, k.pinned, k.folded && np == 1, lp);
  f.grid[0] = f.n_wg = k.S_pad / (256 * np), f.lds = lds(lp), f.can_fuse = lp;
  return f;
}
// The caller may fold this evaluation's exponentials into the launch: the selected build takes them, on a shard of at most 512
// workgroups.  (late r03: with the Paterson-Stockmeyer 4 x 4 exponential and the coefficients in the kernel-argument block the
// folded launch is 41 us per step at 50 000 sites against 42.5-43 with a launch of its own.)
inline bool nuc_may_fold(NucKey k) {
  k.folded = true;
  return k.n_ops > 0 && k.nuc != 2 && k.S_pad % 256 == 0 && k.S_pad / 256 <= 512 && select_nuc_form(k).inst.FOLD;
}

}  // namespace hyhip
