// Host-only check of hyphy_amd/csrc/prune_form.h (tests/test_prune_form_cpu.py compiles and runs it): over the whole key space the
// selector picks what the launch cascades it replaced picked, only compiled instantiations, never a fused-combine target without
// the build that serves it, within the LDS and grid bounds, and it reaches every instantiation of the lists.  No GPU, no HIP header.
#include <stdio.h>
#include <string.h>

#include "../hyphy_amd/csrc/prune_form.h"

using namespace hyhip;

namespace {
int g_failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                     \
    }                                                                 \
  } while (0)

// ---------------------------------------------------------------------------------------------------------------------------
// FROZEN: the two cascades as they stood before the selector (launch_prune_T / launch_prune_NW / launch_prune_mfma and
// launch_prune_nuc with their predicates), every hipLaunchKernelGGL reduced to "return the descriptor".  Not to be kept in step
// with prune_form.h: it is the record of the old rules.  (prune_wave_kernel's APF and FUSE arguments, false at every site, are left out.)
// ---------------------------------------------------------------------------------------------------------------------------
struct OldForm {
  bool launched = false;  // false: the cascade returned -1
  PruneInst inst;
  int grid[3] = {0, 0, 0}, block = 0;
  size_t lds = 0;
  int dNW = 0, dT = 0, park = -1;  // note_wave_dispatch / note_team_dispatch
  const char *label = "";
  bool on_chain = false;
};
OldForm old_wave(int NW, int NP, bool CLDS, bool TRACE, bool LB, int OCC, bool PRE, bool REP, const int (&g)[3], size_t lds, int dNW, int park,
                 const char *label) {
  OldForm o;
  o.launched = true, o.inst = wave_inst(NW, CLDS, NP, TRACE, LB, OCC, PRE, REP);
  o.grid[0] = g[0], o.grid[1] = g[1], o.grid[2] = g[2], o.block = 64, o.lds = lds;
  o.dNW = dNW, o.dT = 1, o.park = park, o.label = label;
  return o;
}
OldForm old_team(int NW, int T, bool CLDS, bool TRACE, int ABL, bool CHAIN, bool FUSE, bool REP, const int (&g)[3], size_t lds, int dNW, int dT,
                 bool on_chain, const char *label) {
  OldForm o;
  o.launched = true, o.inst = team_inst(NW, CLDS, T, TRACE, ABL, CHAIN, FUSE, REP);
  o.grid[0] = g[0], o.grid[1] = g[1], o.grid[2] = g[2], o.block = 64 * NW, o.lds = lds;
  o.dNW = dNW, o.dT = dT, o.park = -1, o.label = label, o.on_chain = on_chain;
  return o;
}
OldForm old_launch_prune(const PruneKey &a) {
  const int NW = (a.NW >= 1 && a.NW <= 3) ? a.NW : 4;  // (switch (a.NW) { case 1: case 2: case 3: default: 4 })
  const bool CLDS = a.codes_in_lds;
  const int gx_chain = (a.chain && a.T == 1 && a.xcd_pad && !a.timeline) ? ((a.ntiles + 7) & ~7) : a.ntiles / a.T;
  const int grid[3] = {a.chain ? gx_chain : a.ntiles / a.T, a.n_cat > 0 ? a.n_cat : 1, a.n_prog > 0 ? a.n_prog : 1};
  const size_t lds = CLDS ? (size_t)a.L * a.T * 16 * 2 : 0;
  const int gridc[3] = {gx_chain, a.n_cat > 0 ? a.n_cat : 1, a.n_prog > 0 ? a.n_prog : 1};
  const int gridf[3] = {a.n_prog > 0 ? a.n_prog : 1, a.n_cat > 0 ? a.n_cat : 1, a.ntiles};
  const int(&gridw)[3] = a.chain ? gridc : gridf;
  if (a.variant == 1 && a.T == 1) {
    const size_t lds1 = CLDS ? (size_t)a.L * 16 * 2 : 0;
    if (a.leaf_tab && a.timeline && NW == 4 && CLDS)
      return old_wave(4, a.n_slots <= 3 ? 1 : 2, true, true, false, HYPHY_OCC3, true, true, gridw, lds1, 4, a.n_slots <= 3 ? 1 : 2, "occ2 trace trunk");
    if (a.leaf_tab && NW == 4 && CLDS && (a.wave_variant == 2 || a.wave_variant == 3) && a.n_slots <= 2)
      return old_wave(4, 0, true, false, true, 3, a.wave_variant != 2, true, gridw, lds1, 4, 0, a.wave_variant == 2 ? "occ3 trunk" : "occ3+pre trunk");
    if (a.leaf_tab) {
      const int np = a.n_slots <= 2 ? 0 : (a.n_slots == 3 ? 1 : 2);
      return old_wave(NW, np, CLDS, false, false, HYPHY_OCC3, true, true, gridw, lds1, NW, np, "occ2 trunk");
    }
    if (a.timeline && NW == 4 && CLDS)
      return old_wave(4, a.n_slots <= 3 ? 1 : 2, true, true, false, HYPHY_OCC3, true, false, gridw, lds1, 4, a.n_slots <= 3 ? 1 : 2, "occ2 trace");
    if (NW == 4 && CLDS && a.wave_variant == 2 && a.n_slots <= 2) return old_wave(4, 0, true, false, true, 3, false, false, gridw, lds1, 4, 0, "occ3");
    if (NW == 4 && CLDS && a.wave_variant == 3 && a.n_slots <= 2) return old_wave(4, 0, true, false, true, 3, true, false, gridw, lds1, 4, 0, "occ3+pre");
    const int np = a.n_slots <= 2 ? 0 : (a.n_slots == 3 ? 1 : 2);
    return old_wave(NW, np, CLDS, false, false, HYPHY_OCC3, true, false, gridw, lds1, NW, np, "occ2");
  }
  if (a.leaf_tab && a.variant != 1) {
    if (NW == 4 && CLDS) {
      if (a.T == 1 && a.chain) return old_team(4, 1, true, false, 0, true, false, true, grid, lds, 4, 1, true, "trunk");
      if (a.T == 1) return old_team(4, 1, true, false, 0, false, false, true, grid, lds, 4, 1, false, "trunk");
    }
    return OldForm();
  }
  if (a.variant == 2 && a.chain && a.T == 1) {
    if (NW == 4 && CLDS && a.target) return old_team(4, 1, true, false, 0, true, true, false, grid, lds, NW, 1, true, "");
    return old_team(NW, 1, CLDS, false, 0, true, false, false, grid, lds, NW, 1, true, "");
  }
  if (a.timeline) return old_team(NW, 1, CLDS, true, 0, false, false, false, grid, lds, NW, 1, false, "trace");
  const int dT = a.T <= 3 ? a.T : 4;
  if (NW == 4 && CLDS && a.T == 1 && a.ablate) {
    switch (a.ablate) {
      case 1: case 2: case 4: case 16: case 62: case 63: case 127:
        return old_team(4, 1, true, false, a.ablate, false, false, false, grid, lds, NW, dT, false, "");
      default: break;
    }
  }
  switch (a.T) {
    case 1:
      if (NW == 4 && CLDS && a.target) return old_team(4, 1, true, false, 0, false, true, false, grid, lds, NW, dT, false, "");
      return old_team(NW, 1, CLDS, false, 0, false, false, false, grid, lds, NW, dT, false, "");
    case 2: return old_team(NW, 2, CLDS, false, 0, false, false, false, grid, lds, NW, dT, false, "");
    case 3: return old_team(NW, 3, CLDS, false, 0, false, false, false, grid, lds, NW, dT, false, "");
    default: return old_team(NW, 4, CLDS, false, 0, false, false, false, grid, lds, NW, dT, false, "");
  }
}
int old_prune_mfma_grid(const PruneKey &a) { return a.ntiles / a.T; }
bool old_prune_fuses_reduce(const PruneKey &a) {
  if (a.NW != 4 || !a.codes_in_lds || a.T != 1 || a.timeline || a.ablate) return false;
  if (a.leaf_tab) return false;
  return a.variant == 0 || (a.variant == 2 && a.chain);
}

bool old_takes_leaf_pairs(const NucKey &a) { return a.nuc != 0 && a.L <= 256; }
int old_nuc2_np(const NucKey &a) {
  if (!old_takes_leaf_pairs(a) || !a.PT) return 0;
  if (a.nuc == 1 || a.S_pad % 512 != 0) return 1;
  if (a.nuc == 2) return 2;
  return 1;
}
size_t old_nuc2_lds(const NucKey &a, int np, bool lp = false) {
  return (size_t)(lp ? a.L + a.root_inode : a.L) * 16 * 8 + (size_t)4 * np * 256 * (4 * 8 + 4) + (lp ? (size_t)(a.n_ops + 4) * 16 : 0);
}
bool old_nuc_uses_lp(const NucKey &a, int np) {
  return np == 1 && (a.nuc_lp >= 0 ? a.nuc_lp != 0 : a.S_pad / 256 <= 2 * a.cus) && old_nuc2_lds(a, 1, true) <= (size_t)(112 * 1024);
}
bool old_folds_expm(const NucKey &a) { return a.n_ops > 0 && old_takes_leaf_pairs(a) && a.nuc != 2 && a.S_pad % 256 == 0 && a.S_pad / 256 <= 512; }
bool old_nuc_fuses_reduce(const NucKey &a) { return a.n_ops > 0 && old_nuc_uses_lp(a, old_nuc2_np(a)); }
int old_nuc_grid(const NucKey &a) {
  const int np = old_nuc2_np(a);
  return np ? a.S_pad / (256 * np) : (a.S_pad + 255) / 256;
}
struct OldNuc {
  bool launched = false;
  PruneInst inst;
  int grid = 0, block = 256;
  size_t lds = 0;
  bool drops_exponentials = false;  // handed folded exponentials, launched a build without them
};
OldNuc old_nuc(PruneInst inst, int grid, size_t lds) {
  OldNuc o;
  o.launched = true, o.inst = inst, o.grid = grid, o.lds = lds;
  return o;
}
OldNuc old_launch_prune_nuc(const NucKey &a) {
  if (a.n_ops <= 0) return OldNuc();
  const bool pin = a.pinned;
  const int np = old_nuc2_np(a);
  if (a.leaf_tab) return old_nuc(nuc_inst(false, true), (a.S_pad + 255) / 256, 0);
  if (np == 0) return old_nuc(nuc_inst(pin, false), (a.S_pad + 255) / 256, 0);
  const int grid = a.S_pad / (256 * np);
  const size_t lds = old_nuc2_lds(a, np);
  if (old_nuc_uses_lp(a, np)) {
    const size_t ldl = old_nuc2_lds(a, 1, true);
    return old_nuc(nuc2_inst(1, pin, a.folded, true), grid, ldl);
  }
  if (a.folded && np == 1) return old_nuc(nuc2_inst(1, pin, true, false), grid, lds);
  OldNuc o = old_nuc(nuc2_inst(np, pin, false, false), grid, lds);
  o.drops_exponentials = a.folded;
  return o;
}
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int n_insts = (int)(sizeof(kPruneInsts) / sizeof(kPruneInsts[0]));
static_assert(n_insts == 56 + 59 + 3 + 10, "prune_wave_kernel 56, prune_mfma_kernel 59, prune_nuc_kernel 3, prune_nuc2_kernel 10 instantiations");
bool reached[n_insts] = {};
int index_of(const PruneInst &x) {
  for (int i = 0; i < n_insts; i++)
    if (kPruneInsts[i] == x) return i;
  return -1;
}

void check_prune() {
  for (int i = 0; i < n_insts; i++)
    for (int j = 0; j < i; j++) CHECK(!(kPruneInsts[i] == kPruneInsts[j]));  // listed once
  const int ablates[] = {0, 1, 2, 4, 8, 16, 62, 63, 127, 256}, tile_mult[] = {1, 7, 8, 9, 64};
  const int shapes[][3] = {{0, 0, 7}, {3, 1, 300}, {1, 5, 64}};  // (n_cat, n_prog, L)
  long long keys = 0;
  PruneKey k;
  for (k.NW = 1; k.NW <= 4; k.NW++)
  for (k.T = 1; k.T <= 5; k.T++)
  for (k.variant = 0; k.variant <= 2; k.variant++)
  for (k.wave_variant = 0; k.wave_variant <= 3; k.wave_variant++)
  for (k.n_slots = 2; k.n_slots <= 4; k.n_slots++)
  for (int ablate : ablates)
  for (int tm : tile_mult)
  for (const auto &sh : shapes)
  for (int bits = 0; bits < 64; bits++) {
    k.ablate = ablate, k.ntiles = tm * k.T, k.n_cat = sh[0], k.n_prog = sh[1], k.L = sh[2];
    k.chain = bits & 1, k.codes_in_lds = bits & 2, k.leaf_tab = bits & 4, k.timeline = bits & 8, k.target = bits & 16, k.xcd_pad = bits & 32;
    keys++;
    const PruneForm f = select_prune_form(k);
    PruneKey kt = k;
    kt.target = true;
    const bool fuses = f.can_fuse;  // prune_fuses_reduce
    CHECK(fuses == select_prune_form(kt).inst.FUSE && fuses == select_prune_form(kt).can_fuse);  // (the answer does not depend on the target)
    const bool team = f.inst.family == PruneFamily::team, wave = f.inst.family == PruneFamily::wave;
    {  // what the evaluation stage reads before the launcher has read HYPHY_HIP_XCD_PAD, and the family before it has a trace buffer
      PruneKey kx = k;
      kx.xcd_pad = !k.xcd_pad;
      const PruneForm fx = select_prune_form(kx);
      CHECK(fx.inst == f.inst && fx.n_wg == f.n_wg && fx.can_fuse == f.can_fuse);
      kx = k, kx.timeline = !k.timeline;
      CHECK(select_prune_form(kx).inst.family == f.inst.family && select_prune_form(kx).n_wg == f.n_wg);
    }

    // -- no orphan record: the build carries the combine exactly when a target came with a key for which the predicate says yes
    CHECK(f.inst.FUSE == (k.target && fuses));
    CHECK(fuses == old_prune_fuses_reduce(k));
    CHECK(f.n_wg == old_prune_mfma_grid(k));

    // -- equality with the cascade.  Two sets of keys no caller produces are apart:
    //    (a) a target where the predicate says no (the stage wires red_out only behind prune_fuses_reduce): the cascade looked at the
    //        target alone and would have launched a FUSE build under an ablation bit without a build of its own, under a timeline on
    //        a chain, and for variant 2 without a chain; the selector keeps to the predicate;
    //    (b) a trunk with variant 1 and T > 1 (shard_geometry sets variant 0 whenever T != 1): the cascade fell through to the
    //        level-schedule builds, which know nothing of generalised leaves; the selector reports that no build serves it.
    OldForm o = old_launch_prune(k);
    if (k.target && !old_prune_fuses_reduce(k)) o.inst.FUSE = false;                     // (a)
    if (k.leaf_tab && k.variant == 1 && k.T != 1) o = OldForm();                         // (b)
    CHECK(o.launched == (team || wave));
    if (o.launched && (team || wave)) {
      CHECK(o.inst == f.inst);
      CHECK(o.grid[0] == f.grid[0] && o.grid[1] == f.grid[1] && o.grid[2] == f.grid[2] && o.block == f.block && o.lds == f.lds);
      CHECK(o.dNW == f.inst.NW && o.dT == f.disp_T && o.park == f.park && o.on_chain == f.on_chain && strcmp(o.label, f.label) == 0);
    }

    // -- membership; "none" exactly for a trunk under the row-split kernel outside NW == 4, codes in LDS, T == 1
    const bool team_rules = !(k.variant == 1 && k.T == 1);
    CHECK((f.inst.family == PruneFamily::none) == (team_rules && k.leaf_tab && !(k.NW == 4 && k.codes_in_lds && k.T == 1)));
    if (team || wave) {
      const int at = index_of(f.inst);
      CHECK(at >= 0);
      if (at >= 0) reached[at] = true;
    }

    // -- resources: the tile dimension is padded to a multiple of 8 exactly when the XCD padding applies, and then covers every tile
    if (team || wave) {
      const bool padded = k.chain && k.T == 1 && k.xcd_pad && !k.timeline;
      const int tiles_dim = (wave && !k.chain) ? f.grid[2] : f.grid[0];
      if (padded) CHECK(tiles_dim % 8 == 0 && tiles_dim >= k.ntiles && tiles_dim < k.ntiles + 8);
      else CHECK(tiles_dim == k.ntiles / k.T);
      // workgroups that write wg_sum: one per tile (wave; the surplus of a padded grid retires), one per T tiles (team)
      CHECK(f.n_wg == (wave ? k.ntiles : k.ntiles / k.T));
      CHECK(f.block == 64 * (wave ? 1 : f.inst.NW) && f.grid[1] >= 1 && f.grid[2] >= 1);
      CHECK(f.lds <= 64 * 1024);
    }
  }
  CHECK(keys == 4LL * 5 * 3 * 4 * 3 * 10 * 5 * 3 * 64);
}

void check_nuc() {
  const int Ls[] = {2, 256, 257}, S_pads[] = {256, 512, 768, 512 * 256, 513 * 256}, n_opss[] = {0, 1, 100, 6000}, roots[] = {1, 255, 600};
  const int nucs[] = {-1, 0, 1, 2, 3}, lps[] = {-1, 0, 1}, cuss[] = {1, 256};
  NucKey k;
  for (int L : Ls)
  for (int S_pad : S_pads)
  for (int n_ops : n_opss)
  for (int root : roots)
  for (int nuc : nucs)
  for (int lp : lps)
  for (int cus : cuss)
  for (int bits = 0; bits < 16; bits++) {
    k.L = L, k.S_pad = S_pad, k.n_ops = n_ops, k.root_inode = root, k.nuc = nuc, k.nuc_lp = lp, k.cus = cus;
    k.PT = bits & 1, k.leaf_tab = bits & 2, k.pinned = bits & 4, k.folded = bits & 8;
    const PruneForm f = select_nuc_form(k);
    const OldNuc o = old_launch_prune_nuc(k);

    // -- equality with the cascade (which launched nothing for an empty schedule; the launcher still returns before it selects)
    if (o.launched) {
      CHECK(o.inst == f.inst && o.grid == f.grid[0] && f.grid[1] == 1 && f.grid[2] == 1 && o.block == f.block && o.lds == f.lds);
      // the suspect: folded exponentials handed to a build that ignores them (HYPHY_HIP_NUC=2, two patterns per thread).  The gate
      // in front of every folded launch (prune_nuc_folds_expm) refuses that key, so it is never asked for.
      if (o.drops_exponentials) CHECK(!nuc_may_fold(k) && k.nuc == 2);
    }
    // -- the predicates.  With a trunk leaf table AND transposed matrices (no caller: the trunk passes PT = nullptr) the old
    //    predicates answered for prune_nuc2_kernel while the cascade launched prune_nuc_kernel<false, true>; the selector's follow the launch.
    const bool split = k.leaf_tab && k.PT && old_takes_leaf_pairs(k);
    CHECK(f.leaf_pairs == old_takes_leaf_pairs(k));
    if (!split) {
      CHECK(f.n_wg == old_nuc_grid(k) && f.n_wg == f.grid[0]);
      CHECK((k.n_ops > 0 && f.can_fuse) == old_nuc_fuses_reduce(k) && f.can_fuse == f.inst.LP);
    } else {
      CHECK(!f.inst.LP && f.n_wg == (k.S_pad + 255) / 256);
    }
    NucKey kf = k;
    kf.PT = true, kf.leaf_tab = false;  // (what prune_nuc_folds_expm knows: L, S_pad, n_ops)
    CHECK(nuc_may_fold(kf) == old_folds_expm(k));
    // -- no orphan: a caller told "may fold" / "fuses" gets the build that folds / carries the combine
    kf = k, kf.folded = true;
    if (nuc_may_fold(k) && k.PT && !k.leaf_tab) CHECK(select_nuc_form(kf).inst.FOLD);
    if (!split && old_nuc_fuses_reduce(k)) CHECK(o.launched && f.inst.LP);

    // -- membership, resources
    const int at = index_of(f.inst);
    CHECK(at >= 0);
    if (at >= 0) reached[at] = true;
    CHECK(f.lds <= kNucLdsCap && f.block == 256);
    if (f.inst.family == PruneFamily::nuc) CHECK(f.lds == 0 && f.n_wg == (k.S_pad + 255) / 256);  // one workgroup per 256 patterns writes a partial
    else CHECK(f.inst.family == PruneFamily::nuc2 && f.n_wg * 256 * f.inst.NP == k.S_pad && k.L * 128 <= 32 * 1024);
  }
}
}  // namespace

int main() {
  check_prune();
  check_nuc();
  for (int i = 0; i < n_insts; i++) CHECK(reached[i]);  // reachability: every listed instantiation is selected by some key
  if (g_failed) {
    fprintf(stderr, "prune_form_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  printf("prune_form_check: ok\n");
  return 0;
}
