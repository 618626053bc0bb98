// Run-time schedule tuner of libhyphy_hip.so and the launch of the current schedule (shared with the evaluation path).
#include <map>
#include <mutex>
#include <tuple>

#include "partition.h"

namespace hyhip {

// Upload the current schedule.  sync_always (the tuner): select the device and wait even with nothing to upload; else only before a copy.
int upload_schedule(hyphy_hip_partition *p, Shard &s, bool sync_always) {
  if (sync_always) HIPCHK(hipSetDevice(s.device));
  if (sync_always || !p->ops_host.empty()) HIPCHK(hipStreamSynchronize(s.stream));
  if (p->ops_host.empty()) return 0;
  memcpy(s.h_ops, p->ops_host.data(), p->ops_host.size() * sizeof(int4));
  HIPCHK(hipMemcpyAsync(s.ops, s.h_ops, p->ops_host.size() * sizeof(int4), hipMemcpyHostToDevice, s.stream));
  for (size_t k = 0; k < p->programs.size(); k++)
    s.h_prog[k] = make_int4(p->programs[k].off, p->programs[k].n, p->programs[k].parent, p->programs[k].need);
  HIPCHK(hipMemcpyAsync(s.prog, s.h_prog, p->programs.size() * sizeof(int4), hipMemcpyHostToDevice, s.stream));
  if (p->chain) {
    memcpy(s.h_jn, p->jn_host.data(), p->jn_host.size() * sizeof(int4));
    HIPCHK(hipMemcpyAsync(s.jn, s.h_jn, p->jn_host.size() * sizeof(int4), hipMemcpyHostToDevice, s.stream));
    if (ensure_deposits(p, s)) return -1;
  }
  return 0;
}

// The pruning step of the current schedule (no expm, no reduction), for evaluations and the tuner's passes alike: prune_args_current
// brings the twin images up to date and completes a PruneArgs from the partition, launch_prune_current walks the levels, or the trunk
// walk, under it.  An evaluation adds what is its own (timeline buffer, fused-combine block) and hands the arguments back as `eval`.
PruneArgs prune_args_current(hyphy_hip_partition *p, Shard &s, int cat, int n_cat_batch) {
  if (p->rr_active && p->chain && s.twins_dirty) refresh_twins(p, s);
  PruneArgs pa = base_prune_args(p, s, cat, n_cat_batch);
  for (const auto &pr : p->programs) pa.n_ops = std::max(pa.n_ops, pr.n);  // longest program
  pa.ops = s.ops, pa.prog = s.prog;
  pa.n_prog_total = p->chain ? (int)p->I : (int)p->programs.size();
  pa.chain = p->chain ? 1 : 0;
  pa.jn = s.jn, pa.deposits = s.deposits, pa.cs_deposits = s.deposits_class_stride;
  pa.ablate = sw::ablate();
  return pa;
}

int launch_prune_current(hyphy_hip_partition *p, Shard &s, int cat, int n_cat_batch, const PruneArgs *eval, bool eval_walk) {
  PruneArgs pa = eval ? *eval : prune_args_current(p, s, cat, n_cat_batch);
  // the trunk of a class-compressed partition, lazy full pass: one row-split walk per tile instead of the schedule (repeats.hip)
  const bool walk = eval ? eval_walk : trunk_walk_applies(p, s);  // (an evaluation has decided already: its fused combine depends on it)
  if (walk) {
    if (launch_trunk_walk(p, s, cat, n_cat_batch, eval != nullptr, &pa)) return -1;  // (its own timeline: evaluations only)
    if (eval) s.last_walk = true;  // (hyphy_hip_prune_kernel_name speaks of evaluations: the tuner's passes leave it alone)
    if (eval) p->last_form_walk = true;
    return 0;
  }
  if (eval) s.last_walk = false;
  double *const red_out = pa.red_out;
  for (size_t lv = 0; lv < p->levels.size(); lv++) {  // one launch per level of subtree fragments
    pa.prog = s.prog + p->levels[lv].first;
    pa.n_prog = p->levels[lv].count;
    pa.do_root = (lv + 1 == p->levels.size()) ? 1 : 0;
    pa.red_out = pa.do_root ? red_out : nullptr;  // (the launch that finalises the roots carries the fused final combine)
    if (launch_prune_mfma(pa, s.stream))  // (the two messages differed before the copies were joined: kept)
      return fail("internal: no pruning kernel for this launch form (variant " + std::to_string(p->variant) +
                  (eval ? ", " + std::to_string(p->NW) + " row blocks)" : ")"));
  }
  if (eval) {  // (hyphy_hip_last_prune_form: what the launcher dispatched, and the cut it ran under)
    p->last_form_walk = false;
    p->last_dispatch = last_prune_dispatch();
    p->last_cut = (p->levels.empty() || pa.n_ops <= 0) ? -1 : (p->chain ? p->chain_m_used : 0);
    p->last_rerooted = p->rr_active;
  }
  return 0;
}

// Schedule tuner.  How a full pass is best cut (level-peeled fragments, or chains with sources of at most m nodes)
// depends on the tree's shape, the shard size and the number of classes in the launch; the pruning pass is idempotent,
// so on the first steady-state full pass (lazy persistence: nothing but the root is stored) the library simply runs
// the pass under each candidate cut on the resident transition matrices, times it with an event pair and keeps the
// fastest (a few milliseconds, once per partition and class-batch mode).  HYPHY_HIP_TUNE=0 or any explicit cut
// (HYPHY_HIP_CHAIN_M / HYPHY_HIP_CUT / HYPHY_HIP_FRAGMENT) disables it.
int tune_schedule(hyphy_hip_partition *p, int cat, int n_cat_batch) {
  p->tuned_for = p->batch_classes;
  const int I = p->vw().I;  // (the tree the schedules are cut from: the trunk when the partition is class-compressed)
  Shard &s = p->shards[0];
  const int T0 = s.T;
  // a candidate: kernel (0 row-split workgroups / 1 wave per tile / 2 row-split workgroups on a chain schedule / 3 (trunks) the
  // row-split walk, trunk_walk_kernel, with trunk_walk_backing's kernel behind it for the passes it does not serve), cut
  // (m > 0: chain schedule with sources of at most m nodes, -1: level-peeled fragments, 0: the kernel's own heuristic),
  // instantiation of the wave kernel (0 / 2: three waves per SIMD), re-rooting candidate (-1: the given root)
  struct Cand { int kernel, m, wv, rr; };
  auto label = [](const Cand &c) {
    char b[48];
    snprintf(b, sizeof b, "%s%s%s%d", c.rr >= 0 ? (c.rr ? "rr1/" : "rr0/") : "", c.wv == 2 ? "occ3/" : "",
             c.kernel == 3 ? "walk" : c.kernel == 0 ? "wg-kernel" : (c.kernel == 2 ? "team/m" : (c.m < 0 ? "levels" : "m")), c.m < 0 ? 0 : c.m);
    return std::string(b);
  };
  auto apply = [&](const Cand &c) -> bool {  // build the candidate's schedule; false: not applicable
    p->variant = c.kernel == 3 ? trunk_walk_backing(p) : c.kernel;
    p->trunk_walk = c.kernel == 3;
    p->wave_variant = c.kernel == 1 ? c.wv : 0;
    p->n_slots = p->variant == 1 ? (c.wv == 2 ? 2 : p->n_slots_wave) : lds_slots(T0);
    p->chain_m_forced = c.m;
    if (c.rr >= 0 && p->rr_path != p->rr_cands[(size_t)c.rr]) {
      p->rr_path = p->rr_cands[(size_t)c.rr];
      for (Shard &sh : p->shards) sh.twins_dirty = true;  // (other twins: refreshed by the transpose kernel before the launch)
    }
    p->rr_use = c.rr >= 0;
    build_schedule(p, nullptr, 0, true);
    if (p->ops_host.size() > ops_capacity(p)) return false;
    if (c.m > 0 && !p->chain) return false;  // (m >= I, or a tree the join table cannot describe: the same as no cut)
    if (c.rr >= 0 && !p->rr_active) return false;
    if (c.kernel == 3 && !trunk_walk_applies(p, s)) return false;
    return true;
  };
  int err = 0;
  auto time_it = [&](const Cand &c) -> double {  // fastest of two passes behind a warm-up pass, ms; < 0: not measured
    if (!apply(c)) return -1.;
    if (upload_schedule(p, s, true)) {
      err = -1;
      return -1.;
    }
    float ms = 0.f, ms2 = 0.f;
    bool launched = launch_prune_current(p, s, cat, n_cat_batch) == 0;  // warm-up (instruction cache, schedule in L2)
    if (hipEventRecord(s.ev[0], s.stream) != hipSuccess) return -1.;
    launched = launched && launch_prune_current(p, s, cat, n_cat_batch) == 0;
    if (hipEventRecord(s.ev[1], s.stream) != hipSuccess) return -1.;
    launched = launched && launch_prune_current(p, s, cat, n_cat_batch) == 0;
    if (hipEventRecord(s.ev[2], s.stream) != hipSuccess) return -1.;
    if (!launched) {
      err = -1;  // (fail() has the message)
      return -1.;
    }
    if (hipStreamSynchronize(s.stream) != hipSuccess || hipGetLastError() != hipSuccess) {
      err = fail("schedule tuner: a candidate launch failed");
      return -1.;
    }
    if (hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) != hipSuccess || hipEventElapsedTime(&ms2, s.ev[1], s.ev[2]) != hipSuccess) return -1.;
    const double t = std::min(ms, ms2);
    p->tune_report += (p->tune_report.empty() ? "" : " ") + label(c) + ":";
    char b[32];
    snprintf(b, sizeof b, "%.1fus", 1e3 * t);
    p->tune_report += b;
    return t;
  };
  p->tune_report.clear();
  Cand best{1, -1, 0, -1};
  double best_ms = 1e30;
  // What was chosen for the same tree, shard size and class batch earlier in this process is taken over without timing
  // anything: analyses that create one likelihood function after another on the same tree (FEL: one per site) tune once.
  // (HYPHY_HIP_TUNE_CACHE=0: every partition measures for itself.)
  struct Key {
    int64_t D, L, I, ntiles, classes, forced, mode, form;
    uint64_t topo;
    bool operator<(const Key &o) const {
      return std::tie(D, L, I, ntiles, classes, forced, mode, form, topo) <
             std::tie(o.D, o.L, o.I, o.ntiles, o.classes, o.forced, o.mode, o.form, o.topo);
    }
  };
  struct Choice { Cand cand; double ms; };
  static std::map<Key, Choice> cache;
  static std::mutex cache_mutex;
  const bool cache_on = sw::tune_cache();
  uint64_t topo = 1469598103934665603ull;  // FNV-1a over the parent vector
  for (int64_t v : p->vw().parents) topo = (topo ^ (uint64_t)v) * 1099511628211ull;
  if (p->mode == 1)  // (the trunk depends on the alignment: leaves that are class tables gather differently from plain ones)
    for (int sl : p->vw().slot) topo = (topo ^ (uint64_t)sl) * 1099511628211ull;
  // (form: the switches that take candidates out of the stages below — HYPHY_HIP_SLOTS and _WAVE_VARIANT the second stage's, _REROOT
  //  the third's — and the slot budget the wave kernel's candidates are compiled for.  A choice made without them must not be taken over
  //  by a partition created or evaluated under one of them: the three-waves instantiation has no parking slot and ignores both.)
  const int64_t form = (sw::wave_form_forced() ? 1 : 0) | (int64_t)(sw::wave_variant(-1) + 1) << 1 | (int64_t)p->n_slots_wave << 8 |
                       (int64_t)(sw::given(sw::REROOT) ? 2 + (sw::reroot() & 1) : 0) << 12;
  const Key key{p->D, p->vw().L, p->vw().I, s.ntiles, n_cat_batch, p->kernel_forced ? p->variant + (p->trunk_walk ? 8 : 0) : -1, p->mode, form, topo};
  if (cache_on) {
    std::lock_guard<std::mutex> lock(cache_mutex);
    auto hit = cache.find(key);
    if (hit != cache.end() && apply(hit->second.cand)) {
      p->tuned_ms = hit->second.ms;
      p->tune_report = "(same tree, shard size and class batch as an earlier partition of this process) -> " + label(hit->second.cand);
      sw::note("schedule tuner (%d classes per launch): %s\n", n_cat_batch, p->tune_report.c_str());
      return 0;
    }
  }
  // ---- first stage: the cut, per kernel ----
  std::vector<Cand> stage1;
  const int forced = p->kernel_forced ? p->variant : -1;  // HYPHY_HIP_KERNEL / T > 1: only that kernel's cuts compete
  if (forced < 0 || forced == 1) {
    stage1.push_back({1, -1, 0, -1});
    for (int m : {1, 2, 3, 5, 8, 12, 16, 24, 40, 64})
      if (m < I && (m >= 3 || p->mode == 1)) stage1.push_back({1, m, 0, -1});  // (a trunk is a handful of nodes: small sources matter there)
  }
  const bool small = T0 == 1 && s.ntiles < 2 * s.cus;   // below two tiles per CU
  const bool medium = T0 == 1 && s.ntiles < 4 * s.cus;
  if ((forced < 0 && small) || forced == 0) stage1.push_back({0, 0, 0, -1});  // one workgroup walks the whole tree of its tile
  if (((forced < 0 && medium && sw::team()) || forced == 2) && T0 == 1)
    for (int m : {3, 5, 8, 12, 16, 24})
      if (m < I) stage1.push_back({2, m, 0, -1});
  // r06: the trunk of a class-compressed partition under row-split workgroups (prune_mfma_kernel<.., REP>): a trunk is a handful of
  // nodes, its launch is bound by a tile's critical path — a team's edge product is a quarter of a wave's
  if (p->mode == 1 && forced == 1 && sw::trunk_team() && T0 == 1 && p->NW == 4 && s.ntiles < 8 * s.cus &&
      (size_t)p->vw().L * 32 + (size_t)(p->vw().L + p->vw().I) * 16 <= 24576) {
    stage1.push_back({0, 0, 0, -1});
    for (int m : {1, 2, 3, 5, 8})
      if (m < I) stage1.push_back({2, m, 0, -1});
  }
  // r06: ... and as ONE row-split walk per tile (trunk_walk_kernel: six-team occupancy class, A ring, B from LDS — the lower phase's kernel
  // shape); any shard size
  if (p->mode == 1 && (forced == 1 || forced == 0) && T0 == 1 && p->NW >= 2 && !p->rep_walk_host.empty() &&
      (size_t)p->vw().L * 32 + (size_t)(p->vw().L + p->vw().I) * 16 <= 24576)
    stage1.push_back({3, 0, 0, -1});
  std::vector<std::pair<double, int>> ranked[4];  // per kernel: (time, cut) of the chain schedules
  for (const Cand &c : stage1) {
    const double t = time_it(c);
    if (err) return -1;
    if (t < 0.) continue;
    if (c.m > 0) ranked[c.kernel].push_back(std::make_pair(t, c.m));
    if (t < best_ms) {
      best_ms = t;
      best = c;
    }
  }
  for (auto &r : ranked) std::sort(r.begin(), r.end());
  // ---- second stage: the wave kernel's instantiation compiled for 3 waves per SIMD (finalised node in LDS, no parking
  // slot, no register prefetch of deposits) on its three fastest cuts — it wins where waves are plentiful ----
  const double stage1_ms = best_ms;
  int wave_wv = 0;  // instantiation the wave kernel's candidates of the third stage use
  if (best.kernel == 1 && best.m > 0 && p->NW == 4 && !sw::wave_form_forced())
    for (size_t k = 0; k < ranked[1].size() && k < 3; k++) {
      const Cand c{1, ranked[1][k].second, 2, -1};
      const double t = time_it(c);
      if (err) return -1;
      // (5 % margin over the first stage: at equal tuner times the production pass of the 2-waves build is the faster one —
      //  at the headline size the tuner's back-to-back passes put this build 0-3 % ahead and production runs it 3-5 us
      //  behind (122-125 against 119 us); where it really wins the margin is 6 % (128 x 100 k) to 9 % (three batched classes))
      if (t >= 0. && t < 0.95 * stage1_ms && t < best_ms) {
        best_ms = t;
        best = c;
        wave_wv = 2;
      }
    }
  // ---- third stage: the same tree hung from the node that minimises its height (re-rooted schedules): shorter critical
  // path per tile, the same work — wins on small and medium shards of unbalanced trees ----
  if (best.m > 0 && !p->rr_path.empty() && n_cat_batch <= 1 && !sw::given(sw::REROOT)) {
    const int kn = best.kernel;
    bool rr_won = false;
    for (size_t ci = 0; ci < p->rr_cands.size(); ci++)
      for (size_t k = 0; k < ranked[kn].size() && k < 3; k++) {
        const Cand c{kn, ranked[kn][k].second, kn == 1 ? wave_wv : 0, (int)ci};
        const double t = time_it(c);
        if (err) return -1;
        // (5 % margin against the given root: the tuner's pass ranked a re-rooted form of the headline tree 4.5 % ahead that
        // was 1 % behind in production)
        if (t >= 0. && t < (rr_won ? 1.0 : 0.95) * best_ms) {
          best_ms = t;
          best = c;
          rr_won = true;
        }
      }
  }
  apply(best);  // (leaves kernel, slot budget, instantiation, cut and re-rooting path set; the caller rebuilds the schedule)
  if (cache_on) {
    std::lock_guard<std::mutex> lock(cache_mutex);
    cache[key] = Choice{best, best_ms};
  }
  p->tuned_ms = best_ms;
  p->tune_report += " -> " + label(best);
  sw::note("schedule tuner (%d classes per launch): %s\n", n_cat_batch, p->tune_report.c_str());
  return 0;
}

}  // namespace hyhip
