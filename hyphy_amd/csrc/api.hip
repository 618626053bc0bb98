// C-ABI of libhyphy_hip.so (include/hyphy_hip.h): partition state, pattern sharding over devices, evaluation entry
// points, kernel sequencing.  The schedule compiler lives in schedule.hip, the run-time tuner in tuner.hip, RCCL in
// comm.hip; shared host-side types in partition.h.  Host-side bookkeeping only — all arithmetic of the hot path happens
// in expm.hip / prune.hip / sitefit.hip.
#include "partition.h"

using namespace hyhip;

namespace hyhip {

thread_local std::string g_last_error;

int fail(const std::string &msg) {
  g_last_error = msg;
  return -1;
}

namespace {

void free_shard(Shard &s) {
  hipSetDevice(s.device);
  if (s.stream) hipStreamSynchronize(s.stream);
  s.own.release_all();  // (the stream was synchronised above)
  for (RepPassSlot &ps : s.rep_slot)
    if (ps.ev) hipEventDestroy(ps.ev);
  for (auto &e : s.ev)
    if (e) hipEventDestroy(e);
  for (auto &e : s.ev_ar)
    if (e) hipEventDestroy(e);
  for (auto &e : s.ring)
    if (e) hipEventDestroy(e);
  for (auto &e : s.coeff_ev)
    if (e) hipEventDestroy(e);
  for (auto &e : s.tstage_ev)
    if (e) hipEventDestroy(e);
  if (s.comm && g_rccl.CommDestroy) g_rccl.CommDestroy(s.comm);
  if (s.own_stream) pool_stream_put(s.own_stream);
  s = Shard();
}

int upload_small(Shard &s, const double *src, size_t n, double *dst) {
  if (n > s.h_small_cap) return fail("internal: staging buffer too small");
  HIPCHK(hipStreamSynchronize(s.stream));  // staging buffer reuse
  memcpy(s.h_small, src, n * sizeof(double));
  HIPCHK(hipMemcpyAsync(dst, s.h_small, n * sizeof(double), hipMemcpyHostToDevice, s.stream));
  return 0;
}

// Sequence number for the result record of a synchronous evaluation (0: the caller must wait for the stream).
double next_seq(Shard &s, bool host_record) {
  if (!sw::spin() || !host_record || !s.d_hout) {
    s.seq_wait = 0.;
    return 0.;
  }
  s.seq_wait = s.seq_next;
  s.seq_next += 1.;
  return s.seq_wait;
}

}  // namespace

double result_seq(Shard &s, bool host_record) { return next_seq(s, host_record); }

// Twin images of re-rooted schedules (ExpmArgs::n_twin): slot of twin j relative to the class base, and the refresh by the
// branch cache's transpose kernel for the cases the exponential kernel did not cover (a writer other than the fused path,
// new root frequencies without a new matrix).
void refresh_twins(hyphy_hip_partition *p, Shard &s) {
  if (p->rr_path.empty() || p->nuc) return;
  const size_t DD = (size_t)p->DP * p->DP;
  for (size_t j = 0; j + 1 < p->rr_path.size(); j++)
    launch_transpose_frag(s.Pfrag + (size_t)p->vw().slot[p->vw().L + p->rr_path[j + 1]] * DD, s.Pfrag + (size_t)(twin_slot0(p) + (int)j) * DD,
                          j == 0 ? s.pi : nullptr, p->NW, s.stream);
  s.twins_dirty = false;
}

// Edge products of the non-last arrivers of a chain schedule: one tile per (class, internal node of the view, tile).  Sized for the
// tree the schedules are cut from — the trunk when the partition runs class-compressed (16 of 62 internal nodes at the headline
// workload, 20 of 127 at 128 x 100 k: 1.0 GB instead of 6.5) — and grown when a larger view needs it.
int ensure_deposits(hyphy_hip_partition *p, Shard &s) {
  const size_t node_stride = (size_t)s.ntiles * 16 * p->DP;
  const size_t class_stride = (size_t)p->vw().I * node_stride;
  const size_t need = (size_t)p->C * class_stride;
  s.deposits_class_stride = class_stride;
  if (s.deposits_cap >= need) return 0;
  HIPCHK(s.own.regrow({device_block(s.deposits, need * sizeof(double))}, s.deposits_cap, need, need, FreeMode::Sync));
  if (sw::poison()) {
    HIPCHK(hipMemset(s.deposits, 0xff, need * sizeof(double)));
    HIPCHK(hipDeviceSynchronize());
  }
  return 0;
}
void release_deposits(Shard &s) {  // (a smaller view takes over: ensure_deposits sizes them again)
  s.own.drop(s.deposits, FreeMode::Sync);
  s.deposits_cap = 0;
}

// Everything in a PruneArgs that does not depend on the schedule being launched.
PruneArgs base_prune_args(hyphy_hip_partition *p, Shard &s, int cat, int n_cat_batch) {
  const int64_t B = p->B;
  const int DP = p->DP;
  PruneArgs pa{};  // (what is not set below is null / zero: the schedule, the chain part, the timeline, the fused final combine)
  pa.n_prog = pa.do_root = pa.n_prog_total = 1;
  pa.NW = p->NW, pa.T = s.T, pa.S_pad = s.S_pad, pa.ntiles = s.ntiles;
  const hyphy_hip_partition::View &v = p->vw();  // (node indices and leaf numbers are the view's; class strides the partition's)
  pa.root_inode = v.I - 1;
  pa.root_slot = p->root_slot;
  pa.L = v.L;
  pa.variant = p->variant;
  pa.n_slots = p->n_slots;
  pa.codes_in_lds = ((size_t)v.L * s.T * 32 + (size_t)(v.L + v.I) * 16 <= 24576) ? 1 : 0;
  pa.Pfrag = s.Pfrag + (size_t)cat * B * DP * DP;
  pa.PTg = s.PTg + (size_t)cat * B * DP * DP;
  pa.codes = s.codes;
  pa.codes_tile = s.codes_tile;
  if (p->mode == 1) {  // the trunk of a class-compressed partition: generalised leaves (repeats.hip)
    pa.codes_tile = s.rep_codes_tile;
    pa.codes = nullptr;  // (row-major leaf table: the kernels of this mode read the tile-major one)
    pa.leaf_tab = s.rep_leaf;
    pa.gtab = s.rep_tab + (size_t)cat * s.rep_rows * DP;
    pa.gcnt = s.rep_cnt + (size_t)cat * s.rep_rows;
    pa.cs_gtab = (size_t)s.rep_rows * DP;
    pa.cs_gcnt = (size_t)s.rep_rows;
  }
  pa.pin = s.pin;
  pa.pin_leaf = (p->pin_node >= 0 && p->pin_node < p->L) ? (int)p->pin_node : -1;
  pa.pin_inode = p->pin_node >= p->L ? (int)(p->pin_node - p->L) : -1;
  pa.ambig = s.ambig;
  pa.partials = s.partials + (size_t)cat * s.partial_stride;
  pa.counts = s.counts + (size_t)cat * p->I * s.S_pad;
  pa.pi = s.pi;
  pa.site_lik = s.site_lik + (size_t)cat * s.S_pad;
  pa.site_cnt = s.site_cnt + (size_t)cat * s.S_pad;
  pa.freq = s.freq;
  if (p->rr_active && p->chain && !p->nuc) pa.pi = s.pi_ones;  // (re-rooted schedule: pi is folded into the old root's twin image)
  pa.wg_sum = s.wg_sum, pa.wg_cnt = s.wg_cnt, pa.wg_flag = s.wg_flag;
  pa.n_cat = n_cat_batch;
  pa.cs_P = (size_t)B * DP * DP;
  pa.cs_partials = s.partial_stride;
  pa.cs_counts = (size_t)p->I * s.S_pad;
  pa.cs_site = (size_t)s.S_pad;
  pa.cs_wg = (size_t)s.ntiles / s.T;
  pa.frag_ctr = s.frag_ctr;
  pa.hand_cnt = s.hand_cnt;
  pa.wave_variant = sw::wave_variant(p->wave_variant);
  return pa;
}

namespace {

// Pinned staging of the class-batched mixture entry points (Shard::h_mixst): [C class weights | B + 1 offsets (int) | mixture weights]
size_t mixst_weights_at(const hyphy_hip_partition *p) { return (size_t)p->C + ((size_t)p->B + 2) / 2; }

// ---- one evaluation on one shard: enqueue_eval runs the stages below, in this order, over one context on its stack ----
struct Timeline;
struct EvalCtx {
  hyphy_hip_partition *p;
  Shard &s;
  int cat, n_cat_batch;                          // class (class 0 of a batch), classes in the launch
  bool sched_changed, pi_changed, slots_changed;  // what eval_common found changed against the host caches
  const EvalRequest &rq;
  Trace tr{"enqueue"};
  int n_ops = 0;                  // longest program of the schedule: > 0 means a pruning launch follows
  bool use_gen = false;           // 4 states: the run-time generated kernel serves this pass
  ExpmArgs folded_expm;           // 4 states, small shard (have_folded): the exponentials the pruning launch computes itself
  bool have_folded = false, stamp = false;  // stamp: this evaluation carries a kernel-duration stamp ...
  size_t ring_slot = 0;           // ... in this pair of the timing ring
  int n_wg = 0;                   // workgroups of the launch that leaves per-workgroup partial sums
  bool fused_reduce = false;      // ... which also ran the final combine
  double *site_lik() const { return s.site_lik + (size_t)cat * s.S_pad; }
  int32_t *site_cnt() const { return s.site_cnt + (size_t)cat * s.S_pad; }
  int32_t *d_slots() const { return s.slots + (size_t)cat * p->B; }
  const double *dense_q() const { return rq.q_source == QSource::OwnStaged ? s.qbuf : rq.q; }
  bool q_on_device() const { return rq.q_source != QSource::HostDense; }
  int enqueue_eval();
  int stage_schedule(), stage_pi(), stage_slot_table(), stage_expm_mixture(), stage_expm_plain(), stage_stamps_open(), stage_prune_nuc(),
      stage_prune_mfma(), stage_stamps_close(), stage_export(), stage_reduce();
  int stage_expm_class_mixture(bool mix_built);
  void stage_gen_decision();
  ExpmArgs expm_args_common(bool built) const;
  int guard_coeff_slot();
  bool fused_combine_allowed() const;
  template <typename Args>
  void wire_fused_combine(Args &a, int *red_done);
  int dump_timeline(const Timeline &tl);
};

int EvalCtx::stage_schedule() {  // schedule upload, deposits of chain schedules
  HIPCHK(hipSetDevice(s.device));
  tr.lap("setdevice");
  if (sched_changed && !p->ops_host.empty()) {  // (a chain schedule's deposits are seen to inside)
    if (upload_schedule(p, s, false)) return -1;
  } else if (p->chain && ensure_deposits(p, s)) return -1;
  return 0;
}

int EvalCtx::stage_pi() {  // root frequencies, zero padded (uploaded only when they change)
  if (pi_changed) {
    std::vector<double> pi(p->nuc ? 4 : p->DP, 0.0);
    for (int64_t k = 0; k < p->D; k++) pi[k] = rq.root_freqs[k];
    if (upload_small(s, pi.data(), pi.size(), s.pi)) return -1;
    if (!p->rr_path.empty()) s.twins_dirty = true;  // (pi sits in the twin of the old root's edge; an expm launch that covers every twin clears this again)
  }
  tr.lap("ops+pi");
  if (p->all_timings) HIPCHK(hipEventRecord(s.ev[0], s.stream));
  tr.lap("event0");
  return 0;
}

// 4 states: a schedule that keeps coming back runs as straight-line code compiled at run time (nucgen.hip) — requested after
// HYPHY_HIP_NUCGEN_AFTER evaluations under it, used from the evaluation that finds it compiled; the interpreter until then and for
// everything the generator does not cover (pinned states, the trunk of a class-compressed partition, one-leaf entries)
void EvalCtx::stage_gen_decision() {
  for (const auto &pr : p->programs) n_ops = std::max(n_ops, pr.n);
  if (!(p->nuc && p->mode == 0 && p->nucgen_key != 0 && n_ops > 0 && p->pin_node < 0 && p->nuc_leaf_pairs && p->programs.size() == 1 &&
        s.S_pad % 256 == 0))
    return;
  const int gm = sw::nucgen();  // 0 off, 1 background compilation (default), 2 synchronous
  if (gm == 0) return;
  use_gen = nucgen_ready(p->nucgen_key);
  if (!use_gen && (gm == 2 || ++p->nucgen_uses >= sw::nucgen_after()) && !p->nucgen_asked) {
    p->nucgen_asked = true;
    nucgen_request(p->nucgen_key, p->ops_host.data() + p->programs[0].off, p->programs[0].n, (int)p->L, !p->cached_persist, p->nucgen_small, (int)p->B, gm == 2);
    use_gen = nucgen_ready(p->nucgen_key);
  }
}

// n_cat_batch > 1: the matrices of ALL rate classes in one expm launch, class-major; destination
// slot of matrix (c, k) is c*B + q_nodes[k] relative to class 0's image arrays
int EvalCtx::stage_slot_table() {
  if (!slots_changed) return 0;
  const int64_t B = p->B, n_q = rq.n_q;
  int32_t *h_slots = s.h_slots + (size_t)cat * B;
  HIPCHK(hipStreamSynchronize(s.stream));
  for (int k = 0; k < n_cat_batch; k++)
    for (int64_t j = 0; j < n_q; j++) {
      if (rq.q_nodes[j] < 0 || rq.q_nodes[j] >= B) return fail("q_nodes entry out of range");
      h_slots[k * n_q + j] = (int32_t)(k * B + rq.q_nodes[j]);
    }
  HIPCHK(hipMemcpyAsync(d_slots(), h_slots, n_q * n_cat_batch * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
  return 0;
}

// What every exponential launch of an evaluation states: size, status word and — `built`: rows staged by hyphy_hip_build_q — the template part.
ExpmArgs EvalCtx::expm_args_common(bool built) const {
  ExpmArgs ea;
  ea.D = (int)p->D;
  ea.status = s.status;
  if (built) {
    ea.templates = s.templates;
    ea.templates_pad = s.templates_pad;
    ea.coeffs = s.coeffs_cur ? s.coeffs_cur : s.coeffs;
    ea.coeffs_host = (s.coeffs_cur && s.d_hcoeffs) ? s.h_coeffs + (s.coeffs_cur - s.d_hcoeffs) : nullptr;
    ea.K = (int)p->K;
  }
  return ea;
}

// The fused expm kernel reads a coefficient ring slot over PCIe when it EXECUTES: behind the launch that consumes the slot an
// asynchronous caller (d_logl_out) records the slot's event, and hyphy_hip_build_q waits for it before rewriting the slot.
int EvalCtx::guard_coeff_slot() {
  if (!rq.d_logl_out || s.coeff_slot < 0) return 0;
  HIPCHK(hipEventRecord(s.coeff_ev[s.coeff_slot], s.stream));
  s.coeff_busy[s.coeff_slot] = true;
  return 0;
}

// explicit-form branch-site mixtures: exponentiate every component, then mix into the branch's matrix images.  Component rate
// matrices: dense from the host, or (the shard's own buffer behind hyphy_hip_build_q) formed inside the exponential kernel from the
// staged coefficient rows, one row per (branch, component)
int EvalCtx::stage_expm_mixture() {
  const int64_t D = p->D, B = p->B, n_q = rq.n_q;
  const int DP = p->DP;
  const bool mix_built = q_on_device() && dense_q() == s.qbuf && p->coeffs_pending;
  if ((q_on_device() && !mix_built) || rq.q_is_probability || (n_cat_batch != 1 && !rq.batch))
    return fail("mixture evaluation: host rate matrices or hyphy_hip_build_q rows");
  // a class batch: the components of ALL classes in one exponential launch, class-major (component (c, k, m) at c * n_tot + off[k] + m)
  const size_t n_tot = (size_t)rq.mix->n_tot, n_all = n_tot * (size_t)(rq.batch ? n_cat_batch : 1), DD = (size_t)D * D;
  if (mix_built && s.coeff_rows != (int64_t)n_all)
    return fail("mixture evaluation: hyphy_hip_build_q staged a different number of rows than the components of this evaluation");
  // (rows are staged without saying what they are: the first evaluation that consumes a staging claims it — one row per (branch,
  //  component) here, per (class, branch, component) in a class batch — and an evaluation of another kind that happens to need the
  //  same number of rows is refused)
  const int kind = rq.batch ? 3 : 2;
  if (mix_built && s.coeff_kind == 1) return fail("mixture evaluation: the staged rows were consumed as one row per (class, branch): call hyphy_hip_build_q first");
  if (mix_built && s.coeff_kind != 0 && s.coeff_kind != kind)
    return fail(kind == 3 ? "mixture evaluation: the staged rows were consumed as one row per (branch, component) of one class: call hyphy_hip_build_q first"
                          : "mixture evaluation: the staged rows were consumed as one row per (class, branch, component): call hyphy_hip_build_q first");
  if (mix_built) s.coeff_kind = kind;
  {  // (n_q <= B: eval_common has checked); the rate matrices' block only where dense matrices arrive
    const size_t cap = std::max(n_all, (size_t)(2 * B));
    if (s.mix_cap < n_all) s.mix_counts_dev.clear();  // (mix_off moves with its group)
    HIPCHK(s.own.regrow({device_block(s.mix_p, cap * DD * sizeof(double)), device_block(s.mix_w, cap * sizeof(double)),
                         device_block(s.mix_off, ((size_t)B + 1) * sizeof(int))},
                        s.mix_cap, n_all, cap, FreeMode::Sync));
    if (!mix_built || !rq.batch)  // (one-class calls keep the allocations they always made)
      HIPCHK(s.own.regrow({device_block(s.mix_q, cap * DD * sizeof(double))}, s.mix_q_cap, n_all, cap, FreeMode::Sync));
  }
  if (rq.batch) return stage_expm_class_mixture(mix_built);
  s.mix_counts_dev.clear();  // (the offsets of this call replace a class batch's)
  std::vector<int> off((size_t)n_q + 1, 0);
  for (int64_t k = 0; k < n_q; k++) off[k + 1] = off[k] + (int)rq.mix->count[k];
  if (!mix_built) HIPCHK(hipMemcpyAsync(s.mix_q, dense_q(), n_tot * DD * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(s.mix_w, rq.mix->weights, n_tot * sizeof(double), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(s.mix_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));  // (pageable sources; `off` goes out of scope)
  ExpmArgs ea = expm_args_common(mix_built);
  ea.Q = s.mix_q, ea.n = (int)n_tot, ea.Prow = s.mix_p;
  const bool coeffs_consumed = launch_expm(ea, s.stream);
  if (mix_built && !coeffs_consumed && guard_coeff_slot()) return -1;
  s.twins_dirty = true;  // (the mixing kernel writes matrix images without their twins)
  launch_mix_images(s.mix_p, s.mix_off, s.mix_w, d_slots(), (int)n_q, (int)D,
                    p->nuc ? nullptr : s.Pfrag + (size_t)cat * B * DP * DP, p->nuc ? nullptr : s.PTg + (size_t)cat * B * DP * DP,
                    p->nuc ? s.Prow + (size_t)cat * B * 16 : nullptr, s.stream,
                    p->nuc ? s.Prow + ((size_t)p->C * B + (size_t)cat * B) * 16 : nullptr);
  return 0;
}

// ... of a class batch (stage_expm_mixture has sized the device blocks and claimed the rows): ONE exponential launch over the C * n_tot
// components, then mix_class_images_kernel with a grid row per class.  Weights and offsets travel through the pinned staging the entry
// point prepared (prepare_class_mixture_staging), in-stream: with rows staged by hyphy_hip_build_q nothing here waits for the stream;
// the offsets are uploaded only when the counts or the list changed.  Dense matrices come from pageable memory: one wait.
int EvalCtx::stage_expm_class_mixture(bool mix_built) {
  const int64_t D = p->D, B = p->B, n_q = rq.n_q;
  const int DP = p->DP;
  const size_t n_tot = (size_t)rq.mix->n_tot, n_all = n_tot * (size_t)n_cat_batch, DD = (size_t)D * D;
  if (!s.h_mixst || s.mixst_cap < n_all) return fail("internal: the class-mixture staging was not prepared");
  int *h_off = reinterpret_cast<int *>(s.h_mixst + p->C);
  double *h_w = s.h_mixst + mixst_weights_at(p);
  s.mixst_inflight = true;
  const std::vector<int64_t> &known = s.mix_counts_dev;
  if (slots_changed || known.size() != (size_t)n_q || memcmp(known.data(), rq.mix->count, (size_t)n_q * sizeof(int64_t))) {
    h_off[0] = 0;
    for (int64_t k = 0; k < n_q; k++) h_off[k + 1] = h_off[k] + (int)rq.mix->count[k];
    HIPCHK(hipMemcpyAsync(s.mix_off, h_off, ((size_t)n_q + 1) * sizeof(int), hipMemcpyHostToDevice, s.stream));
    s.mix_counts_dev.assign(rq.mix->count, rq.mix->count + n_q);
  }
  memcpy(h_w, rq.mix->weights, n_all * sizeof(double));
  HIPCHK(hipMemcpyAsync(s.mix_w, h_w, n_all * sizeof(double), hipMemcpyHostToDevice, s.stream));
  if (!mix_built) {
    HIPCHK(hipMemcpyAsync(s.mix_q, dense_q(), n_all * DD * sizeof(double), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));  // (pageable source)
  }
  ExpmArgs ea = expm_args_common(mix_built);
  ea.Q = s.mix_q, ea.n = (int)n_all, ea.Prow = s.mix_p;
  const bool coeffs_consumed = launch_expm(ea, s.stream);
  if (mix_built && !coeffs_consumed && guard_coeff_slot()) return -1;
  s.twins_dirty = true;  // (the mixing kernel writes matrix images without their twins)
  launch_mix_class_images(s.mix_p, s.mix_off, s.mix_w, d_slots(), (int)n_q, n_cat_batch, (int)n_tot, (int)D,
                          s.Pfrag + (size_t)cat * B * DP * DP, s.PTg + (size_t)cat * B * DP * DP, s.stream);
  return 0;
}

int EvalCtx::stage_expm_plain() {
  const int64_t D = p->D, B = p->B, n_q = rq.n_q, n_mat = n_q * n_cat_batch;
  const int DP = p->DP, q_is_prob = rq.q_is_probability;
  const double *dq = dense_q();
  const bool own = q_on_device() && dq == s.qbuf && !q_is_prob;
  const bool q_from_templates = own && p->coeffs_pending;
  if (own) {
    // the partition's own Q buffer is only meaningful behind hyphy_hip_build_q: either the staged coefficients
    // (fused construction) or the materialised matrices, with exactly the rows this evaluation consumes
    if (!q_from_templates && !s.qbuf_built) return fail("evaluate from the Q buffer: no rate matrices staged (call hyphy_hip_build_q first)");
    if (s.coeff_rows != n_mat) return fail("evaluate from the Q buffer: hyphy_hip_build_q staged a different number of matrices than this evaluation consumes");
    if (s.coeff_kind >= 2) return fail("evaluate from the Q buffer: the staged rows were consumed as mixture components: call hyphy_hip_build_q first");
    s.coeff_kind = 1;
  }
  if (!q_on_device()) {
    HIPCHK(hipMemcpyAsync(s.qbuf, dq, (size_t)n_mat * D * D * sizeof(double), hipMemcpyHostToDevice, s.stream));
    dq = s.qbuf;
  }
  ExpmArgs ea = expm_args_common(q_from_templates);  // (fused build: coefficients were staged by hyphy_hip_build_q)
  ea.Q = dq, ea.slots = d_slots(), ea.n = (int)n_mat, ea.is_prob = q_is_prob;
  ea.prof = sw::expm_prof_now() ? 1 : 0;
  if (p->nuc) {
    ea.Prow = s.Prow + (size_t)cat * B * 16;
    ea.PTrow = s.Prow + ((size_t)p->C * B + (size_t)cat * B) * 16;  // (transposed copies behind the row-major ones)
  } else {
    ea.Pfrag = s.Pfrag + (size_t)cat * B * DP * DP;
    ea.PTg = s.PTg + (size_t)cat * B * DP * DP;
    if (sw::expm_mask() && s.expm_need) {
      ea.need = s.expm_need;
      ea.need_B = (int)B;
    }
  }
  if (!p->rr_path.empty() && !p->nuc && n_cat_batch <= 1) {  // keep the transposed twins in step with the matrices they mirror
    const size_t k = p->rr_path.size() - 1;
    ea.n_twin = (int)k;
    for (size_t j = 0; j < k; j++) ea.twin_src[j] = p->vw().slot[p->vw().L + p->rr_path[j + 1]];
    ea.twin_dst0 = twin_slot0(p);
    ea.twin_pi = s.pi;
    size_t covered = 0;
    for (int64_t q = 0; q < n_q; q++)
      for (size_t j = 0; j < k; j++)
        if (rq.q_nodes[q] == ea.twin_src[j]) covered++;
    if (covered == k) s.twins_dirty = false;           // every twin rewritten by this launch (with the current pi)
  }
  tr.lap("slots+q");
  if (p->nuc && p->mode == 0 && (!use_gen || p->nucgen_small) && prune_nuc_folds_expm((int)p->L, s.S_pad, n_ops) && !(q_from_templates && !ea.coeffs)) {
    folded_expm = ea;  // (4 states, small shard: the pruning launch computes the exponentials itself — and guards the ring slot behind it)
    have_folded = true;
    set_last_expm_kernel("");
  } else {
    const bool coeffs_consumed = launch_expm(ea, s.stream);
    if (q_from_templates && !coeffs_consumed && guard_coeff_slot()) return -1;
  }
  tr.lap("launch_expm");
  return 0;
}

// kernel-duration stamps (an event pair around the pruning launches: two barrier packets, ~5 us of stream time at the
// headline size): one evaluation in 16 by default — an optimiser's sweep should not pay for a profile nobody reads —,
// HYPHY_HIP_TIMING_EVERY=n keeps one in n (bench.py: 4, the rocprofv3 runs: 1)
int EvalCtx::stage_stamps_open() {
  const int timing_every = sw::timing_every();
  stamp = timing_every == 1 || p->all_timings || (s.eval_count++ % (uint64_t)timing_every) == 0;
  s.last_stamped = stamp;
  ring_slot = (size_t)(s.ring_count % kTimingRing) * 2;
  if (stamp && !s.ring[ring_slot]) {  // (the ring's events are made on first use: a short-lived partition never pays for 2 048 of them)
    HIPCHK(hipEventCreate(&s.ring[ring_slot]));
    HIPCHK(hipEventCreate(&s.ring[ring_slot + 1]));
  }
  if (p->all_timings) HIPCHK(hipEventRecord(s.ev[1], s.stream));  // (before the ring's stamp: the exponentials' interval ends here)
  if (stamp) HIPCHK(hipEventRecord(s.ring[ring_slot], s.stream));
  return 0;
}
int EvalCtx::stage_stamps_close() {
  tr.lap("launch_prune");
  if (stamp) {
    HIPCHK(hipEventRecord(s.ring[ring_slot + 1], s.stream));
    s.ring_count++;
  }
  if (p->all_timings) HIPCHK(hipEventRecord(s.ev[2], s.stream));
  return 0;
}

// Fused final combine: the launch that finalises the roots also sums the per-tile partial sums and publishes the record —
// the last root-finalising wave does what wg_reduce_kernel would do in a launch of its own (prune.hip: publish_partial); red_done: its zeroed arrival word.
template <typename Args>
void EvalCtx::wire_fused_combine(Args &a, int *red_done) {
  double *const d_logl_out = rq.d_logl_out, *rec = s.d_hout ? s.d_hout : s.out;
  fused_reduce = true;
  if (&s == &p->shards[0]) p->last_reduce = {"fused", n_wg, false};
  a.red_out = d_logl_out ? d_logl_out : rec, a.red_rec = d_logl_out ? s.out + 1 : rec + 1;
  a.red_status = d_logl_out ? nullptr : s.status;
  a.red_seq = next_seq(s, !d_logl_out), a.red_done = red_done;
}
// what both pruning stages ask before they fuse (HYPHY_HIP_FUSED_REDUCE is theirs to read: its default differs)
bool EvalCtx::fused_combine_allowed() const {
  return rq.reduce && n_ops > 0 && !rq.floor_log && n_cat_batch <= 1 && !p->export_sites;
}

int EvalCtx::stage_prune_nuc() {
  const int64_t B = p->B;
  NucArgs na;
  na.ops = s.ops + (p->programs.empty() ? 0 : p->programs[0].off), na.n_ops = n_ops;
  na.S_pad = s.S_pad, na.L = (int)p->L, na.root_inode = (int)p->I - 1;
  na.P = s.Prow + (size_t)cat * B * 16, na.PT = s.Prow + ((size_t)p->C * B + (size_t)cat * B) * 16;
  na.codes = s.codes, na.ambig = s.ambig, na.pi = s.pi, na.freq = s.freq, na.pin = s.pin;
  na.pin_leaf = (p->pin_node >= 0 && p->pin_node < p->L) ? (int)p->pin_node : -1;
  na.pin_inode = p->pin_node >= p->L ? (int)(p->pin_node - p->L) : -1;
  na.partials = s.partials + (size_t)cat * s.partial_stride, na.counts = s.counts + (size_t)cat * p->I * s.S_pad;
  na.site_lik = site_lik(), na.site_cnt = site_cnt();
  na.wg_sum = s.wg_sum, na.wg_cnt = s.wg_cnt, na.wg_flag = s.wg_flag;
  if (p->mode == 1) {  // the trunk of a class-compressed partition (repeats.hip): generalised leaves, one leaf per entry
    const hyphy_hip_partition::View &v = p->vw();
    na.L = v.L, na.root_inode = v.I - 1;
    na.codes = s.rep_codes_tile;   // (4 states: row-major [view leaf][pattern])
    na.PT = nullptr;               // (prune_nuc_kernel)
    na.leaf_tab = s.rep_leaf;
    na.gtab = s.rep_tab + (size_t)cat * s.rep_rows * 4, na.gcnt = s.rep_cnt + (size_t)cat * s.rep_rows;
  }
  const PruneForm nf = prune_nuc_form(na, have_folded);
  n_wg = nf.n_wg;
  if (sw::fused_reduce() != 0 && p->mode == 0 && fused_combine_allowed() && (use_gen ? p->nucgen_small : (n_ops > 0 && nf.can_fuse)))
    wire_fused_combine(na, s.wg_flag + (size_t)p->C * s.wg_cap + 3);  // (the spare words behind the flags; zeroed at creation)
  const ExpmArgs *folded = have_folded ? &folded_expm : nullptr;
  if (!(use_gen && nucgen_launch(p->nucgen_key, na, s.stream, p->nucgen_small, (int)p->B, folded))) {
    if (use_gen) return fail("internal: the generated 4-state kernel could not be launched");
    if (launch_prune_nuc(na, s.stream, folded)) return fail("internal: no 4-state pruning kernel for this launch form");
  }
  s.last_nucgen = use_gen;
  if (folded && folded->templates && guard_coeff_slot()) return -1;  // (the ring slot is read by THIS launch)
  return 0;
}

// HYPHY_HIP_TIMELINE (tracing only): synchronous dump of the s_memtime stamps of the pruning launches, in the form of the kernel that ran
struct Timeline {
  const char *path;
  bool per_wave;
  size_t waves, n;  // records of the per-wave form; words in all
  long long *buf;
};
int EvalCtx::dump_timeline(const Timeline &tl) {
  std::vector<long long> h(tl.n);
  HIPCHK(hipStreamSynchronize(s.stream));
  HIPCHK(hipMemcpy(h.data(), tl.buf, tl.n * sizeof(long long), hipMemcpyDeviceToHost));
  FILE *f = fopen(tl.path, "w");
  if (!f) return 0;
  if (tl.per_wave) {
    fprintf(f, "# wave t_start t_prologue t_program t_end levels how hw_id xcc_id   (100 MHz ticks; grid = %s)  then shader cycles: "
               "16 phase buckets (prune.hip HYPHY_TR)\n",
            p->chain ? "tiles x classes x sources" : "programs x classes x tiles");
    for (size_t k = 0; k < tl.waves; k++) {
      const long long *r = &h[k * 24];
      fprintf(f, "%zu", k);
      for (int i = 0; i < 24; i++) fprintf(f, " %lld", r[i]);
      fprintf(f, "\n");
    }
  } else {
    fprintf(f, "# wg wave entry flags t_start t_compute_done t_after_barrier t_finalised\n");
    for (int b = 0; b < kTraceWG; b++)
      for (int w = 0; w < p->NW; w++)
        for (int o = 0; o < n_ops; o++) {
          const long long *r = &h[(((size_t)b * p->NW + w) * n_ops + o) * 4];
          fprintf(f, "%d %d %d %d %lld %lld %lld %lld\n", b, w, o, o < (int)p->ops_host.size() ? (p->ops_host[o].x & 0xff) : 0, r[0], r[1], r[2], r[3]);
        }
  }
  fclose(f);
  return 0;
}

int EvalCtx::stage_prune_mfma() {
  PruneArgs pa = prune_args_current(p, s, cat, n_cat_batch);
  const size_t tl_waves = (size_t)s.ntiles * std::max(1, n_cat_batch) * std::max<size_t>(1, p->programs.size());
  const bool per_wave = prune_form(pa).inst.family == PruneFamily::wave;  // (the kernel that will write the trace buffer: the timeline does not change the family)
  Timeline tl{sw::timeline(), per_wave, tl_waves, per_wave ? tl_waves * 24 : (size_t)kTraceWG * p->NW * std::max(1, n_ops) * 4, nullptr};
  Blocks tl_blk;  // (back to the pool behind the dump)
  if (tl.path && n_ops > 0 && s.T == 1) {
    HIPCHK(tl_blk.get(&tl.buf, tl.n));
    HIPCHK(hipMemsetAsync(tl.buf, 0, tl.n * sizeof(long long), s.stream));
    pa.timeline = tl.buf;
  }
  const PruneForm pf = prune_form(pa);  // (with the timeline, before the combine's target: can_fuse says whether to set one)
  n_wg = pf.n_wg;
  // The fused combine saves 1.5-3 us per evaluation of a small shard (below two tiles per CU; 64 x 1 250: 69.1 -> 67.7 us, 32 x 5 000:
  // 79.8 -> 77.0); at the headline size the gain shrinks to ~1 us while the pruning kernel's own duration grows by the 3-4 us of the
  // serial tail, so larger shards keep the separate kernel.  HYPHY_HIP_FUSED_REDUCE=0/1 forces either.
  const int fuse_forced = sw::fused_reduce();
  const bool walk = trunk_walk_applies(p, s) && !pa.timeline && n_ops > 0;  // (the trunk as one row-split walk per tile, repeats.hip)
  const bool fuse_on = fuse_forced >= 0 ? fuse_forced != 0 : s.ntiles <= 2 * s.cus;  // (the walk at the headline: 90.0 / 89.8 us fused, 88.3 / 89.5 not)
  if (fuse_on && fused_combine_allowed() && !pa.timeline &&
      (walk ? (trunk_walk_fuses_reduce(p) && !sw::walk_timeline()) : pf.can_fuse)) {
    wire_fused_combine(pa, s.frag_ctr + (size_t)p->C * (p->I + 2) * s.ntiles - 1);  // (a word of the arrival counters no schedule indexes; zero between launches)
    pa.red_n = n_wg;
  }
  if (launch_prune_current(p, s, cat, n_cat_batch, &pa, walk)) return -1;
  return pa.timeline ? dump_timeline(tl) : 0;
}

int EvalCtx::stage_export() {
  s.exported = 0;
  if (!(p->export_sites && rq.reduce && !rq.floor_log && n_cat_batch <= 1 && s.d_export)) return 0;
  // per-pattern results for the caller, in ITS order, into host-mapped memory — in front of the kernel that publishes the result
  // record, so that the record's sequence word says they have landed too
  launch_site_export(site_lik(), site_cnt(), s.d_inv, (int)s.S, (p->export_sites & 1) ? s.d_export : nullptr,
                     (p->export_sites & 2) ? reinterpret_cast<long long *>(s.d_export + s.S) : nullptr, s.stream);
  s.exported = p->export_sites;
  return 0;
}

int EvalCtx::stage_reduce() {
  if (rq.reduce && !fused_reduce) {
    // synchronous entry points: the result record goes straight to host-mapped pinned memory (a
    // posted PCIe write from the kernel) — an SDMA device-to-host copy after the kernels costs far more
    double *const d_logl_out = rq.d_logl_out, *rec = s.d_hout ? s.d_hout : s.out;
    double *o0 = d_logl_out ? d_logl_out : rec, *o1 = d_logl_out ? s.out + 1 : rec + 1;
    const int *st = d_logl_out ? nullptr : s.status;
    const double seq = next_seq(s, !d_logl_out);
    hyphy_hip_partition::ReduceForm form;
    if (n_ops > 0 && !rq.floor_log)  // the pruning kernel left per-workgroup partial sums
      form = {launch_wg_reduce(s.wg_sum, s.wg_cnt, s.wg_flag, n_wg, o0, o1, st, s.stream, seq), n_wg, false};
    else {  // nothing was recomputed (or category mode): reduce the stored per-pattern values
      launch_site_reduce(site_lik(), site_cnt(), s.freq, s.S_pad, rq.floor_log ? 1 : 0, o0, o1, st, s.stream, seq);
      form = {"site", s.S_pad, rq.floor_log};
    }
    if (&s == &p->shards[0]) p->last_reduce = form;
  }
  if (p->all_timings) HIPCHK(hipEventRecord(s.ev[3], s.stream));
  HIPCHK(hipGetLastError());
  tr.lap("reduce+events");
  return 0;
}

int EvalCtx::enqueue_eval() {
  if (stage_schedule() || stage_pi()) return -1;
  stage_gen_decision();
  if (rq.n_q > 0) {
    if (stage_slot_table()) return -1;
    if (rq.mix ? stage_expm_mixture() : stage_expm_plain()) return -1;
  }
  if (stage_stamps_open()) return -1;
  if (p->mode == 1 && rep_launch(p, s, cat)) return -1;  // lower phase: the class tables this pass recomputes
  if (p->nuc ? stage_prune_nuc() : stage_prune_mfma()) return -1;
  if (stage_stamps_close()) return -1;
  return stage_export() || stage_reduce() ? -1 : 0;
}

bool same_update(const hyphy_hip_partition *p, const int64_t *u, int64_t n, bool full) {
  if (!p->cached_valid) return false;
  if (full && p->cached_full) return true;
  if (full != p->cached_full) return false;
  if ((int64_t)p->cached_update.size() != n) return false;
  return n == 0 || memcmp(p->cached_update.data(), u, n * sizeof(int64_t)) == 0;
}

int prepare_schedule(hyphy_hip_partition *p, int cat, const int64_t *update_nodes, int64_t n_update, bool *changed,
                     bool force_persist, const int64_t *q_nodes, int64_t n_q, int n_classes) {
  bool full = !p->initialized[cat];
  if (!full && n_update >= p->B) full = true;
  const bool requested_full = full;
  bool persist_all = true;
  const std::vector<char> &res = p->mode == 1 ? p->rep_resident : p->resident;  // (each view keeps its own copies)
  // a partial update needs current persisted copies of EVERY class it walks: promote to a persisting full pass.  (A class batch is
  // keyed on class 0, but after a lazy batched full pass a one-class update restores that class's copies alone: the batch that
  // follows must not take class 0's word for the others.)
  bool stale = false;
  for (int c = cat; c < cat + n_classes && c < (int)res.size(); c++) stale = stale || !res[c];
  if (!full && stale) full = true;
  else if (full && p->initialized[cat] && p->cache_policy == 1 && p->last_full[cat] && !force_persist)
    persist_all = false;
  p->sched_full = full;
  p->sched_persist = persist_all;
  p->last_full[cat] = requested_full ? 1 : 0;
  std::vector<int64_t> view_update;
  if (p->mode == 1) {  // class tables to recompute (item queues on the device), and the trunk's own update list
    if (rep_prepare_pass(p, update_nodes, n_update, q_nodes, n_q, full, cat, n_classes, view_update)) return -1;
  }
  if (same_update(p, update_nodes, n_update, full) && p->cached_persist == persist_all) {
    *changed = false;
    return 0;
  }
  if (p->mode == 1) build_schedule(p, view_update.data(), (int64_t)view_update.size(), full);
  else build_schedule(p, update_nodes, n_update, full);
  if (p->ops_host.size() > ops_capacity(p)) return fail("internal: schedule overflow");
  p->cached_update.assign(update_nodes, update_nodes + (full ? 0 : n_update));
  p->cached_full = full;
  p->cached_persist = persist_all;
  p->cached_valid = 1;
  *changed = true;
  // (nucgen.hip) the key of this schedule's generated kernel: full passes of a 4-state partition under its own tree
  // (small-shard form — matrices in LDS, exponentials and final combine inside the launch — for shards of at most two workgroups
  //  per CU: the interpreter's LP rule; HYPHY_HIP_NUCGEN_SMALL=0/1 forces either)
  p->nucgen_small = !p->shards.empty() && p->shards[0].S_pad / 256 <= 2 * p->shards[0].cus && p->B <= 1024;
  if (const int f = sw::nucgen_small(); f >= 0) p->nucgen_small = f != 0 && p->B <= 1024;
  p->nucgen_key = (p->nuc && p->mode == 0 && full && p->programs.size() == 1 && p->L <= 256)
                      ? nucgen_key(p->ops_host.data() + p->programs[0].off, p->programs[0].n, (int)p->L, !persist_all, p->nucgen_small, (int)p->B) : 0;
  p->nucgen_uses = 0;
  p->nucgen_asked = false;
  return 0;
}

}  // namespace

// Wait for every shard and read its host-mapped result record [log-L, scaler sum, status].
int collect_status(hyphy_hip_partition *p) {
  const bool expm_prof = sw::expm_prof();
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    if (!s.d_hout) HIPCHK(hipMemcpyAsync(s.h_out, s.out, 3 * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    if (s.seq_wait != 0. && s.d_hout && !expm_prof) {
      // the last kernel of the evaluation publishes the sequence number after the record (system-scope fence)
      volatile double *flag = s.h_out + 3;
      bool seen = false;
      for (long spins = 1; !seen; spins++) {
        seen = *flag == s.seq_wait;
        if (!seen && (spins & 0x3fff) == 0) {  // every few tens of microseconds: has the stream died or finished?
          const hipError_t q = hipStreamQuery(s.stream);
          if (q == hipSuccess) {
            seen = *flag == s.seq_wait;
            break;
          }
          if (q != hipErrorNotReady) return fail(std::string("stream failed: ") + hipGetErrorString(q));
        }
      }
      s.seq_wait = 0.;
      if (!seen) HIPCHK(hipStreamSynchronize(s.stream));
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
    } else {
      HIPCHK(hipStreamSynchronize(s.stream));
    }
    if (expm_prof) {
      long long t[8];
      expm_read_profile(t);
      fprintf(stderr, "[hyphy_hip] expm phases (cycles): Q build %lld, norms %lld, Taylor %lld, squarings %lld, store %lld, images %lld\n",
              t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5]);
    }
    if (s.h_out[2] != 0.) {
      hipMemsetAsync(s.status, 0, sizeof(int32_t), s.stream);
      return fail("Failed to compute a valid transition matrix; this is usually caused by ill-conditioned rate "
                  "matrices (e.g. very large rate values)");
    }
  }
  return 0;
}

void record_timings(hyphy_hip_partition *p) {
  Shard &s = p->shards[0];
  float t;
  for (int k = 0; k < 3; k++) {
    t = 0.f;
    if (k == 1) {  // the pruning interval of THIS evaluation, or 0 when it carried no stamp (one evaluation in
                   // HYPHY_HIP_TIMING_EVERY does; hyphy_hip_set_timing_detail stamps every one) — never an older evaluation's
      p->timings[1] = 0.;
      if (s.last_stamped && s.ring_count > 0) {
        const size_t slot = (size_t)((s.ring_count - 1) % kTimingRing) * 2;
        if (hipEventElapsedTime(&t, s.ring[slot], s.ring[slot + 1]) == hipSuccess) p->timings[1] = t;
      }
      continue;
    }
    if (!p->all_timings) continue;
    if (hipEventElapsedTime(&t, s.ev[k], s.ev[k + 1]) == hipSuccess) p->timings[k] = t;
  }
}

// sum of shard partials exactly as ComputeBlock combines its thread blocks (Neumaier,
// likefunc.cpp:11046-11093)
double combine(const std::vector<double> &parts) {
  if (parts.size() == 1) return parts[0];
  double sum = 0., corr = 0.;
  for (double r : parts) {
    if (r != r) return r;
    if (r == -INFINITY) return -INFINITY;
    double t = sum + r;
    if (sum < r) corr += (sum - t) + r;
    else corr += (r - t) + sum;
    sum = t;
  }
  return sum + corr;
}

namespace {

// A synchronous evaluation that returns per-pattern results asks for the export in front of its enqueue (single-device partitions;
// HYPHY_HIP_SITE_EXPORT=0 keeps the copies of gather_sites) ...
int begin_site_export(hyphy_hip_partition *p, bool want_lik, bool want_cnt) {
  if (!p) return 0;
  p->export_sites = 0;
  if (!sw::site_export() || p->shards.size() != 1 || !(want_lik || want_cnt)) return 0;
  Shard &s = p->shards[0];
  if (s.S <= 0 || s.s0 != 0) return 0;
  HIPCHK(hipSetDevice(s.device));
  if (!s.h_export && !s.export_failed) {
    // (the pattern-order map first — a partition whose patterns are sorted must never export without it, and a failed
    //  allocation must not leave a half-initialised export behind: on any failure this partition keeps the copies of gather_sites)
    bool ok = s.own.get_group({device_block(s.d_inv, p->perm.empty() ? 0 : (size_t)s.S * sizeof(int32_t)),
                               pinned_block(s.h_export, (size_t)s.S * 2 * sizeof(double))}) == hipSuccess;
    if (ok && !p->perm.empty()) {
      std::vector<int32_t> inv((size_t)s.S, 0);
      for (int64_t j = 0; j < s.S; j++) inv[(size_t)p->perm[(size_t)j]] = (int32_t)j;
      ok = hipMemcpy(s.d_inv, inv.data(), inv.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && hipHostGetDevicePointer((void **)&s.d_export, s.h_export, 0) == hipSuccess && s.d_export;
    if (!ok) {
      (void)hipGetLastError();
      s.own.drop(s.d_inv, FreeMode::Sync);
      s.own.drop(s.h_export, FreeMode::Sync);
      s.d_export = nullptr;
      s.export_failed = true;
      return 0;
    }
  }
  if (!s.d_export || (!p->perm.empty() && !s.d_inv)) return 0;
  p->export_sites = (want_lik ? 1 : 0) | (want_cnt ? 2 : 0);
  return 0;
}
int gather_sites(hyphy_hip_partition *p, int cat, double *site_lik_out, int64_t *site_scaler_out, bool mixed) {
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    const double *lik = mixed ? s.mixed_lik : s.site_lik + (size_t)cat * s.S_pad;
    const int32_t *cn = mixed ? s.mixed_cnt : s.site_cnt + (size_t)cat * s.S_pad;
    // both arrays through ONE pinned staging block and one wait (r04; was: two pageable temporaries, a wait behind each copy —
    // a host that mixes rate classes itself asks for these once per class and evaluation)
    if (!s.h_site) HIPCHK(s.own.get(pinned_block(s.h_site, (size_t)s.S_pad * (sizeof(double) + sizeof(int32_t)))));
    double *hl = s.h_site;
    int32_t *hc = reinterpret_cast<int32_t *>(s.h_site + s.S_pad);
    if (site_lik_out) HIPCHK(hipMemcpyAsync(hl, lik, s.S * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    if (site_scaler_out) HIPCHK(hipMemcpyAsync(hc, cn, s.S * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (site_lik_out) {
      if (p->perm.empty()) memcpy(site_lik_out + s.s0, hl, s.S * sizeof(double));
      else  // the device keeps its patterns sorted: scatter back into the caller's order
        for (int64_t k = 0; k < s.S; k++) site_lik_out[p->perm[s.s0 + k]] = hl[k];
    }
    if (site_scaler_out)
      for (int64_t k = 0; k < s.S; k++) site_scaler_out[caller_pattern(p, s.s0 + k)] = hc[k];
  }
  return 0;
}

// ... (begin_site_export) and collects them behind the wait for the result record (whatever was not exported comes through gather_sites)
int finish_sites(hyphy_hip_partition *p, int cat, double *site_lik_out, int64_t *site_scaler_out) {
  p->export_sites = 0;
  if (!site_lik_out && !site_scaler_out) return 0;
  Shard &s = p->shards[0];
  const int have = p->shards.size() == 1 ? s.exported : 0;
  s.exported = 0;
  const bool lik_ok = !site_lik_out || (have & 1), cnt_ok = !site_scaler_out || (have & 2);
  if (!(lik_ok && cnt_ok)) return gather_sites(p, cat, site_lik_out, site_scaler_out, false);
  if (site_lik_out) memcpy(site_lik_out, s.h_export, (size_t)s.S * sizeof(double));
  if (site_scaler_out) memcpy(site_scaler_out, s.h_export + s.S, (size_t)s.S * sizeof(int64_t));
  return 0;
}

// The tail of a synchronous entry point: wait for every shard's record, combine, hand out per-pattern values — each in the caller's way:
enum TailCombine { kCombineShards, kCombineHost };  // combine_shards (comm.hip) as HYPHY_HIP_COMBINE says / the host's sum whatever it says
enum TailTimings { kNoTimings, kRecordTimings };    // record_timings behind the wait
enum TailSites { kSitesExported, kSitesGathered, kSitesGatheredMixed };  // finish_sites (export, else copies) / copies of the class's values / of the mixed ones
int result_tail(hyphy_hip_partition *p, int cat, TailCombine comb, TailTimings tim, TailSites sites, double *logl_out,
                double *site_lik_out, int64_t *site_scaler_out) {
  if (collect_status(p)) return -1;
  if (tim == kRecordTimings) record_timings(p);
  if (combine_shards(p, logl_out, comb == kCombineShards)) return -1;
  if (sites == kSitesExported) return finish_sites(p, cat, site_lik_out, site_scaler_out);
  if (site_lik_out || site_scaler_out) return gather_sites(p, cat, site_lik_out, site_scaler_out, sites == kSitesGatheredMixed);
  return 0;
}

// Category mode behind the per-class passes: weights to the device (`always`, or when they changed), mix the classes, reduce the mix
// (`staged`: the weights sit at the head of every shard's pinned class-mixture staging — prepare_class_mixture_staging — and are
//  copied from there in-stream at every call, without a wait)
int mix_and_reduce_categories(hyphy_hip_partition *p, const double *weights, bool always, bool staged = false) {
  const bool w_changed = always || p->cached_weights.size() != (size_t)p->C || memcmp(p->cached_weights.data(), weights, p->C * sizeof(double));
  if (w_changed) p->cached_weights.assign(weights, weights + p->C);
  if (staged) p->cached_weights.clear();  // (known again once every shard's copy is queued)
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    if (staged) {
      s.mixst_inflight = true;
      HIPCHK(hipMemcpyAsync(s.weights, s.h_mixst, (size_t)p->C * sizeof(double), hipMemcpyHostToDevice, s.stream));
    } else if (w_changed && upload_small(s, weights, (size_t)p->C, s.weights)) {
      if (!always) p->cached_weights.clear();  // (the always-uploading entry point never cleared the cache on this path: kept)
      return -1;
    }
    launch_mix_categories(s.site_lik, s.site_cnt, s.weights, (int)p->C, s.S_pad, s.mixed_lik, s.mixed_cnt, s.stream);
    double *rec = s.d_hout ? s.d_hout : s.out;
    launch_site_reduce(s.mixed_lik, s.mixed_cnt, s.freq, s.S_pad, 1, rec, rec + 1, s.status, s.stream, next_seq(s, rec == s.d_hout));
    if (&s == &p->shards[0]) p->last_reduce = {"site", s.S_pad, true};
  }
  if (staged) p->cached_weights.assign(weights, weights + p->C);
  return 0;
}

// The pinned staging of a class-batched mixture call on every shard, for `n_w` mixture weights, with the class weights at its head.
// A copy out of it can still be queued only behind a call that failed before its wait: then, and when the block grows, the stream is
// waited for; in steady state nothing here waits.
int prepare_class_mixture_staging(hyphy_hip_partition *p, size_t n_w, const double *class_weights) {
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    if (s.mixst_inflight) {
      HIPCHK(hipStreamSynchronize(s.stream));
      s.mixst_inflight = false;
    }
    if (!s.h_mixst || s.mixst_cap < n_w) {
      const size_t cap = std::max(n_w, (size_t)(2 * p->B));
      s.mix_counts_dev.clear();
      HIPCHK(s.own.regrow({pinned_block(s.h_mixst, (mixst_weights_at(p) + cap) * sizeof(double))}, s.mixst_cap, n_w + 1, cap, FreeMode::Sync));
    }
    memcpy(s.h_mixst, class_weights, (size_t)p->C * sizeof(double));
  }
  return 0;
}
void class_mixture_staging_done(hyphy_hip_partition *p) {  // (behind the wait for every shard's result record)
  for (Shard &s : p->shards) s.mixst_inflight = false;
}

// ---- hyphy_hip_create, step by step --------------------------------------------------------------------------------------------
struct CreateInput {
  int64_t D, S, L, I, C;
  const int64_t *flat_parents, *leaf_codes;
  const double *ambig;
  int64_t n_ambig;
  const int64_t *pattern_freq;
};

// Step 1: the arguments and the tree.  0: *out is the partition (no shard yet) and *nshards says how many it gets; else hyphy_hip_create's result.
int checked_partition(const CreateInput &in, int device_first, int device_count, hyphy_hip_partition **out, int *nshards_out) {
  const int64_t D = in.D, S = in.S, L = in.L, I = in.I, C = in.C;
  if (D < 2 || D > 64) {
    g_last_error = "unsupported state count (this version: 2 <= D <= 64)";
    return 1;
  }
  if (S < 1 || L < 2 || I < 1 || C < 1 || !in.flat_parents || !in.leaf_codes || !in.pattern_freq)
    return fail("invalid partition dimensions / null input");
  if (L > 65535) {
    g_last_error = "more than 65535 leaves: packed schedule entries unsupported in this version";
    return 1;
  }
  if (in.n_ambig > 32767) {
    g_last_error = "too many distinct ambiguity vectors for the packed leaf table";
    return 1;
  }
  int ndev = hyphy_hip_device_count();
  if (ndev <= 0) return fail("no HIP device available (this library has no CPU fallback)");
  const int force = sw::force_shards();
  if (device_count < 1) device_count = 1;
  if (!force && (device_first < 0 || device_first + device_count > ndev)) return fail("device range out of bounds");
  if (force > 0 && device_first >= ndev) return fail("device out of bounds");
  int nshards = force > 0 ? force : device_count;
  if ((int64_t)nshards > S) nshards = (int)S;
  *nshards_out = nshards;

  hyphy_hip_partition *p = new hyphy_hip_partition();
  p->D = D; p->S = S; p->L = L; p->I = I; p->C = C; p->B = L + I - 1;
  p->nuc = (D == 4);
  p->NW = (int)((D + 15) / 16);
  p->DP = 16 * p->NW;
  p->parents.assign(in.flat_parents, in.flat_parents + L + I);
  p->children.assign(I, std::vector<int>());
  int roots = 0;
  for (int64_t n = 0; n < L + I; n++) {
    int64_t par = in.flat_parents[n];
    if (par < 0) { roots++; continue; }
    if (par >= I || (n >= L && par <= n - L)) { delete p; return fail("flat_parents is not a post-order tree"); }
    p->children[par].push_back((int)n);
  }
  if (roots != 1 || in.flat_parents[L + I - 1] != -1) { delete p; return fail("root must be the last internal node"); }
  for (int64_t k = 0; k < L * S; k++)
    if (in.leaf_codes[k] >= D || in.leaf_codes[k] < -in.n_ambig) { delete p; return fail("leaf code out of range"); }
  p->initialized.assign(C, 0);
  p->bc_node.assign(C, -1);
  p->bc_use_pi.assign(C, 0);
  p->resident.assign(C, 0);
  p->pin_left.assign(C, std::vector<int64_t>());
  p->last_full.assign(C, 0);
  p->cache_policy = sw::cache_always() ? 0 : 1;
  p->leaf_has_ambig.assign(L, 0);
  for (int64_t l = 0; l < L; l++)
    for (int64_t k = 0; k < S; k++)
      if (in.leaf_codes[l * S + k] < 0) {
        p->leaf_has_ambig[l] = 1;
        break;
      }
  *out = p;
  return 0;
}

// Step 2: a shard's geometry and the kernel its size asks for.  Host arithmetic only: of the device it needs the CU count.
void shard_geometry(hyphy_hip_partition *p, Shard &s, int cus) {
  const int64_t L = p->L, I = p->I;
  const int DP = p->DP;
  const int tiles_override = sw::tiles();
  const int64_t tiles = (s.S + 15) / 16;
  int T = 1;
  if (!p->nuc) {
    // T = 1 everywhere the wave-per-tile kernel applies (any shard of >= 1.75 tiles per CU: measured 2.3x
    // faster than the T = 2 workgroup kernel at 128 taxa x 100k codons, 2 718 vs 6 190 us); T > 1 only beyond
    // the grid limit of 65 535 tiles
    T = tiles <= 65535 ? 1 : (tiles <= 2 * 65535 ? 2 : 4);
    if (tiles_override >= 1 && tiles_override <= 4) T = tiles_override;
  }
  s.T = T;
  s.cus = cus;
  if (p->nuc) p->n_slots = 2 + kNucParkSlots;  // (prune_nuc_kernel parks pending nodes in LDS)
  if (p->nuc) p->nuc_leaf_pairs = prune_nuc_takes_leaf_pairs((int)L);
  if (!p->nuc) {
    // Kernel choice (measured, tools/sweep_small_shards.sh): the wave-per-tile kernel (no cross-wave
    // exchange, child -> parent through registers) wins once every SIMD holds ~2 waves of it — 160 vs 183 us
    // at 624 tiles; below that its 64-MFMA-per-edge chains are pure latency (167 us at 312 tiles as at
    // 624) and the workgroup-per-tile kernel, which splits a tile's rows over four waves, is faster
    // (123 us at 312 tiles, 63 us at 78).
    // (r02: with chain schedules the wave-per-tile kernel also wins at a rank's share of the headline workload —
    //  89 vs 118 us at 312 tiles, 52 vs 61 us at 78; below ~a quarter tile per CU the row-split workgroup kernel
    //  keeps its shorter critical path.  The schedule tuner re-checks the choice on the first steady-state pass.)
    p->variant = tiles >= (int64_t)cus / 4 ? 1 : 0;
    p->kernel_forced = false;
    if (const int k = sw::kernel(); k >= 0) {  // (diagnostic override)
      p->variant = k;  // 0: workgroup per tile, 1: wave per tile, 2: workgroup per tile on chain schedules
      p->kernel_forced = true;
    }
    if (T != 1) {
      p->variant = 0;
      p->kernel_forced = true;
    }
    // two "exchange" ids (register hand-over) + wave-private LDS parking slots: two where two tiles + the leaf codes fit an
    // eighth of the CU's 160 KiB (eight waves per CU stay resident: 61 states up to 128 taxa), else one
    {
      const size_t tile_bytes = (size_t)p->NW * 4 * 64 * sizeof(double), codes_bytes = (size_t)p->L * 16 * sizeof(int16_t);
      p->n_slots_wave = 2 * tile_bytes + codes_bytes <= 20480 ? 4 : 3;
    }
    if (const int n = sw::slots()) p->n_slots_wave = n;
    p->n_slots = p->variant == 1 ? p->n_slots_wave : lds_slots(T);
  }
  if (p->nuc) {
    s.S_pad = (int)((s.S + 511) / 512 * 512);  // (prune_nuc2_kernel: 256 threads x 2 patterns per workgroup)
    s.ntiles = 0;
    s.partial_stride = (size_t)I * 4 * s.S_pad;
  } else {
    s.ntiles = (int)((tiles + T - 1) / T * T);
    s.S_pad = s.ntiles * 16;
    s.partial_stride = (size_t)I * s.ntiles * 16 * DP;
  }
  s.wg_cap = p->nuc ? (s.S_pad + 255) / 256 : s.ntiles;
  s.h_small_cap = (size_t)std::max<int64_t>(std::max<int64_t>(DP, p->C), 64);
}

// Step 3: the stream, the events and every block a shard holds from creation on, as one table.  -1: fail() has said which is missing.
int allocate_shard(hyphy_hip_partition *p, Shard &s, int64_t n_ambig) {
  const int64_t D = p->D, L = p->L, I = p->I, C = p->C, B = p->B;
  const int DP = p->DP;
  const size_t mfma = p->nuc ? 0 : 1, nuc = p->nuc ? 1 : 0;  // (a row of no bytes is no block: the field stays null)
  // (+2 node slots per class behind the last class: outside vector of the cached branch and a scratch slot, see
  //  hyphy_hip_branch_cache_build)
  const size_t node_stride = p->nuc ? (size_t)4 * s.S_pad : (size_t)s.ntiles * 16 * DP;
  const size_t wg_rows = (size_t)C * s.wg_cap + 4;  // x C: rate-class batching writes one row per class; + 4: the fused final combine reads them with 16-byte loads
  pool_stream_get(&s.own_stream);
  s.stream = s.own_stream;
  for (auto &e : s.ev) hipEventCreate(&e);
  s.ring.assign(2 * kTimingRing, nullptr);
  const BlockReq table[] = {
      device_block(s.codes, (size_t)L * s.S_pad * sizeof(int16_t), "s.codes"),
      device_block(s.codes_tile, mfma * L * s.S_pad * sizeof(int16_t), "s.codes_tile"),
      device_block(s.expm_need, mfma * B, "s.expm_need"),
      device_block(s.bc_ops, mfma * ops_capacity(p) * sizeof(int4), "s.bc_ops"),
      device_block(s.bc_prog, mfma * sizeof(int4), "s.bc_prog"),
      device_block(s.bc_slot, mfma * C * sizeof(int32_t), "s.bc_slot"),
      device_block(s.bc_q, mfma * D * D * sizeof(double), "s.bc_q"),
      device_block(s.freq, (size_t)s.S_pad * sizeof(double), "s.freq"),
      device_block(s.pin, (size_t)s.S_pad * sizeof(int16_t), "s.pin"),
      device_block(s.ambig, (size_t)std::max<int64_t>(1, n_ambig) * DP * sizeof(double), "s.ambig"),
      device_block(s.partials, ((size_t)C * s.partial_stride + 2 * C * node_stride) * sizeof(double), "s.partials"),
      device_block(s.counts, ((size_t)C * I + 2 * C) * s.S_pad * sizeof(int32_t), "s.counts"),
      device_block(s.site_lik, (size_t)C * s.S_pad * sizeof(double), "s.site_lik"),
      device_block(s.site_cnt, (size_t)C * s.S_pad * sizeof(int32_t), "s.site_cnt"),
      device_block(s.mixed_lik, (size_t)s.S_pad * sizeof(double), "s.mixed_lik"),
      device_block(s.mixed_cnt, (size_t)s.S_pad * sizeof(int32_t), "s.mixed_cnt"),
      device_block(s.Prow, nuc * 2 * C * B * 16 * sizeof(double), "s.Prow"),  // row-major, then transposed (prune_nuc2_kernel)
      // (+ transposed path matrices of the branch cache, + twins of re-rooted schedules)
      device_block(s.Pfrag, mfma * ((size_t)C * B + (size_t)C * (I + 2) + kMaxTwin) * DP * DP * sizeof(double), "s.Pfrag"),
      device_block(s.pi_ones, mfma * DP * sizeof(double), "s.pi_ones"),
      device_block(s.PTg, mfma * C * B * DP * DP * sizeof(double), "s.PTg"),
      device_block(s.qbuf, (size_t)C * B * D * D * sizeof(double), "s.qbuf"),
      device_block(s.slots, (size_t)C * B * sizeof(int32_t), "s.slots"),
      device_block(s.ops, ops_capacity(p) * sizeof(int4), "s.ops"),
      device_block(s.prog, (size_t)(I + 2) * sizeof(int4), "s.prog"),
      device_block(s.jn, (size_t)(I + 2) * sizeof(int4), "s.jn"),
      device_block(s.frag_ctr, mfma * C * (I + 2) * s.ntiles * sizeof(int), "s.frag_ctr"),
      device_block(s.hand_cnt, mfma * C * I * s.ntiles * 32 * sizeof(int32_t), "s.hand_cnt"),
      device_block(s.pi, (size_t)DP * sizeof(double), "s.pi"),
      device_block(s.out, 4 * sizeof(double), "s.out"),        // device-side result record [log-L, scaler sum, status copy, pad]
      device_block(s.status, sizeof(int32_t), "s.status"),     // set by the expm kernel when a matrix fails
      device_block(s.weights, (size_t)C * sizeof(double), "s.weights"),
      device_block(s.wg_sum, wg_rows * sizeof(double), "s.wg_sum"),
      device_block(s.wg_cnt, wg_rows * sizeof(long long), "s.wg_cnt"),
      device_block(s.wg_flag, wg_rows * sizeof(int), "s.wg_flag"),
      pinned_block(s.h_ops, ops_capacity(p) * sizeof(int4)),
      pinned_block(s.h_prog, (size_t)(I + 2) * sizeof(int4)),
      pinned_block(s.h_jn, (size_t)(I + 2) * sizeof(int4)),
      pinned_block(s.h_out, 4 * sizeof(double)),
      pinned_block(s.h_slots, (size_t)C * B * sizeof(int32_t)),
      pinned_block(s.h_small, s.h_small_cap * sizeof(double))};
  const BlockReq *missing = nullptr;
  if (s.own.get_group(table, sizeof table / sizeof table[0], &missing) != hipSuccess)
    return fail(missing->pinned ? std::string("hipHostMalloc failed") : std::string("hipMalloc failed (") + missing->name + ")");
  // HYPHY_HIP_POISON=1 (tests): fill every fresh allocation with 0xff bytes (NaN / -1), so that anything read before
  // it is written shows up even in a process whose recycled device memory happens to hold zeros
  if (sw::poison())
    for (const BlockReq &b : table)
      if (*b.field && !b.pinned && !sw::nopoison(b.name)) {
        hipMemset(*b.field, 0xff, b.bytes);
        hipDeviceSynchronize();
      }
  return 0;
}

// Step 4: what the blocks hold before the first evaluation.  `codes_out`: the leaf table in device pattern order ([L][S_pad]; padding
// patterns use state 0, weight 0), which the class computation of subtree repeats reads.
void upload_shard(hyphy_hip_partition *p, Shard &s, const CreateInput &in, std::vector<int16_t> &codes) {
  const int64_t D = p->D, S = p->S, L = p->L, I = p->I, C = p->C, B = p->B;
  const int DP = p->DP;
  auto src_pattern = [&](int64_t j) -> int64_t { return p->perm.empty() ? j : p->perm[j]; };
  if (!p->nuc) {  // which matrix images a branch's consumers read (ExpmArgs::need): leaves are gathered from by state — the column-gather
                  // image —, internal branches are A operands of edge products; a leaf with ambiguity codes is both
    std::vector<unsigned char> need((size_t)B, 3);
    for (int64_t c = 0; c < L && c < B; c++) need[(size_t)c] = p->leaf_has_ambig[(size_t)c] ? 3 : 2;
    for (int64_t c = L; c < L + I - 1 && c < B; c++) need[(size_t)c] = 1;
    hipMemcpy(s.expm_need, need.data(), (size_t)B, hipMemcpyHostToDevice);
  }
  hipMemset(s.pin, 0, (size_t)s.S_pad * sizeof(int16_t));
  if (!p->nuc) {
    std::vector<double> ones(DP, 0.);
    for (int64_t k = 0; k < D; k++) ones[k] = 1.;
    hipMemcpy(s.pi_ones, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice);
    hipMemset(s.frag_ctr, 0, (size_t)C * (I + 2) * s.ntiles * sizeof(int));
  }
  hipMemset(s.wg_flag + (size_t)C * s.wg_cap, 0, 4 * sizeof(int));  // (the last word: arrival counter of the 4-state kernel's fused combine)
  hipMemsetAsync(s.status, 0, sizeof(int32_t), s.stream);
  if (hipHostGetDevicePointer((void **)&s.d_hout, s.h_out, 0) != hipSuccess) s.d_hout = nullptr;
  for (int k = 0; k < 4; k++) s.h_out[k] = 0.;
  hipMemsetAsync(s.partials, 0, (size_t)C * s.partial_stride * sizeof(double), s.stream);
  hipMemsetAsync(s.counts, 0, (size_t)C * I * s.S_pad * sizeof(int32_t), s.stream);
  hipMemsetAsync(s.site_lik, 0, (size_t)C * s.S_pad * sizeof(double), s.stream);
  hipMemsetAsync(s.site_cnt, 0, (size_t)C * s.S_pad * sizeof(int32_t), s.stream);
  // leaf table: int64 pattern-indexed -> packed int16 [L][S_pad]
  codes.assign((size_t)L * s.S_pad, 0);
  for (int64_t l = 0; l < L; l++)
    for (int64_t k = 0; k < s.S; k++) codes[(size_t)l * s.S_pad + k] = (int16_t)in.leaf_codes[l * S + src_pattern(s.s0 + k)];
  std::vector<double> fr(s.S_pad, 0.0);
  for (int64_t k = 0; k < s.S; k++) fr[k] = (double)in.pattern_freq[src_pattern(s.s0 + k)];
  std::vector<double> amb((size_t)std::max<int64_t>(1, in.n_ambig) * DP, 0.0);
  const int astride = p->nuc ? 4 : DP;
  for (int64_t a = 0; a < in.n_ambig; a++)
    for (int64_t k = 0; k < D; k++) amb[a * astride + k] = in.ambig[a * D + k];
  hipMemcpy(s.codes, codes.data(), codes.size() * sizeof(int16_t), hipMemcpyHostToDevice);
  if (!p->nuc) {  // tile-major copy [tile][L][16] for the wave-per-tile kernels: a tile's codes are one 32 L-byte run
    std::vector<int16_t> ct((size_t)L * s.S_pad, 0);
    for (int64_t l = 0; l < L; l++)
      for (int64_t k = 0; k < s.S_pad; k++) ct[((size_t)(k >> 4) * L + l) * 16 + (k & 15)] = codes[(size_t)l * s.S_pad + k];
    hipMemcpy(s.codes_tile, ct.data(), ct.size() * sizeof(int16_t), hipMemcpyHostToDevice);
  }
  hipMemcpy(s.freq, fr.data(), fr.size() * sizeof(double), hipMemcpyHostToDevice);
  hipMemcpy(s.ambig, amb.data(), amb.size() * sizeof(double), hipMemcpyHostToDevice);
  // (the host copy is only kept for the class computation of subtree repeats)
  if (sw::repeats() == 0) std::vector<int16_t>().swap(codes);
}

}  // namespace

}  // namespace hyhip

extern "C" {

const char *hyphy_hip_last_error(void) { return g_last_error.c_str(); }

int hyphy_hip_prune_launches(hyphy_hip_partition *p) { return p ? (int)std::max<size_t>(1, p->levels.size()) : 0; }

const char *hyphy_hip_last_expm_kernel(void) { return last_expm_kernel(); }

const char *hyphy_hip_prune_kernel_name(const hyphy_hip_partition *p) {
  if (!p) return "";
  if (p->nuc && !p->shards.empty() && p->shards[0].last_nucgen) return "nucgen_kernel";  // (run-time generated, nucgen.hip)
  if (p->nuc) return (p->nuc_leaf_pairs && p->mode == 0) ? "prune_nuc2_kernel" : "prune_nuc_kernel";
  if (p->mode == 1 && !p->shards.empty() && p->shards[0].last_walk) return "trunk_walk_kernel";  // (repeats.hip)
  return p->variant == 1 ? "prune_wave_kernel" : "prune_mfma_kernel";  // (variant 2: the same kernel on a chain schedule)
}

const char *hyphy_hip_last_prune_form(const hyphy_hip_partition *p) {
  if (!p || p->nuc) return "";
  static thread_local std::string out;
  if (p->last_form_walk) return (out = "trunk_walk_kernel NW=" + std::to_string(p->NW)).c_str();
  if (p->last_cut < 0) return "";
  const hyhip::PruneDispatch &d = p->last_dispatch;
  char b[160];
  int n = snprintf(b, sizeof b, "%s NW=%d", d.kernel, d.NW);
  if (d.park >= 0) n += snprintf(b + n, sizeof b - n, " park=%d", d.park);
  else n += snprintf(b + n, sizeof b - n, " T=%d%s", d.T, d.on_chain ? " on-chain" : "");
  if (d.inst[0]) n += snprintf(b + n, sizeof b - n, " %s", d.inst);
  if (p->last_cut > 0) n += snprintf(b + n, sizeof b - n, "; chain m=%d", p->last_cut);
  else n += snprintf(b + n, sizeof b - n, "; levels");
  if (p->last_rerooted) snprintf(b + n, sizeof b - n, "; re-rooted");
  return (out = b).c_str();
}

const char *hyphy_hip_last_reduce_form(const hyphy_hip_partition *p) {
  if (!p || !p->last_reduce.kind[0]) return "";
  static thread_local std::string out;
  const auto &f = p->last_reduce;
  if (!strcmp(f.kind, "hmm")) return (out = p->hmm_form).c_str();  // (shard 0 ran it alone: no host sum behind it)
  out = std::string(f.kind) + (strcmp(f.kind, "site") ? " n=" : " S_pad=") + std::to_string(f.n) + (f.floor ? " floor" : "");
  if (p->shards.size() > 1) out += "; host x" + std::to_string(p->shards.size());
  return out.c_str();
}

int64_t hyphy_hip_prune_timings(hyphy_hip_partition *p, double *out_ms, int64_t n) {
  if (!p || !out_ms || n <= 0 || p->shards.empty()) return 0;
  Shard &s = p->shards[0];
  if (hipSetDevice(s.device) != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess) return 0;
  const int64_t have = (int64_t)std::min<uint64_t>(s.ring_count, (uint64_t)kTimingRing);
  const int64_t m = std::min(n, have);
  for (int64_t k = 0; k < m; k++) {
    const uint64_t idx = s.ring_count - (uint64_t)m + (uint64_t)k;
    const size_t slot = (size_t)(idx % kTimingRing) * 2;
    float t = 0.f;
    if (hipEventElapsedTime(&t, s.ring[slot], s.ring[slot + 1]) != hipSuccess) t = 0.f;
    out_ms[k] = t;
  }
  return m;
}
const char *hyphy_hip_version(void) { return "hyphy_hip 0.1 (gfx950, FP64 MFMA)"; }

int64_t hyphy_hip_plan_switches(char *out, int64_t cap) {
  const std::string t = sw::plan_text();
  const int64_t need = (int64_t)t.size() + 1;  // (with the terminating zero)
  if (!out || cap < need) return -need;
  memcpy(out, t.c_str(), (size_t)need);
  return need;
}

int hyphy_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void hyphy_hip_destroy(hyphy_hip_partition *p) {
  if (!p) return;
  for (Shard &s : p->shards) free_shard(s);
  p->own.drop(p->h_qstage, FreeMode::Sync);
  if (p->xch) hyphy_hip_xch_close(p->xch);
  delete p;
}

int hyphy_hip_create(hyphy_hip_partition **out, int64_t D, int64_t S, int64_t L, int64_t I, int64_t C,
                     const int64_t *flat_parents, const int64_t *leaf_codes, const double *ambig, int64_t n_ambig,
                     const int64_t *pattern_freq, int device_first, int device_count) {
  if (!out) return fail("out == NULL");
  *out = nullptr;
  const CreateInput in = {D, S, L, I, C, flat_parents, leaf_codes, ambig, n_ambig, pattern_freq};
  hyphy_hip_partition *p = nullptr;
  int nshards = 0;
  if (const int r = checked_partition(in, device_first, device_count, &p, &nshards)) return r;
  if (!p->nuc && sw::sort_patterns()) sort_patterns(p, leaf_codes, L, S);
  init_plain_view(p);
  if (!p->nuc && C == 1) reroot_path(p);

  const int force = sw::force_shards();
  int64_t base = S / nshards, rem = S % nshards, s0 = 0;
  p->shards.resize((size_t)nshards);  // (in place before anything is allocated: a shard owns its blocks and does not copy)
  for (int k = 0; k < nshards; k++) {
    Shard &s = p->shards[(size_t)k];
    s.device = force > 0 ? device_first : device_first + k;
    s.s0 = s0;
    s.S = base + (k < rem ? 1 : 0);
    s0 += s.S;
  }
  std::vector<std::vector<int16_t>> shard_codes;  // per shard: the leaf table in device pattern order (class computation below)
  for (Shard &s : p->shards) {
    if (hipSetDevice(s.device) != hipSuccess) { hyphy_hip_destroy(p); return fail("hipSetDevice failed"); }
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, s.device);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      hyphy_hip_destroy(p);
      return fail(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    }
    shard_geometry(p, s, prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
    if (allocate_shard(p, s, n_ambig)) {
      hyphy_hip_destroy(p);
      return -1;
    }
    shard_codes.emplace_back();
    upload_shard(p, s, in, shard_codes.back());
    if (hipStreamSynchronize(s.stream) != hipSuccess || hipGetLastError() != hipSuccess) {
      hyphy_hip_destroy(p);
      return fail("device initialisation failed");
    }
  }
  // subtree repeats: classes, compressed set, trunk view and tables (repeats.hip); leaves rep_on false when it would not pay
  rep_setup(p, shard_codes);  // (never fails the creation: a partition whose tables cannot be set up evaluates plain)
  *out = p;
  return 0;
}

/* Subtree repeats (repeats.hip) are used wherever they pay; `on` = 0 turns them off for this partition (the pruning kernels
 * then walk every node at every pattern), 1 back on.  Same results either way (HYPHY_HIP_REPEATS=0 does the same for
 * every partition created afterwards). */
int hyphy_hip_set_repeats(hyphy_hip_partition *p, int on) {
  if (!p) return fail("partition == NULL");
  if (finish_pending_async(p)) return -1;
  p->rep_enabled = on != 0;
  p->rep_decided = true;  // (the caller's choice stands: no measurement overrides it)
  return 0;
}

/* What the class compression does on this partition's first shard: out[0] available, [1] class tables, [2] table rows (classes
 * padded to tiles of 16: the edge products of the lower phase), [3] / [4] internal nodes / leaves of the trunk, [5] edge
 * products one full pass executes with repeats on, [6] ... with repeats off (every internal edge at every pattern), [7] in use. */
int hyphy_hip_repeat_stats(const hyphy_hip_partition *p, int64_t out[8]) {
  if (!p || !out) return fail("null argument");
  for (int k = 0; k < 8; k++) out[k] = 0;
  const Shard &s = p->shards[0];
  out[6] = (p->I - 1) * (int64_t)s.S_pad;
  out[5] = out[6];
  if (!p->rep_on) return 0;
  out[0] = 1;
  out[1] = (int64_t)p->rep_nodes.size();
  out[2] = s.rep_rows;
  out[3] = p->views[1].I;
  out[4] = p->views[1].L;
  out[5] = (int64_t)(p->views[1].I - 1) * s.S_pad;
  for (size_t d = 0; d < p->rep_nodes.size(); d++)  // (a path of k nodes is walked once per 16 classes of its top node)
    out[5] += (int64_t)s.rep_tabs[d].rows * (int64_t)std::max<size_t>(1, p->rep_nodes[d].path.size());
  out[7] = p->rep_enabled ? 1 : 0;
  return 0;
}

}  // extern "C"

namespace hyhip {

// The persisted conditionals of class `cat` are stale (the last full pass ran with lazy persistence): re-run
// the pruning pass over the resident transition matrices with every node stored.
int ensure_resident(hyphy_hip_partition *p, int64_t cat) {
  if (p->resident[cat]) return 0;
  if (!p->initialized[cat] || p->cached_pi.size() != (size_t)p->D) return fail("conditionals not resident: evaluate first");
  std::vector<int64_t> all(p->B);
  for (int64_t k = 0; k < p->B; k++) all[k] = k;
  const std::vector<double> pi = p->cached_pi;
  const std::vector<char> lf = p->last_full;
  EvalRequest rq = request_of(cat, UpdateList{all.data(), p->B}, MatrixList{nullptr, 0}, pi.data());  // a persisting full pass over the resident matrices
  rq.reduce = true, rq.floor_log = false, rq.force_persist = true;
  if (eval_common(p, rq)) return -1;
  p->last_full = lf;  // (an internal pass: the caller's own sequence of evaluations is what the policy looks at)
  return collect_status(p);
}

// An uncollected hyphy_hip_evaluate_async owns the host-mapped result record: every entry point that is about to write it
// (or to wait on it) finishes the pending evaluation first (include/hyphy_hip.h: "any other evaluation entry point ...").
int finish_pending_async(hyphy_hip_partition *p) {
  if (!p->async_pending) return 0;
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    s.seq_wait = 0.;
  }
  p->async_pending = false;
  return 0;
}

// What class c's stored conditionals and per-pattern values hold of a pin after the evaluation just enqueued (partition.h: pin_left).
// A pin sits in the conditional of the pinned internal node, or of the pinned leaf's parent.  The evaluation recomputed that node — and
// with it everything above — when it was a full pass or listed anything below it as dirty (build_schedule recomputes every ancestor of a
// listed node); a node it recomputed without the pin is clean again, the pinned one is not.
static void note_pins(hyphy_hip_partition *p, int64_t c, const int64_t *update_nodes, int64_t n_update) {
  std::vector<int64_t> &left = p->pin_left[(size_t)c];
  if (left.empty() && p->pin_node < 0) return;
  const auto recomputed = [&](int64_t n) {
    if (p->sched_full) return true;
    const int64_t at = n < p->L ? p->parents[(size_t)n] : n - p->L;  // internal index of the node whose conditional holds the pin
    for (int64_t k = 0; k < n_update; k++) {
      const int64_t u = update_nodes[k];
      if (u < 0 || u >= p->B) continue;
      for (int64_t a = p->parents[(size_t)u]; a >= 0 && a <= at; a = p->parents[(size_t)(p->L + a)])
        if (a == at) return true;  // (children are numbered before parents: the walk stops once it is past the node)
    }
    return false;
  };
  left.erase(std::remove_if(left.begin(), left.end(), [&](int64_t n) { return n != p->pin_node && recomputed(n); }), left.end());
  if (p->pin_node >= 0 && std::find(left.begin(), left.end(), p->pin_node) == left.end()) left.push_back(p->pin_node);
}

int eval_common(hyphy_hip_partition *p, const EvalRequest &rq) {
  int64_t cat = rq.cat, n_update = rq.n_update;  // (rewritten below: class batching, new root frequencies)
  const int64_t *update_nodes = rq.update_nodes, *const q_nodes = rq.q_nodes;
  const int64_t n_q = rq.n_q;
  const double *const root_freqs = rq.root_freqs;
  const bool batch = rq.batch, force_persist = rq.force_persist;
  if (!p) return fail("partition == NULL");
  if (cat < 0) cat = 0;
  if (cat >= p->C) return fail("rate class out of range");
  if (finish_pending_async(p)) return -1;
  if (batch) {  // all classes in one launch: bookkeeping is shared, keyed on class 0
    if (p->nuc) return fail("internal: class batching is for the MFMA path");
    cat = 0;
    for (int64_t c = 1; c < p->C; c++)
      if (p->initialized[c] != p->initialized[0]) p->initialized[0] = 0;  // mixed state: force a full pass
  }
  // any ordinary evaluation invalidates the branch cache of its class (as the reference resets cachedBranches)
  if (batch) std::fill(p->bc_node.begin(), p->bc_node.end(), -1);
  else if (cat >= 0 && cat < (int64_t)p->bc_node.size()) p->bc_node[cat] = -1;
  if (!root_freqs) return fail("root_freqs == NULL");
  if ((n_update > 0 && !update_nodes) || (n_q > 0 && (!q_nodes || (rq.q_source != QSource::OwnStaged && !rq.q)))) return fail("null node / matrix list");
  if (n_q > p->B) return fail("more matrices than branches");
  if (!p->initialized[cat] && n_q < p->B)
    return fail("first evaluation of a rate class must supply all L+I-1 transition matrices");
  {  // validate the matrix list BEFORE any host cache is touched (a failed call must not leave a half-committed state)
    std::vector<char> seen(p->B, 0);
    for (int64_t k = 0; k < n_q; k++) {
      if (q_nodes[k] < 0 || q_nodes[k] >= p->B) return fail("q_nodes entry out of range");
      if (seen[q_nodes[k]]) return fail("q_nodes lists a branch twice");
      seen[q_nodes[k]] = 1;
    }
  }
  // the view this evaluation runs under: the class-compressed one wherever it exists, except with pinned states and for the
  // internal passes that restore the per-pattern copies of every node (branch cache, downloads)
  if (p->rep_on && p->rep_enabled && !p->rep_decided && !sw::given(sw::REPEATS) && !sw::tune()) {
    //  no measurement will ever settle on / off for this partition (the tuner is disabled): the static rule instead
    p->rep_decided = true;
    if (!rep_static_decision(p)) p->rep_enabled = false;
    p->rep_report = std::string("repeats: no measurement (HYPHY_HIP_TUNE=0), static rule -> ") + (p->rep_enabled ? "on" : "off");
    sw::note("%s\n", p->rep_report.c_str());
  }
  // New root frequencies and nothing to update: ComputeBlock applies theProbs at the root on every call, while the stored per-pattern
  // values hold the old ones — one child of the root is listed, so the root is combined again from all of its children.  (Per class:
  // the frequencies are shared, each class's stored values are its own.)
  if (p->cached_pi.size() != (size_t)p->D || memcmp(p->cached_pi.data(), root_freqs, p->D * sizeof(double))) p->pi_stale.assign(p->C, 1);
  const int64_t root_child = p->children[p->I - 1].front();
  if (n_update == 0 && p->initialized[cat] && !p->pi_stale.empty() &&
      (batch ? std::find(p->pi_stale.begin(), p->pi_stale.end(), 1) != p->pi_stale.end() : p->pi_stale[cat] != 0)) {
    update_nodes = &root_child;
    n_update = 1;
  }
  switch_mode(p, (p->rep_on && p->rep_enabled && p->pin_node < 0 && !force_persist) ? 1 : 0);
  bool changed = false;
  const int64_t bc = batch ? p->C : 1;
  if (bc != p->batch_classes) {
    p->batch_classes = bc;
    p->cached_valid = 0;  // fragment sizing depends on how many classes share the launch
  }
  if (prepare_schedule(p, (int)cat, update_nodes, n_update, &changed, force_persist, q_nodes, n_q, batch ? (int)p->C : 1)) return -1;
  {
    const bool tune_on = p->tuned_for != p->batch_classes && sw::tune() && !sw::schedule_forced();
    if (tune_on && !p->nuc && (p->variant >= 1 || (!p->kernel_forced && p->shards[0].ntiles >= 32)) && p->shards[0].T == 1 && p->sched_full && !p->sched_persist &&
        p->tuned_for != p->batch_classes && p->initialized[cat]) {
      if (tune_schedule(p, (int)cat, batch ? (int)p->C : 1)) return -1;
      // class-compressed or plain?  settled once per partition by timing both (repeats.hip), unless the caller or the environment chose
      if (p->mode == 1 && !p->rep_decided && !sw::given(sw::REPEATS) && rep_decide(p, (int)cat, batch ? (int)p->C : 1)) return -1;
      build_schedule(p, nullptr, 0, true);  // the chosen cut (a full pass: no update list)
      if (p->ops_host.size() > ops_capacity(p)) return fail("internal: schedule overflow");
      changed = true;
    }
  }
  bool pi_changed = p->cached_pi.size() != (size_t)p->D || memcmp(p->cached_pi.data(), root_freqs, p->D * sizeof(double));
  if (pi_changed) p->cached_pi.assign(root_freqs, root_freqs + p->D);
  if (p->cached_slots.size() != (size_t)p->C) p->cached_slots.assign(p->C, std::vector<int64_t>());
  // (a batched evaluation writes its C * n_q slot numbers from the start of the device table, across the regions the classes use one at
  //  a time: a switch between the two forms invalidates what is known about EVERY class's region, not only this call's — r06: the
  //  adapter's category hook alternates batched passes with one-class line searches, and class 1 found class 0's batch table in its
  //  region: exponentials written to slots beyond the last class)
  if (p->slots_batch_mode != (batch ? 1 : 0))
    for (auto &v : p->cached_slots) v.assign(1, -1);  // (no list of node codes equals this)
  std::vector<int64_t> &cs = p->cached_slots[cat];
  bool slots_changed = cs.size() != (size_t)n_q || (n_q > 0 && memcmp(cs.data(), q_nodes, n_q * sizeof(int64_t)));
  if (slots_changed) cs.assign(q_nodes, q_nodes + n_q);
  p->slots_batch_mode = batch ? 1 : 0;
  for (Shard &s : p->shards) {
    EvalCtx ctx{p, s, (int)cat, batch ? (int)p->C : 1, changed, pi_changed, slots_changed, rq};
    if (ctx.enqueue_eval()) {
      // some shard may hold a stale schedule / slot table / frequency vector now: rebuild everything next time
      p->cached_valid = 0;
      p->cached_pi.clear();
      for (auto &v : p->cached_slots) v.clear();
      p->slots_batch_mode = -1;
      p->initialized[cat] = 0;
      return -1;
    }
  }
  std::vector<char> &res_here = p->mode == 1 ? p->rep_resident : p->resident, &res_other = p->mode == 1 ? p->resident : p->rep_resident;
  if (batch)
    for (int64_t c = 0; c < p->C; c++) {
      p->initialized[c] = 1;
      if (p->sched_full) res_here[c] = p->sched_persist ? 1 : 0;
      if (!res_other.empty()) res_other[c] = 0;  // (the other view's copies are stale now)
      p->last_full[c] = p->last_full[0];
    }
  p->initialized[cat] = 1;
  if (p->sched_full) res_here[cat] = p->sched_persist ? 1 : 0;
  if (!res_other.empty()) res_other[cat] = 0;
  if (batch) std::fill(p->pi_stale.begin(), p->pi_stale.end(), 0);  // (every pass reaches the root)
  else p->pi_stale[cat] = 0;
  for (int64_t c = batch ? 0 : cat; c < (batch ? p->C : cat + 1); c++) note_pins(p, c, update_nodes, n_update);
  return 0;  // (coefficients staged by hyphy_hip_build_q stay valid — and pending — until the next hyphy_hip_build_q)
}

// value of a device scalar behind everything queued on the (single) shard's stream -> host, through the host-mapped record
__global__ void publish_scalar_kernel(const double *__restrict__ value, double *__restrict__ rec, const int *__restrict__ status,
                                      double seq) {
  rec[0] = value[0];
  rec[1] = 0.;
  rec[2] = status ? (double)*status : 0.;
  if (seq != 0.) {
    __threadfence_system();
    reinterpret_cast<volatile double *>(rec)[3] = seq;
  }
}
int publish_and_collect(hyphy_hip_partition *p, const double *d_value, double *value_out) {
  if (finish_pending_async(p)) return -1;
  Shard &s = p->shards[0];
  HIPCHK(hipSetDevice(s.device));
  double *rec = s.d_hout ? s.d_hout : s.out;
  hipLaunchKernelGGL(publish_scalar_kernel, dim3(1), dim3(1), 0, s.stream, d_value, rec, (const int *)s.status,
                     next_seq(s, rec == s.d_hout));
  HIPCHK(hipGetLastError());
  if (collect_status(p)) return -1;
  *value_out = s.h_out[0];
  return 0;
}

// A shard that takes no part in the last kernel of a synchronous call (hmm.hip: shard 0 finishes alone) still posts its record, for
// the expm status collect_status reads.
int post_status_record(Shard &s) {
  HIPCHK(hipSetDevice(s.device));
  double *rec = s.d_hout ? s.d_hout : s.out;
  hipLaunchKernelGGL(publish_scalar_kernel, dim3(1), dim3(1), 0, s.stream, (const double *)s.out, rec, (const int *)s.status,
                     next_seq(s, rec == s.d_hout));
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace hyhip

extern "C" {

int hyphy_hip_evaluate(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                       const int64_t *q_nodes, int64_t n_q, const double *q_dense, int q_is_probability,
                       const double *root_freqs, double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  if (p && begin_site_export(p, site_lik_out != nullptr, site_scaler_out != nullptr)) return -1;
  EvalRequest rq = request_of(cat, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::HostDense, rq.q = q_dense, rq.q_is_probability = q_is_probability;
  rq.reduce = true, rq.floor_log = false;
  if (eval_common(p, rq)) {
    if (p) p->export_sites = 0;
    return -1;
  }
  p->export_sites = 0;
  return result_tail(p, cat < 0 ? 0 : (int)cat, kCombineShards, kRecordTimings, kSitesExported, logl_out, site_lik_out, site_scaler_out);
}

}  // extern "C"

// the two mixture entry points from the component counts onwards (`rq`: the lists and the matrix source)
static int evaluate_mixture_common(hyphy_hip_partition *p, EvalRequest rq, const int64_t *n_components, const double *weights,
                                   double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  MixSpec mix{n_components, weights, 0};
  for (int64_t k = 0; k < rq.n_q; k++) {
    if (n_components[k] < 1 || n_components[k] > kMixRows) return fail("mixture evaluation: 1..16 components per branch");
    mix.n_tot += n_components[k];
  }
  rq.reduce = true, rq.floor_log = false;
  rq.mix = rq.n_q > 0 ? &mix : nullptr;
  if (eval_common(p, rq)) return -1;
  // (unlike hyphy_hip_evaluate: the host's sum whatever HYPHY_HIP_COMBINE says, and copies instead of the export)
  return result_tail(p, rq.cat < 0 ? 0 : (int)rq.cat, kCombineHost, kRecordTimings, kSitesGathered, logl_out, site_lik_out, site_scaler_out);
}

extern "C" {

/* Branch-site mixtures on every branch (the reference's "explicit form" models: BUSTED / BS-REL whole-alignment
 * evaluation): P_b = sum_m weights exp(Q_bm), formed on the device; 1..16 components per branch, a count of its own on each.
 * A component that cannot be exponentiated fails the call whatever its weight, 0 included (include/hyphy_hip.h). */
int hyphy_hip_evaluate_mixture(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                               const int64_t *q_nodes, int64_t n_q, const int64_t *n_components, const double *q_dense,
                               const double *weights, const double *root_freqs, double *logl_out, double *site_lik_out,
                               int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (n_q > 0 && (!n_components || !weights || !q_dense)) return fail("mixture evaluation: null argument");
  EvalRequest rq = request_of(cat, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::HostDense, rq.q = q_dense;
  return evaluate_mixture_common(p, rq, n_components, weights, logl_out, site_lik_out, site_scaler_out);
}

/* The same with the component rate matrices formed ON THE DEVICE (r04): Q_(b,m) = sum_k x_(b,m),k T_k over the templates of
 * hyphy_hip_set_q_templates / hyphy_hip_update_q_templates, one coefficient row per (branch of q_nodes, component) staged by
 * hyphy_hip_build_q (n = sum of n_components rows, branch-major) — no dense matrix crosses PCIe.  BS-REL / BUSTED components
 * differ in a global only (omega_m): component m of a branch with locals x_b is x_b at the columns of component m's templates. */
int hyphy_hip_evaluate_mixture_built(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                     const int64_t *q_nodes, int64_t n_q, const int64_t *n_components, const double *weights,
                                     const double *root_freqs, double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (!p->K) return fail("evaluate_mixture_built: templates not set");
  if (n_q > 0 && (!n_components || !weights)) return fail("mixture evaluation: null argument");
  if (n_q <= 0) return fail("evaluate_mixture_built: no matrices (use hyphy_hip_evaluate_built for a pure re-evaluation)");
  EvalRequest rq = request_of(cat, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::OwnStaged;
  return evaluate_mixture_common(p, rq, n_components, weights, logl_out, site_lik_out, site_scaler_out);
}

/* Asynchronous pair (partitions of one likelihood function on different devices / streams overlap: the host enqueues
 * every partition's evaluation before it waits for the first — the reference's partition loop, likefunc.cpp:2524-2589,
 * is serial).  The matrices are copied to a pinned staging buffer, so the caller's array is free on return. */
int hyphy_hip_evaluate_async(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                             const int64_t *q_nodes, int64_t n_q, const double *q_dense, int q_is_probability,
                             const double *root_freqs) {
  if (!p) return fail("partition == NULL");
  if (p->async_pending && hyphy_hip_synchronize(p)) return -1;
  p->async_pending = false;
  const size_t n = (size_t)std::max<int64_t>(0, n_q) * p->D * p->D;
  if (n > 0) {
    if (!q_dense) return fail("null matrix list");
    if (p->h_qstage_cap < n) {
      if (hyphy_hip_synchronize(p)) return -1;
      const size_t cap = std::max(n, (size_t)p->B * p->D * p->D);
      HIPCHK(p->own.regrow({pinned_block(p->h_qstage, cap * sizeof(double))}, p->h_qstage_cap, n, cap, FreeMode::Sync));
    }
    // (the previous asynchronous evaluation was collected or synchronised above: the staging buffer is free)
    memcpy(p->h_qstage, q_dense, n * sizeof(double));
  }
  EvalRequest rq = request_of(cat, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::HostDense, rq.q = n > 0 ? p->h_qstage : nullptr, rq.q_is_probability = q_is_probability;
  rq.reduce = true, rq.floor_log = false;
  if (eval_common(p, rq)) return -1;
  p->async_pending = true;
  p->async_cat = cat < 0 ? 0 : cat;
  return 0;
}

int hyphy_hip_collect(hyphy_hip_partition *p, double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (!p->async_pending) return fail("collect: no asynchronous evaluation pending");
  p->async_pending = false;
  return result_tail(p, (int)p->async_cat, kCombineHost, kRecordTimings, kSitesGathered, logl_out, site_lik_out, site_scaler_out);
}

int hyphy_hip_evaluate_built_sites(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                   const int64_t *q_nodes, int64_t n_q, const double *root_freqs, double *logl_out,
                                   double *site_lik_out, int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (begin_site_export(p, site_lik_out != nullptr, site_scaler_out != nullptr)) return -1;
  const int rc = hyphy_hip_evaluate_built(p, cat, update_nodes, n_update, q_nodes, n_q, root_freqs, logl_out);
  p->export_sites = 0;
  if (rc) return -1;
  return finish_sites(p, cat < 0 ? 0 : (int)cat, site_lik_out, site_scaler_out);
}

int hyphy_hip_evaluate_built(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                             const int64_t *q_nodes, int64_t n_q, const double *root_freqs, double *logl_out) {
  if (!p) return fail("partition == NULL");
  if (!p->K) return fail("evaluate_built: templates not set");
  EvalRequest rq = request_of(cat, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::OwnStaged;  // (filled / staged by build_q on every shard)
  rq.reduce = true, rq.floor_log = false;
  if (eval_common(p, rq)) return -1;
  Trace tr("evaluate_built");
  if (collect_status(p)) return -1;
  tr.lap("wait");
  return combine_shards(p, logl_out);
}

int hyphy_hip_evaluate_device(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                              const int64_t *q_nodes, int64_t n_q, const double *d_q, int q_is_probability,
                              const double *root_freqs, double *d_logl_out) {
  if (!p) return fail("partition == NULL");
  if (p->shards.size() != 1) return fail("evaluate_device needs a single-device partition");
  Trace tr("evaluate_device");
  struct Fin { Trace &t; ~Fin() { t.lap("total"); } } fin{tr};
  EvalRequest rq = request_of(cat, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::DeviceDense, rq.q = d_q, rq.q_is_probability = q_is_probability;
  rq.d_logl_out = d_logl_out;
  rq.reduce = true, rq.floor_log = false;
  return eval_common(p, rq);
}

/* A device scalar (the all-reduced log-likelihood of a multi-rank evaluation: hyphy_hip_evaluate_device + the caller's
 * collective on the same stream) back on the host the way the synchronous entry points do it: a one-thread kernel behind
 * everything queued on the partition's stream posts [value, 0, expm status, sequence word] into the host-mapped result
 * record and the host spins on the sequence word — no device-to-host copy command, no stream synchronisation. */

int hyphy_hip_fetch_device_scalar(hyphy_hip_partition *p, const double *d_value, double *value_out) {
  if (!p || !d_value || !value_out) return fail("fetch_device_scalar: null argument");
  if (p->shards.size() != 1) return fail("fetch_device_scalar needs a single-device partition");
  return publish_and_collect(p, d_value, value_out);
}

int hyphy_hip_evaluate_categories(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                  const int64_t *q_nodes, int64_t n_q, const double *q_dense, int q_is_probability,
                                  const double *weights, const double *root_freqs, double *logl_out,
                                  double *site_lik_out, int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (!weights) return fail("weights == NULL");
  const int64_t D = p->D;
  EvalRequest rq = request_of(0, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::HostDense, rq.q = q_dense, rq.q_is_probability = q_is_probability;
  rq.reduce = false, rq.floor_log = true;  // (the per-pattern values of every class, floored: mixed and reduced below)
  if (!p->nuc) {
    // rate-class batching: ONE expm launch over C*n_q matrices and ONE pruning launch with a grid row
    // per class (3x the workgroups of a single pass: the matrix pipe finally has enough waves)
    rq.batch = true;
    if (eval_common(p, rq)) return -1;
  } else {
    for (int64_t c = 0; c < p->C; c++) {
      if (!p->initialized[c]) p->cached_valid = 0;
      rq.cat = c;
      rq.q = q_dense ? q_dense + (size_t)c * n_q * D * D : nullptr;
      if (eval_common(p, rq)) return -1;
    }
  }
  // (this entry point uploads the weights at every call — a wait for the stream —, its built twin only when they change)
  if (mix_and_reduce_categories(p, weights, /* always = */ true)) return -1;
  return result_tail(p, 0, kCombineHost, kNoTimings, kSitesGatheredMixed, logl_out, site_lik_out, site_scaler_out);
}

int hyphy_hip_evaluate_categories_built_sites(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                              const int64_t *q_nodes, int64_t n_q, const double *weights,
                                              const double *root_freqs, double *logl_out, double *site_lik_out,
                                              int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (!p->K) return fail("evaluate_categories_built: templates not set");
  if (p->nuc) return fail("evaluate_categories_built: MFMA partitions only (4-state: hyphy_hip_evaluate_categories)");
  if (!weights) return fail("weights == NULL");
  EvalRequest rq = request_of(0, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::OwnStaged;
  rq.reduce = false, rq.floor_log = true, rq.batch = true;
  if (eval_common(p, rq)) return -1;
  if (mix_and_reduce_categories(p, weights, /* always = */ false)) return -1;
  return result_tail(p, 0, kCombineHost, kNoTimings, kSitesGatheredMixed, logl_out, site_lik_out, site_scaler_out);
}

int hyphy_hip_evaluate_categories_built(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                        const int64_t *q_nodes, int64_t n_q, const double *weights,
                                        const double *root_freqs, double *logl_out) {
  return hyphy_hip_evaluate_categories_built_sites(p, update_nodes, n_update, q_nodes, n_q, weights, root_freqs, logl_out, nullptr, nullptr);
}

}  // extern "C"

// the two class-batched mixture entry points from the component counts onwards (`rq`: the lists and the matrix source)
static int evaluate_categories_mixture_common(hyphy_hip_partition *p, EvalRequest rq, const int64_t *n_components, const double *mix_weights,
                                              const double *class_weights, double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  MixSpec mix{n_components, mix_weights, 0};
  for (int64_t k = 0; k < rq.n_q; k++) {
    if (n_components[k] < 1 || n_components[k] > kMixRows) return fail("mixture evaluation: 1..16 components per branch");
    mix.n_tot += n_components[k];
  }
  rq.reduce = false, rq.floor_log = true;  // (the per-pattern values of every class, floored: mixed and reduced below)
  if (p->nuc) {  // 4 states: the classes one after another through the one-class staging, as hyphy_hip_evaluate_categories does
    const double *q = rq.q;
    for (int64_t c = 0; c < p->C; c++) {
      if (!p->initialized[c]) p->cached_valid = 0;
      MixSpec one{n_components, mix_weights ? mix_weights + (size_t)c * mix.n_tot : nullptr, mix.n_tot};
      rq.cat = c;
      rq.q = q ? q + (size_t)c * mix.n_tot * p->D * p->D : nullptr;
      rq.mix = rq.n_q > 0 ? &one : nullptr;
      if (eval_common(p, rq)) return -1;
    }
    if (mix_and_reduce_categories(p, class_weights, /* always = */ true)) return -1;
    return result_tail(p, 0, kCombineHost, kNoTimings, kSitesGatheredMixed, logl_out, site_lik_out, site_scaler_out);
  }
  rq.batch = true;
  rq.mix = rq.n_q > 0 ? &mix : nullptr;
  if (prepare_class_mixture_staging(p, (size_t)p->C * mix.n_tot, class_weights)) return -1;
  if (eval_common(p, rq)) return -1;
  if (mix_and_reduce_categories(p, class_weights, /* always = */ false, /* staged = */ true)) return -1;
  if (result_tail(p, 0, kCombineHost, kNoTimings, kSitesGatheredMixed, logl_out, site_lik_out, site_scaler_out)) return -1;
  class_mixture_staging_done(p);
  return 0;
}

extern "C" {

/* Rate classes over branch-site mixtures in one batched evaluation (include/hyphy_hip.h): class c evolves on branch q_nodes[k] under
 * P = sum_m mix_weights[c][.] exp(Q[c][.]); ONE exponential launch over the C * n_tot components, mix_class_images_kernel with a grid
 * row per class, one pruning launch with a grid row per class, and the class mix of hyphy_hip_evaluate_categories. */
int hyphy_hip_evaluate_categories_mixture(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update, const int64_t *q_nodes,
                                          int64_t n_q, const int64_t *n_components, const double *q_dense, const double *mix_weights,
                                          const double *class_weights, const double *root_freqs, double *logl_out,
                                          double *site_lik_out, int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (!class_weights) return fail("class_weights == NULL");
  if (n_q > 0 && (!n_components || !mix_weights || !q_dense)) return fail("mixture evaluation: null argument");
  EvalRequest rq = request_of(0, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::HostDense, rq.q = n_q > 0 ? q_dense : nullptr;
  return evaluate_categories_mixture_common(p, rq, n_components, mix_weights, class_weights, logl_out, site_lik_out, site_scaler_out);
}

/* The same from rows staged by hyphy_hip_build_q: C * n_tot rows, one per (class, branch, component) in that order.  In steady
 * state the host waits once, for the result record. */
int hyphy_hip_evaluate_categories_mixture_built(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                                const int64_t *q_nodes, int64_t n_q, const int64_t *n_components,
                                                const double *mix_weights, const double *class_weights, const double *root_freqs,
                                                double *logl_out, double *site_lik_out, int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (!p->K) return fail("evaluate_categories_mixture_built: templates not set");
  if (p->nuc) return fail("evaluate_categories_mixture_built: MFMA partitions only (4-state: hyphy_hip_evaluate_categories_mixture)");
  if (!class_weights) return fail("class_weights == NULL");
  if (n_q > 0 && (!n_components || !mix_weights)) return fail("mixture evaluation: null argument");
  EvalRequest rq = request_of(0, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::OwnStaged;
  return evaluate_categories_mixture_common(p, rq, n_components, mix_weights, class_weights, logl_out, site_lik_out, site_scaler_out);
}

// The two category entry points above with the hidden-Markov combine (hmm.hip) in place of the weighted mix: the class passes are
// queued as there, mix_and_reduce_categories is skipped altogether, and hmm_combine's last kernel posts the result record: one wait.
int hyphy_hip_evaluate_categories_hmm(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update, const int64_t *q_nodes,
                                      int64_t n_q, const double *q_dense, int q_is_probability, const double *transition,
                                      const double *initial, const double *root_freqs, double *logl_out) {
  if (p && !logl_out) return fail("evaluate_categories_hmm: logl_out == NULL");
  if (const int rc = hmm_check(p, transition, initial, "evaluate_categories_hmm", false)) return rc;
  EvalRequest rq = request_of(0, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::HostDense, rq.q = q_dense, rq.q_is_probability = q_is_probability;
  rq.reduce = false, rq.floor_log = true;
  if (!p->nuc) {
    rq.batch = true;
    if (eval_common(p, rq)) return -1;
  } else {
    for (int64_t c = 0; c < p->C; c++) {
      if (!p->initialized[c]) p->cached_valid = 0;
      rq.cat = c;
      rq.q = q_dense ? q_dense + (size_t)c * n_q * p->D * p->D : nullptr;
      if (eval_common(p, rq)) return -1;
    }
  }
  return hmm_combine(p, transition, initial, logl_out, nullptr);
}

int hyphy_hip_evaluate_categories_built_hmm(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update, const int64_t *q_nodes,
                                            int64_t n_q, const double *transition, const double *initial, const double *root_freqs,
                                            double *logl_out) {
  if (p && !logl_out) return fail("evaluate_categories_built_hmm: logl_out == NULL");
  if (const int rc = hmm_check(p, transition, initial, "evaluate_categories_built_hmm", false)) return rc;
  if (!p->K) return fail("evaluate_categories_built_hmm: templates not set");
  if (p->nuc) return fail("evaluate_categories_built_hmm: MFMA partitions only (4-state: hyphy_hip_evaluate_categories_hmm)");
  EvalRequest rq = request_of(0, UpdateList{update_nodes, n_update}, MatrixList{q_nodes, n_q}, root_freqs);
  rq.q_source = QSource::OwnStaged;
  rq.reduce = false, rq.floor_log = true, rq.batch = true;
  if (eval_common(p, rq)) return -1;
  return hmm_combine(p, transition, initial, logl_out, nullptr);
}

int hyphy_hip_download_partials(hyphy_hip_partition *p, int64_t cat, double *inode_cache, int64_t *scaler_counts) {
  if (!p) return fail("partition == NULL");
  if (cat < 0) cat = 0;
  if (cat >= p->C) return fail("rate class out of range");
  if (ensure_resident(p, cat)) return -1;
  const int64_t D = p->D, I = p->I, S = p->S;
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (inode_cache) {
      if (p->nuc) {
        std::vector<double> tmp((size_t)I * 4 * s.S_pad);
        HIPCHK(hipMemcpy(tmp.data(), s.partials + (size_t)cat * s.partial_stride, tmp.size() * sizeof(double),
                         hipMemcpyDeviceToHost));
        for (int64_t n = 0; n < I; n++)
          for (int64_t k = 0; k < s.S; k++)
            for (int j = 0; j < 4; j++)
              inode_cache[(n * S + caller_pattern(p, s.s0 + k)) * 4 + j] = tmp[((size_t)n * 4 + j) * s.S_pad + k];
      } else {
        Blocks blk;
        double *dtmp = nullptr;
        HIPCHK(blk.get(&dtmp, (size_t)I * s.S * D));
        launch_unpack_partials_mfma(s.partials + (size_t)cat * s.partial_stride, (int)I, s.ntiles, p->NW, (int)D,
                                    (int)s.S, dtmp, s.stream);
        hipError_t e;
        if (p->perm.empty()) {
          e = hipMemcpy2DAsync(inode_cache + s.s0 * D, (size_t)S * D * sizeof(double), dtmp,
                               (size_t)s.S * D * sizeof(double), (size_t)s.S * D * sizeof(double), (size_t)I,
                               hipMemcpyDeviceToHost, s.stream);
          hipStreamSynchronize(s.stream);
        } else {  // sorted patterns: through a host copy, one node at a time, back into the caller's pattern order
          std::vector<double> tmp((size_t)s.S * D);
          e = hipStreamSynchronize(s.stream);  // (the unpack kernel runs on the shard's stream)
          for (int64_t n = 0; n < I && e == hipSuccess; n++) {
            e = hipMemcpy(tmp.data(), dtmp + (size_t)n * s.S * D, tmp.size() * sizeof(double), hipMemcpyDeviceToHost);
            for (int64_t k = 0; k < s.S; k++)
              memcpy(inode_cache + ((size_t)n * S + p->perm[s.s0 + k]) * D, tmp.data() + (size_t)k * D, (size_t)D * sizeof(double));
          }
        }
        if (e != hipSuccess) return fail(std::string("download_partials: ") + hipGetErrorString(e));
      }
    }
    if (scaler_counts) {
      std::vector<int32_t> tmp((size_t)I * s.S_pad);
      HIPCHK(hipMemcpy(tmp.data(), s.counts + (size_t)cat * I * s.S_pad, tmp.size() * sizeof(int32_t),
                       hipMemcpyDeviceToHost));
      for (int64_t n = 0; n < I; n++)
        for (int64_t k = 0; k < s.S; k++) {
          scaler_counts[n * S + caller_pattern(p, s.s0 + k)] = tmp[(size_t)n * s.S_pad + k];
        }
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Pinned node states: ComputeBlock's branchIndex / branchValues ("setBranch", likefunc.cpp:10950-10957;
// tree_evaluator.cpp:163-181 for a leaf, :583-594 + :3624 for an internal node) — the evaluations that follow
// see node `node` fixed to states[pattern].  Used by marginal ancestral reconstruction
// (RecoverAncestralSequencesMarginal, likefunc2.cpp:932-1040: one pinned evaluation per node and state).
// ---------------------------------------------------------------------------------------------------
int hyphy_hip_set_pinned_states(hyphy_hip_partition *p, int64_t node, const int64_t *states) {
  if (!p) return fail("partition == NULL");
  if (node < 0 || !states) {
    // (back to the re-rooted form of the steady-state passes, the tuner's or HYPHY_HIP_REROOT=1's: the pinned passes' schedule is
    //  not one, and an unchanged update list would keep it)
    if (p->pin_node >= 0 && (p->rr_use || sw::reroot() == 1)) p->cached_valid = 0;
    p->pin_node = -1;
    return 0;
  }
  if (node >= p->L + p->I) return fail("set_pinned_states: node out of range");
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    std::vector<int16_t> h(s.S_pad, 0);
    for (int64_t k = 0; k < s.S; k++) {
      const int64_t st = states[caller_pattern(p, s.s0 + k)];
      if (st < 0 || st >= p->D) return fail("set_pinned_states: state out of range");
      h[k] = (int16_t)st;
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipMemcpy(s.pin, h.data(), h.size() * sizeof(int16_t), hipMemcpyHostToDevice));
  }
  p->pin_node = node;
  if (p->rr_active) p->cached_valid = 0;  // (re-rooted schedules are built for evaluations without pinned states)
  std::fill(p->bc_node.begin(), p->bc_node.end(), -1);
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// Branch cache: _TheTree::ComputeBranchCache (tree_evaluator.cpp:4286-4845) builds, for one
// branch, everything the likelihood needs except that branch's transition matrix; ComputeLLWithBranchCache
// (tree.cpp:3383-3936) then evaluates L(t) with one [D x D] x [D x S] contraction per call while the
// optimiser's line search varies the branch length (policy code likefunc.cpp:10886-10948, 11125-11258).
// ---------------------------------------------------------------------------------------------------
int hyphy_hip_branch_cache_build(hyphy_hip_partition *p, int64_t cat, int64_t node) {
  if (!p) return fail("partition == NULL");
  if (p->nuc) {
    g_last_error = "branch cache: not available for the 4-state path";
    return 1;
  }
  if (cat < 0) cat = 0;
  if (cat >= p->C) return fail("rate class out of range");
  if (node < 0 || node >= p->B) return fail("branch cache: node out of range (the root has no branch)");
  if (!p->initialized[cat]) return fail("branch cache: evaluate the partition first (conditionals must be resident)");
  if (ensure_resident(p, cat)) return -1;
  switch_mode(p, 0);  // (the outside vector is built over the partition's own tree)
  const int L = (int)p->L, I = (int)p->I, C = (int)p->C;
  const int64_t B = p->B;
  const int DP = p->DP;
  // ancestors of the branch's parent up to the root; a[0] = root ... a[m] = parent of `node`
  std::vector<int> a;
  for (int64_t x = p->parents[node]; x >= 0; x = p->parents[L + x]) a.push_back((int)x);
  std::reverse(a.begin(), a.end());
  const int m = (int)a.size() - 1;
  if (m < 0) return fail("branch cache: node has no parent");
  const int vbase = (C - (int)cat) * I + 2 * (int)cat;        // node slots behind the last class, relative to this class
  const int tbase = (int)((C - cat) * B + cat * (I + 2));     // matrix slots behind the last class, relative to this class
  std::vector<int4> ops;
  for (int k = 0; k <= m; k++) {
    const int vid = k == m ? vbase : vbase + 1;
    const int exclude = k < m ? L + a[k + 1] : (int)node;
    std::vector<int4> entries;
    if (k >= 1) {  // the rest of the tree above: previous chain node through the transposed matrix of a[k]'s branch
      int4 op;
      op.x = OPK_INTERNAL | (((k - 1) & 1) << 24);
      op.y = vid;
      op.z = tbase + k;
      op.w = 0;
      entries.push_back(op);
    }
    const std::vector<int> &ch = p->children[a[k]];
    const int G = p->shards[0].T <= 2 ? 2 : 1;
    std::vector<int> leaves;
    for (int c : ch)
      if (c < L && c != exclude) leaves.push_back(c);
    for (size_t i = 0; i < leaves.size();) {
      int nl = 1;
      const bool amb0 = p->leaf_has_ambig[leaves[i]];
      if (!amb0 && G > 1 && i + 1 < leaves.size() && !p->leaf_has_ambig[leaves[i + 1]]) nl = 2;
      const unsigned l0 = (unsigned)leaves[i], l1 = nl > 1 ? (unsigned)leaves[i + 1] : l0;
      int4 op;
      op.x = OPK_LEAF | (amb0 ? OPF_AMBIG : 0) | (nl << 8) | (0xff << 24);
      op.y = vid;
      op.z = (int)(l0 | (l1 << 16));
      op.w = 0;
      entries.push_back(op);
      i += nl;
    }
    for (int c : ch)
      if (c >= L && c != exclude) {
        int4 op;
        op.x = OPK_INTERNAL_GLOBAL | (0xff << 24);
        op.y = vid;
        op.z = c;
        op.w = c - L;
        entries.push_back(op);
      }
    if (entries.empty()) {  // (a root whose only other child is the excluded one: the outside vector is all ones)
      int4 op;
      op.x = OPK_LEAF | (0xff << 24);
      op.y = vid;
      op.z = 0;
      op.w = 0;
      entries.push_back(op);
    }
    entries.back().x |= OPF_LAST | ((k & 1) ? OPF_PARITY : 0) | ((k & 1) << 16);
    for (const int4 &e : entries) ops.push_back(e);
  }
  int4 nop;
  nop.x = OPK_LEAF | (0xff << 24);
  nop.y = vbase + 1;
  nop.z = 0;
  nop.w = 0;
  if (ops.size() & 1) ops.push_back(nop);
  const int n = (int)ops.size();
  ops.push_back(nop);
  ops.push_back(nop);
  if (ops.size() > ops_capacity(p)) return fail("internal: branch-cache schedule overflow");
  const int4 prog = make_int4(0, n, -1, 0);
  const int32_t slot = (int32_t)node;
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipMemcpyAsync(s.bc_ops, ops.data(), ops.size() * sizeof(int4), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(s.bc_prog, &prog, sizeof(int4), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(s.bc_slot + cat, &slot, sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));  // (the host vectors go out of scope)
    double *Pf = s.Pfrag + (size_t)cat * B * DP * DP;
    for (int k = 1; k <= m; k++)  // M_k[j][i] = P_{a[k]}[i][j], times pi_i on the edge that leaves the old root
      launch_transpose_frag(Pf + (size_t)(L + a[k]) * DP * DP, Pf + (size_t)(tbase + k) * DP * DP, k == 1 ? s.pi : nullptr,
                            p->NW, s.stream);
    PruneArgs pa = base_prune_args(p, s, (int)cat, 1);
    pa.ops = s.bc_ops;
    pa.prog = s.bc_prog;
    pa.n_ops = n;
    pa.n_prog = 1;
    pa.do_root = 0;
    pa.n_prog_total = 1;
    if (launch_prune_mfma(pa, s.stream)) return fail("internal: branch cache: no pruning kernel for this launch form");
    HIPCHK(hipGetLastError());
  }
  p->bc_node[cat] = node;
  p->bc_use_pi[cat] = m == 0 ? 1 : 0;
  return 0;
}

int hyphy_hip_branch_cache_evaluate(hyphy_hip_partition *p, int64_t cat, int64_t node, const double *q_dense,
                                    int q_is_probability, double *logl_out, double *site_lik_out,
                                    int64_t *site_scaler_out) {
  if (!p) return fail("partition == NULL");
  if (cat < 0) cat = 0;
  if (cat >= p->C) return fail("rate class out of range");
  if (p->bc_node[cat] < 0 || p->bc_node[cat] != node)
    return fail("branch cache: no cache resident for this branch (call hyphy_hip_branch_cache_build after an evaluation)");
  if (!q_dense) return fail("null matrix pointer");
  if (finish_pending_async(p)) return -1;
  p->rep_stale_branch = node;  // (this branch's matrix image is rewritten below: its class table is stale)
  std::fill(p->rep_resident.begin(), p->rep_resident.end(), 0);
  const int L = (int)p->L, I = (int)p->I, C = (int)p->C;
  const int64_t B = p->B, D = p->D;
  const int DP = p->DP;
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipMemcpyAsync(s.bc_q, q_dense, (size_t)D * D * sizeof(double), hipMemcpyHostToDevice, s.stream));
    ExpmArgs ea;
    ea.Q = s.bc_q, ea.slots = s.bc_slot + cat, ea.n = 1, ea.D = (int)D, ea.is_prob = q_is_probability;
    ea.status = s.status;
    ea.Pfrag = s.Pfrag + (size_t)cat * B * DP * DP;
    ea.PTg = s.PTg + (size_t)cat * B * DP * DP;
    launch_expm(ea, s.stream);
    s.twins_dirty = true;  // (this branch's image was rewritten without its twin, if it has one)
    BcArgs ba;
    ba.NW = p->NW;
    ba.S_pad = s.S_pad;
    ba.ntiles = s.ntiles;
    ba.L = L;
    ba.node_A = (C - (int)cat) * I + 2 * (int)cat;
    ba.child_internal = node >= L ? (int)(node - L) : -1;
    ba.child_leaf = node < L ? (int)node : 0;
    ba.use_pi = p->bc_use_pi[cat];
    ba.Pfrag = ea.Pfrag + (size_t)node * DP * DP;
    ba.PTg = ea.PTg + (size_t)node * DP * DP;
    ba.codes_tile = s.codes_tile;
    ba.ambig = s.ambig;
    ba.partials = s.partials + (size_t)cat * s.partial_stride;
    ba.counts = s.counts + (size_t)cat * I * s.S_pad;
    ba.pi = s.pi;
    ba.freq = s.freq;
    ba.site_lik = s.site_lik + (size_t)cat * s.S_pad;
    ba.site_cnt = s.site_cnt + (size_t)cat * s.S_pad;
    ba.wg_sum = s.wg_sum;
    ba.wg_cnt = s.wg_cnt;
    ba.wg_flag = s.wg_flag;
    launch_bc_eval(ba, s.stream);
    double *rec = s.d_hout ? s.d_hout : s.out;
    const char *form = launch_wg_reduce(s.wg_sum, s.wg_cnt, s.wg_flag, s.ntiles, rec, rec + 1, s.status, s.stream, next_seq(s, rec == s.d_hout));
    if (&s == &p->shards[0]) p->last_reduce = {form, s.ntiles, false};
    HIPCHK(hipGetLastError());
  }
  return result_tail(p, (int)cat, kCombineHost, kNoTimings, kSitesGathered, logl_out, site_lik_out, site_scaler_out);
}

int hyphy_hip_expm_batch(int64_t D, int64_t n, const double *q_dense, double *p_out) {
  if (D < 2 || D > 64) {
    g_last_error = "unsupported state count (this version: 2 <= D <= 64)";
    return 1;
  }
  if (n <= 0) return 0;
  if (!q_dense || !p_out) return fail("null matrix pointer");
  if (hyphy_hip_device_count() <= 0) return fail("no HIP device available (this library has no CPU fallback)");
  double *dq = nullptr, *dp = nullptr;
  int32_t *st = nullptr;
  const size_t bytes = (size_t)n * D * D * sizeof(double);
  Blocks blk;
  HIPCHK(blk.get(&dq, (size_t)n * D * D));
  HIPCHK(blk.get(&dp, (size_t)n * D * D));
  HIPCHK(blk.get(&st, 1));
  HIPCHK(hipMemset(st, 0, sizeof(int32_t)));
  HIPCHK(hipMemcpy(dq, q_dense, bytes, hipMemcpyHostToDevice));
  ExpmArgs ea;
  ea.Q = dq; ea.n = (int)n; ea.D = (int)D;
  ea.Prow = dp; ea.status = st;
  launch_expm(ea, nullptr);
  int32_t hst = 0;
  hipError_t e1 = hipMemcpy(p_out, dp, bytes, hipMemcpyDeviceToHost);
  hipError_t e2 = hipMemcpy(&hst, st, sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e1 != hipSuccess || e2 != hipSuccess) return fail("expm_batch: device copy failed");
  if (hst) return fail("Failed to compute a valid transition matrix; this is usually caused by ill-conditioned rate "
                       "matrices (e.g. very large rate values)");
  return 0;
}

// [K][64*64] copies of the templates for expm64_kernel: zero padding, zero diagonals (the kernel derives Q_ii itself)
static std::vector<double> padded_templates(const double *templates, int64_t K, int64_t D) {
  std::vector<double> pad((size_t)K * 64 * 64, 0.0);
  for (int64_t k = 0; k < K; k++)
    for (int64_t r = 0; r < D; r++)
      for (int64_t c = 0; c < D; c++)
        if (r != c) pad[((size_t)k * 64 + r) * 64 + c] = templates[((size_t)k * D + r) * D + c];
  return pad;
}

int hyphy_hip_set_q_templates(hyphy_hip_partition *p, int64_t K, const double *templates) {
  if (!p || K < 1 || !templates) return fail("invalid templates");
  const int64_t D = p->D;
  p->K = 0;  // (until every shard holds the new set)
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    // rows: one per (class, branch), or — mixtures built on the device — one per (branch, component), up to kMixRows components
    const size_t coeff_rows_cap = (size_t)std::max<int64_t>(p->C, kMixRows) * p->B;
    // pinned rings: four slots of coefficients (hyphy_hip_build_q), two of template images (hyphy_hip_update_q_templates: the copy of
    // one update may still be queued when the next arrives)
    s.tstage_slot = (size_t)K * D * D + (p->DP == 64 ? (size_t)K * 64 * 64 : 0);
    const BlockReq blocks[] = {device_block(s.templates, (size_t)K * D * D * sizeof(double)),
                               device_block(s.coeffs, coeff_rows_cap * K * sizeof(double)),
                               pinned_block(s.h_coeffs, (size_t)4 * coeff_rows_cap * K * sizeof(double)),
                               device_block(s.templates_pad, p->DP == 64 ? (size_t)K * 64 * 64 * sizeof(double) : 0),
                               pinned_block(s.h_tstage, 2 * s.tstage_slot * sizeof(double))};
    s.own.drop(blocks, 5, FreeMode::Sync);
    s.d_hcoeffs = nullptr;
    s.coeff_rows_cap = 0;
    HIPCHK(s.own.get_group(blocks, 5));
    s.coeff_rows_cap = coeff_rows_cap;  // (grown on demand by hyphy_hip_build_q: rows per (class, branch, component))
    if (hipHostGetDevicePointer((void **)&s.d_hcoeffs, s.h_coeffs, 0) != hipSuccess) s.d_hcoeffs = nullptr;
    s.coeffs_cur = nullptr;
    s.coeff_rows = 0;
    s.coeff_kind = 0;
    s.coeff_slot = -1;
    s.qbuf_built = false;
    for (int k = 0; k < 4; k++) {
      s.coeff_busy[k] = false;
      if (!s.coeff_ev[k]) HIPCHK(hipEventCreateWithFlags(&s.coeff_ev[k], hipEventDisableTiming));
    }
    HIPCHK(hipMemcpy(s.templates, templates, (size_t)K * D * D * sizeof(double), hipMemcpyHostToDevice));
    if (s.templates_pad) {
      const std::vector<double> pad = padded_templates(templates, K, D);
      HIPCHK(hipMemcpy(s.templates_pad, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    for (int k = 0; k < 2; k++) {
      s.tstage_busy[k] = false;
      if (!s.tstage_ev[k]) HIPCHK(hipEventCreateWithFlags(&s.tstage_ev[k], hipEventDisableTiming));
    }
  }
  p->K = K;
  p->templates_host.assign(templates, templates + (size_t)K * D * D);
  for (Shard &s : p->shards) s.fit_static_current = false;
  return 0;
}

/* Replace the VALUES of the K templates (same K as hyphy_hip_set_q_templates): in-stream, no reallocation.  For hosts
 * whose templates depend on the global parameters of the current evaluation (template mode of the
 * adapter: Q_b = sum_k x_bk M_k(globals), M_k re-derived at every evaluation from K probe branches). */
int hyphy_hip_update_q_templates(hyphy_hip_partition *p, int64_t K, const double *templates) {
  if (!p || K < 1 || !templates) return fail("invalid templates");
  if (K != p->K) return hyphy_hip_set_q_templates(p, K, templates);
  const int64_t D = p->D;
  const size_t n = (size_t)K * D * D;
  if (p->templates_host.size() == n && !memcmp(p->templates_host.data(), templates, n * sizeof(double))) return 0;
  p->templates_host.assign(templates, templates + n);
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    // r04: through a pinned ring, in-stream, no wait on the host — the copies run behind whatever is queued on the stream and
    // ahead of the exponential launch that reads them (r03 copied from pageable memory and synchronised the stream twice:
    // ~40 us of every evaluation of a host whose templates follow its global parameters).  A slot is reused
    // two updates later; its event says when its copy has run.
    const int slot = (int)(s.tstage_turn++ & 1);
    if (s.tstage_busy[slot]) {
      HIPCHK(hipEventSynchronize(s.tstage_ev[slot]));
      s.tstage_busy[slot] = false;
    }
    double *st = s.h_tstage + (size_t)slot * s.tstage_slot;
    memcpy(st, templates, n * sizeof(double));
    HIPCHK(hipMemcpyAsync(s.templates, st, n * sizeof(double), hipMemcpyHostToDevice, s.stream));
    if (s.templates_pad) {  // [K][64*64]: zero padding, zero diagonals (padded_templates)
      double *pad = st + n;
      memset(pad, 0, (size_t)K * 64 * 64 * sizeof(double));
      for (int64_t k = 0; k < K; k++)
        for (int64_t r = 0; r < D; r++) {
          memcpy(pad + ((size_t)k * 64 + r) * 64, templates + ((size_t)k * D + r) * D, (size_t)D * sizeof(double));
          pad[((size_t)k * 64 + r) * 64 + r] = 0.;
        }
      HIPCHK(hipMemcpyAsync(s.templates_pad, pad, (size_t)K * 64 * 64 * sizeof(double), hipMemcpyHostToDevice, s.stream));
    }
    HIPCHK(hipEventRecord(s.tstage_ev[slot], s.stream));
    s.tstage_busy[slot] = true;
    s.fit_static_current = false;
  }
  return 0;
}

int hyphy_hip_build_q(hyphy_hip_partition *p, int64_t n, const double *coeffs) {
  if (!p || !p->K) return fail("build_q: templates not set");
  if (n < 0 || n > kMixRows * p->C * p->B || !coeffs) return fail("build_q: bad arguments");  // (most: a row per (class, branch, component))
  Trace tr("build_q");
  // When the matrices are consumed by the next hyphy_hip_evaluate_device(q_buffer) — the normal use —
  // the construction is fused into the expm kernel (no Q round trip through HBM, one launch less).
  // HYPHY_HIP_MATERIALIZE_Q=1 keeps the stand-alone kernel so that q_buffer can be read back.
  const bool fuse = !sw::materialize_q();
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    const size_t nbytes = (size_t)n * p->K * sizeof(double);
    if ((size_t)n > s.coeff_rows_cap) {
      // more rows than hyphy_hip_set_q_templates sized the ring for (a class batch of mixtures, C > 1): the ring and the device copy
      // grow, behind a wait for whatever may still read them; a partition that never stages so many keeps what it had
      HIPCHK(hipStreamSynchronize(s.stream));
      const size_t cap = (size_t)n;
      s.d_hcoeffs = nullptr, s.coeffs_cur = nullptr, s.coeff_slot = -1;
      for (int k = 0; k < 4; k++) s.coeff_busy[k] = false;
      HIPCHK(s.own.regrow({device_block(s.coeffs, cap * p->K * sizeof(double)), pinned_block(s.h_coeffs, (size_t)4 * cap * p->K * sizeof(double))},
                          s.coeff_rows_cap, (size_t)n, cap, FreeMode::Sync));
      if (hipHostGetDevicePointer((void **)&s.d_hcoeffs, s.h_coeffs, 0) != hipSuccess) s.d_hcoeffs = nullptr;
    }
    const int slot = (int)(s.coeff_turn++ & 3);  // pinned ring of 4
    if (s.coeff_busy[slot]) {  // a queued expm launch may still read this slot
      HIPCHK(hipEventSynchronize(s.coeff_ev[slot]));
      s.coeff_busy[slot] = false;
    }
    double *stage = s.h_coeffs + (size_t)slot * s.coeff_rows_cap * p->K;
    memcpy(stage, coeffs, nbytes);
    s.coeff_slot = slot;
    s.coeff_rows = n;
    s.coeff_kind = 0;  // (unclaimed: the first evaluation that consumes the rows says what they are)
    s.qbuf_built = !fuse;
    if (fuse && s.d_hcoeffs) {
      // the fused expm kernel reads the (few hundred) coefficients straight from the pinned ring slot over
      // PCIe: no copy kernel, no extra dependency in the stream
      s.coeffs_cur = s.d_hcoeffs + (stage - s.h_coeffs);
    } else {
      s.coeffs_cur = nullptr;
      HIPCHK(hipMemcpyAsync(s.coeffs, stage, nbytes, hipMemcpyHostToDevice, s.stream));
    }
    tr.lap("memcpy");
    if (!fuse) {
      if (n > p->C * p->B) return fail("build_q: HYPHY_HIP_MATERIALIZE_Q holds at most one matrix per (class, branch)");
      launch_build_q(s.templates, s.coeffs, (int)n, (int)p->K, (int)p->D, s.qbuf, s.stream);
    }
    tr.lap("launch");
  }
  p->coeffs_pending = fuse;
  return 0;
}

// Per-site batched fits (kernel and method: sitefit.hip).  The FEL family fits site-specific rate
// multipliers (FEL.bf:593-605: fel.alpha_scaler, fel.beta_scaler_test, fel.beta_scaler_nuisance) with one
// single-site likelihood function per site; this evaluates ALL patterns of the partition, each under its own
// multipliers, for n_sets candidate parameter vectors per pattern in one launch.
static int site_fits_common(hyphy_hip_partition *p, int64_t n_sets, int64_t n_groups, int64_t n_mix,
                            const int64_t *branch_group, const double *branch_coeffs, const double *site_mult,
                            const double *site_weights, const double *root_freqs, double *site_logl_out) {
  if (!p) return fail("partition == NULL");
  if (p->nuc) {
    g_last_error = "site fits: not available for the 4-state path";
    return 1;
  }
  if (!p->K || p->templates_host.empty()) return fail("site fits: templates not set (hyphy_hip_set_q_templates)");
  if (p->K > 4) {
    g_last_error = "site fits: at most 4 templates";
    return 1;
  }
  if (n_sets < 1 || n_sets > 65535 || n_groups < 1 || n_groups > 16 || n_mix < 1 || n_mix > 8)
    return fail("site fits: bad set / group / mixture-component count");
  if (!branch_group || !branch_coeffs || !site_mult || !root_freqs || !site_logl_out || (n_mix > 1 && !site_weights))
    return fail("site fits: null argument");
  if (finish_pending_async(p)) return -1;
  switch_mode(p, 0);  // (the per-site kernel walks the partition's own tree)
  const int64_t D = p->D, B = p->B, K = p->K, S = p->S;
  const int L = (int)p->L, I = (int)p->I, DP = p->DP, NW = p->NW;
  const int NKK = 4 * NW, TILE = NKK * 64;
  for (int64_t b = 0; b < B; b++)
    if (branch_group[b] < 0 || branch_group[b] >= n_groups) return fail("site fits: branch group out of range");
  for (int64_t b = 0; b < B * K; b++)
    if (!(branch_coeffs[b] >= 0.)) return fail("site fits: branch coefficients must be non-negative");
  for (int64_t k = 0; k < n_sets * S * n_mix * n_groups * K; k++)
    if (!(site_mult[k] >= 0.)) return fail("site fits: site multipliers must be non-negative");
  if (n_mix > 1)
    for (int64_t k = 0; k < n_sets * S * n_mix; k++)
      if (!(site_weights[k] >= 0.)) return fail("site fits: mixture weights must be non-negative");

  // schedule of a full pass, compiled for this kernel's slot budget (lazy persistence: only nodes that find no
  // parking slot are stored, to the scratch copy)
  if (p->fit_ops_host.empty()) {
    std::vector<int4> keep;
    keep.swap(p->ops_host);
    const int n_slots0 = p->n_slots;
    const bool persist0 = p->sched_persist;
    p->n_slots = 2 + kSiteFitParkSlots;
    p->sched_persist = false;
    std::vector<int> all(I);
    for (int n = 0; n < I; n++) all[n] = n;
    int off = 0, n = 0;
    emit_program(p, all, &off, &n);
    p->fit_ops_host.swap(p->ops_host);
    p->ops_host.swap(keep);
    p->n_slots = n_slots0;
    p->sched_persist = persist0;
    p->fit_n_ops = n;
    p->fit_spills = false;
    for (int e = 0; e < n; e++) {
      const int4 &op = p->fit_ops_host[e];
      if ((op.x & OPF_LAST) && !(op.x & OPF_NOPERSIST) && op.y != I - 1) p->fit_spills = true;
      if ((op.x & OPF_LAST) && op.y == I - 1) p->fit_ops_host[e].x |= OPF_NOPERSIST;  // the root is consumed in registers
    }
  }
  // template images with diagonals, A-operand layout (cf. the image writer in expm.hip); dmax_k = max_i |T_k[i][i]|
  SiteFitArgs fa;
  memset(&fa, 0, sizeof(fa));
  std::vector<double> img;
  {
    std::vector<double> full((size_t)D * D);
    img.assign((size_t)K * DP * DP, 0.0);
    for (int64_t k = 0; k < K; k++) {
      const double *T = p->templates_host.data() + (size_t)k * D * D;
      double dmax = 0.;
      for (int64_t i = 0; i < D; i++) {
        double rs = 0.;
        for (int64_t j = 0; j < D; j++) {
          if (j != i && !(T[i * D + j] >= 0.)) return fail("site fits: templates must have non-negative off-diagonal entries");
          if (j != i) rs += T[i * D + j];
          full[i * D + j] = T[i * D + j];
        }
        full[i * D + i] = -rs;
        dmax = std::max(dmax, rs);
      }
      fa.dmax[k] = dmax;
      double *out = img.data() + (size_t)k * DP * DP;
      for (int idx = 0; idx < DP * DP; idx++) {
        const int wb = idx / TILE, rem = idx - wb * TILE;
        const int kk2 = rem >> 7, l = (rem >> 1) & 63, kb = rem & 1, kk = 2 * kk2 + kb;
        const int rr = 16 * wb + (l & 15), cc = 4 * kk + (l >> 4);
        out[idx] = (rr < D && cc < D) ? full[(size_t)rr * D + cc] : 0.0;
      }
    }
  }
  {
    // reach: the largest finite distance between two states in the sparsity graph of ANY non-empty subset of the templates
    // (one BFS per state and subset: at most 15 x D sweeps).  A site whose multiplier of a template is zero, or negligible,
    // sees the graph of the remaining templates, and taking a template away can LENGTHEN finite distances, not only cut
    // paths (MG94: 3 in the union, 5 with the synonymous template off: ACC -> CCT).  An entry of exp(Q) first reached after d
    // steps of R is built by the terms d, d + 1, ... of the series alone; the kernel's relative stopping criterion looks
    // `reach` terms back (sitefit.hip).
    int reach = 0;
    std::vector<uint8_t> adj((size_t)D * D);
    std::vector<int> dist(D), queue(D);
    for (int mask = 1; mask < (1 << K); mask++) {
      std::fill(adj.begin(), adj.end(), 0);
      for (int64_t k = 0; k < K; k++) {
        if (!(mask >> k & 1)) continue;
        const double *T = p->templates_host.data() + (size_t)k * D * D;
        for (int64_t i = 0; i < D; i++)
          for (int64_t j = 0; j < D; j++)
            if (j != i && T[i * D + j] > 0.) adj[i * D + j] = 1;
      }
      for (int64_t src = 0; src < D; src++) {
        std::fill(dist.begin(), dist.end(), -1);
        int head = 0, tail = 0;
        dist[src] = 0;
        queue[tail++] = (int)src;
        while (head < tail) {
          const int u = queue[head++];
          for (int64_t v = 0; v < D; v++)
            if (adj[(size_t)u * D + v] && dist[v] < 0) {
              dist[v] = dist[u] + 1;
              queue[tail++] = (int)v;
            }
        }
        for (int64_t v = 0; v < D; v++) reach = std::max(reach, dist[v]);
      }
    }
    fa.reach = reach;
  }
  std::vector<int> grp(B);
  for (int64_t b = 0; b < B; b++) grp[b] = (int)branch_group[b];
  {
    // The series length of an edge grows linearly with its uniformisation rate mu = sum_k x_k dmax_k (sitefit.hip);
    // refuse parameter vectors that would keep a wave busy for seconds (rates this large mean "saturated" anyway).
    std::vector<double> cmax((size_t)n_groups * K, 0.0);  // per group and template: largest branch coefficient x dmax
    for (int64_t b = 0; b < B; b++)
      for (int64_t k = 0; k < K; k++)
        cmax[grp[b] * K + k] = std::max(cmax[grp[b] * K + k], branch_coeffs[b * K + k] * fa.dmax[k]);
    double mu_max = 0.;
    const size_t gk = (size_t)n_groups * K;
    for (int64_t r = 0; r < n_sets * S * n_mix; r++)
      for (int64_t g = 0; g < n_groups; g++) {
        double mu = 0.;
        for (int64_t k = 0; k < K; k++) mu += site_mult[r * gk + g * K + k] * cmax[g * K + k];
        mu_max = std::max(mu_max, mu);
      }
    if (!(mu_max <= kSiteFitMaxRate)) {
      char msg[160];
      snprintf(msg, sizeof msg, "site fits: uniformisation rate %.3g of some site and branch exceeds the limit %.3g "
               "(multipliers too large for this entry point)", mu_max, kSiteFitMaxRate);
      g_last_error = msg;
      return 1;
    }
  }
  std::vector<double> pi(DP, 0.0);
  for (int64_t k = 0; k < D; k++) pi[k] = root_freqs[k];
  const size_t GK = (size_t)n_mix * n_groups * K;  // multipliers per (set, pattern)

  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    if (!s.fit_Timg) {
      HIPCHK(s.own.get_group({device_block(s.fit_Timg, (size_t)4 * DP * DP * sizeof(double)), device_block(s.fit_bcoef, (size_t)B * 4 * sizeof(double)),
                              device_block(s.fit_bgroup, (size_t)B * sizeof(int)), device_block(s.fit_pi, (size_t)DP * sizeof(double)),
                              device_block(s.fit_ops, ops_capacity(p) * sizeof(int4))}));
      s.fit_static_current = false;
    }
    if (!s.fit_static_current) {
      if (p->fit_ops_host.size() > ops_capacity(p)) return fail("internal: site-fit schedule overflow");
      HIPCHK(hipMemcpy(s.fit_Timg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(s.fit_ops, p->fit_ops_host.data(), p->fit_ops_host.size() * sizeof(int4), hipMemcpyHostToDevice));
      s.fit_static_current = true;
    }
    const size_t need = (size_t)n_sets * std::max<size_t>(GK, 1);  // (doubles per pattern)
    const size_t set_bytes = need * s.S_pad * sizeof(double);
    HIPCHK(s.own.regrow({device_block(s.fit_smult, set_bytes), device_block(s.fit_out, set_bytes), device_block(s.fit_smix, set_bytes)},
                        s.fit_sets_cap, need, need, FreeMode::Sync));
    if (p->fit_spills && s.fit_scratch_sets < (size_t)n_sets) {
      const BlockReq scratch[] = {device_block(s.fit_scratch, (size_t)n_sets * I * s.ntiles * TILE * sizeof(double)),
                                  device_block(s.fit_scratch_cnt, (size_t)n_sets * I * s.S_pad * sizeof(int32_t))};
      s.own.drop(scratch, 2, FreeMode::Sync);
      s.fit_scratch_sets = 0;
      size_t free_b = 0, total_b = 0;
      hipMemGetInfo(&free_b, &total_b);
      if (scratch[0].bytes > free_b / 2) {
        g_last_error = "site fits: scratch for spilled nodes does not fit; use fewer parameter sets per call";
        return 1;
      }
      HIPCHK(s.own.get_group(scratch, 2));
      s.fit_scratch_sets = (size_t)n_sets;
    }
    // site multipliers of this shard's pattern range, padded with zeros (padding sites: exp(0) = I, weightless)
    std::vector<double> sm((size_t)n_sets * s.S_pad * GK, 0.0);
    for (int64_t st = 0; st < n_sets; st++)
      for (int64_t k = 0; k < s.S; k++)  // (per pattern: the device order is the sorted one)
        memcpy(sm.data() + ((size_t)st * s.S_pad + k) * GK, site_mult + ((size_t)st * S + caller_pattern(p, s.s0 + k)) * GK,
               (size_t)GK * sizeof(double));
    HIPCHK(hipMemcpyAsync(s.fit_smult, sm.data(), sm.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
    std::vector<double> wm;
    if (n_mix > 1) {  // mixture weights, same padding (they share the multipliers' allocation: need >= n_sets * n_mix)
      wm.assign((size_t)n_sets * s.S_pad * n_mix, 0.0);
      for (int64_t st = 0; st < n_sets; st++)
        for (int64_t k = 0; k < s.S; k++)
          memcpy(wm.data() + ((size_t)st * s.S_pad + k) * n_mix, site_weights + ((size_t)st * S + caller_pattern(p, s.s0 + k)) * n_mix,
                 (size_t)n_mix * sizeof(double));
      HIPCHK(hipMemcpyAsync(s.fit_smix, wm.data(), wm.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
    }
    HIPCHK(hipMemcpyAsync(s.fit_bcoef, branch_coeffs, (size_t)B * K * sizeof(double), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(s.fit_bgroup, grp.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(s.fit_pi, pi.data(), (size_t)DP * sizeof(double), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemsetAsync(s.status, 0, sizeof(int32_t), s.stream));
    fa.ops = s.fit_ops;
    fa.n_ops = p->fit_n_ops;
    fa.NW = NW;
    fa.L = L;
    fa.I = I;
    fa.ntiles = s.ntiles;
    fa.S_pad = s.S_pad;
    fa.K = (int)K;
    fa.G = (int)n_groups;
    fa.n_sets = (int)n_sets;
    fa.Timg = s.fit_Timg;
    fa.bcoef = s.fit_bcoef;
    fa.bgroup = s.fit_bgroup;
    fa.smult = s.fit_smult;
    fa.n_mix = (int)n_mix;
    fa.smix = s.fit_smix;
    fa.codes_tile = s.codes_tile;
    fa.ambig = s.ambig;
    fa.pi = s.fit_pi;
    fa.freq = s.freq;
    fa.scratch = s.fit_scratch;
    fa.scratch_cnt = s.fit_scratch_cnt;
    fa.site_logl = s.fit_out;
    fa.status = s.status;
    HIPCHK(hipEventRecord(s.ev[0], s.stream));
    launch_site_fit(fa, s.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev[1], s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));  // (the staging vectors go out of scope)
    {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess) p->fit_kernel_ms = std::max(&s == &p->shards[0] ? 0.0 : p->fit_kernel_ms, (double)ms);
    }
    std::vector<double> out((size_t)n_sets * s.S_pad);
    int32_t st = 0;
    HIPCHK(hipMemcpy(out.data(), s.fit_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&st, s.status, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemsetAsync(s.status, 0, sizeof(int32_t), s.stream));
    if (st) return fail("site fits: a site likelihood is not a number");
    for (int64_t k = 0; k < n_sets; k++)
      for (int64_t j = 0; j < s.S; j++) site_logl_out[(size_t)k * S + caller_pattern(p, s.s0 + j)] = out[(size_t)k * s.S_pad + j];
  }
  return 0;
}


int hyphy_hip_site_fits_evaluate(hyphy_hip_partition *p, int64_t n_sets, int64_t n_groups, const int64_t *branch_group,
                                 const double *branch_coeffs, const double *site_mult, const double *root_freqs,
                                 double *site_logl_out) {
  return site_fits_common(p, n_sets, n_groups, 1, branch_group, branch_coeffs, site_mult, nullptr, root_freqs, site_logl_out);
}

// Branch-site mixtures per site (MEME / BS-REL style "explicit form" models): on every branch the transition
// matrix of site s is P = sum_m site_weights[s][m] exp(Q^(m)_{b,s}); the series runs once per component (sitefit.hip).
int hyphy_hip_site_fits_evaluate_mixture(hyphy_hip_partition *p, int64_t n_sets, int64_t n_groups, int64_t n_mix,
                                         const int64_t *branch_group, const double *branch_coeffs, const double *site_mult,
                                         const double *site_weights, const double *root_freqs, double *site_logl_out) {
  return site_fits_common(p, n_sets, n_groups, n_mix, branch_group, branch_coeffs, site_mult, site_weights, root_freqs,
                          site_logl_out);
}

double hyphy_hip_site_fits_kernel_ms(const hyphy_hip_partition *p) { return p ? p->fit_kernel_ms : 0.; }

double *hyphy_hip_q_buffer(hyphy_hip_partition *p) { return p && !p->shards.empty() ? p->shards[0].qbuf : nullptr; }

int hyphy_hip_synchronize(hyphy_hip_partition *p) {
  if (!p) return fail("partition == NULL");
  for (Shard &s : p->shards) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipStreamSynchronize(s.stream));
  }
  return 0;
}

int hyphy_hip_set_stream(hyphy_hip_partition *p, void *stream) {
  if (!p) return fail("partition == NULL");
  if (p->shards.size() != 1) return fail("set_stream needs a single-device partition");
  Shard &s = p->shards[0];
  HIPCHK(hipSetDevice(s.device));
  HIPCHK(hipStreamSynchronize(s.stream));
  s.stream = (stream == HYPHY_HIP_OWN_STREAM) ? s.own_stream : (hipStream_t)stream;
  return 0;
}

void *hyphy_hip_stream(hyphy_hip_partition *p) { return p && !p->shards.empty() ? (void *)p->shards[0].stream : nullptr; }

int hyphy_hip_set_timing_detail(hyphy_hip_partition *p, int on) {
  if (!p) return fail("partition == NULL");
  p->all_timings = on != 0;
  return 0;
}

int hyphy_hip_last_timings(hyphy_hip_partition *p, double out[3]) {
  if (!p || !out) return fail("null argument");
  if (hipSetDevice(p->shards[0].device) != hipSuccess) return fail("hipSetDevice failed");
  hipStreamSynchronize(p->shards[0].stream);
  record_timings(p);
  for (int k = 0; k < 3; k++) out[k] = p->timings[k];
  return 0;
}

}  // extern "C"
