/*
 * hyphy_hip.h — C-ABI of the MI355X-native phylogenetic likelihood core.
 *
 * This is the drop-in boundary for the ONE hot path of veg/hyphy that this repository
 * replaces:
 *
 *   _LikelihoodFunction::ComputeBlock            src/core/likefunc.cpp:10783-11289
 *     -> _TheTree::ExponentiateMatrices          src/core/tree.cpp:2932-3113
 *          -> _Matrix::Exponentiate              src/core/matrix.cpp:5537-5951
 *     -> _TheTree::ComputeTreeBlockByBranch      src/core/tree_evaluator.cpp:3556-4171
 *     -> Neumaier combine, - logU * scalers      src/core/likefunc.cpp:11046-11123
 *
 * The reference has no plug-in/FFI interface; its (dead) OpenCL hook shows the seam:
 * construct per partition in SetupLFCaches (likefunc.cpp:4182-4183, 4313-4316), destroy in
 * DeleteCaches/Cleanup (likefunc.cpp:10546-10551, 10594-10599) and one call from ComputeBlock
 * (historically launchmdsocl(...), likefuncocl.cpp:1043-1053).  The entry points below are
 * exactly what a HyPhy host adapter binds at those three touch-points (INTEGRATION.md shows
 * the patch).  Plain C: opaque handle, pointers and sizes only — no C++ or torch types.
 *
 * Conventions
 *   - all sizes int64_t, all reals double (hyFloat, include/hy_types.h:57)
 *   - return 0 = ok; > 0 = "unsupported here, use the CPU path" (no state change);
 *     < 0 = hard error, text in hyphy_hip_last_error() (adapter -> HandleApplicationError,
 *     likefunc.cpp:11284)
 *   - host arrays are borrowed for the duration of the call only
 *   - node codes: n < L is leaf n, n >= L is internal node n-L; both in post-order, root
 *     last (tree.cpp:722-766).  P[i*D+j] = Pr(parent state i -> child state j)
 *   - never called concurrently for one partition (ComputeBlock is entered from the HBL
 *     interpreter's single thread; the library replaces the OpenMP region inside it)
 *   - there is NO CPU fallback inside the library: without a usable MI355X every compute
 *     entry point returns < 0.
 */
#ifndef HYPHY_HIP_H
#define HYPHY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hyphy_hip_partition hyphy_hip_partition; /* device-side state of ONE (filter, tree) partition */

/*
 * Environment switches.  The library works without any of them; a host integrator needs at most the ones listed here (the rows marked
 * `integrator` of the table in hyphy_amd/csrc/switches.h, which is the one place that reads the environment; docs/switches.md is that
 * table as a page, hyphy_hip_plan_switches() returns it with what every switch parses to right now):
 *   HYPHY_HIP_VERBOSE=1           what was decided and why (schedule tuner, subtree repeats on / off, generated kernels) on stderr
 *   HYPHY_HIP_POOL_MB=n           device / pinned blocks of destroyed partitions kept for the next one of the same shape (MiB per kind,
 *                                 default 1024; 0: nothing is kept); read once per process
 *   HYPHY_HIP_CACHE=always        every pass stores every node's conditionals (default: lazy persistence, see hyphy_hip_download_partials)
 *   HYPHY_HIP_TUNE=0              no run-time schedule measurement (with HYPHY_HIP_CUT=levels: bit-identical repeats, see below)
 *   HYPHY_HIP_CUT=levels          fixed multiplication order, no arrival-order joins
 *   HYPHY_HIP_REPEATS=0|1         subtree repeats (the reference's `tcc`) never / always, instead of decided by measurement
 *   HYPHY_HIP_NUCGEN=0|2          4 states: never generate straight-line kernels / compile them synchronously at the first full pass
 *   HYPHY_HIP_NUCGEN_AFTER=n      ... evaluations under one schedule before its kernel is compiled in the background (default 8)
 *   HYPHY_HIP_COMBINE=rccl        one process, several devices: sum the shard partials by one RCCL group all-reduce instead of on the host
 *   HYPHY_HIP_EXCHANGE_TIMEOUT_S  one process per GPU, host-side exchange: how long a rank waits for the others (default 120)
 *   HYPHY_HIP_TIMING_EVERY=n      one evaluation in n carries the kernel-duration stamp (default 16; read once per process):
 *                                 hyphy_hip_last_timings, hyphy_hip_prune_timings
 *   HYPHY_HIP_ALL_TIMINGS         (set to anything) the initial state of hyphy_hip_set_timing_detail
 *   HYPHY_HIP_TRIALS_MB, HYPHY_HIP_JOINT_MB, HYPHY_HIP_SAMPLE_MB, HYPHY_HIP_SIMULATE_MB
 *                                 scratch budgets (MiB, default 1024, read at every call) of hyphy_hip_branch_trials, _joint_ancestral,
 *                                 _sample_ancestral and _simulate, described at those entry points
 * The table says of every switch WHEN it is read: once per process (then cached), while a partition is created, or by every call.
 * Everything else that starts with HYPHY_HIP_ is a DIAGNOSTIC of the kernels' authors: it forces one of the forms the tuner chooses
 * between, turns a mechanism off for an A/B run or writes a trace; docs/switches.md lists them all, with the file that consults each.
 * The tests use them to reach every form; a host should not.  (The adapter of INTEGRATION.md has a handful of variables of its own, which
 * the library never reads: HYPHY_HIP=1 turns it on, HYPHY_HIP_DEVICE(S), HYPHY_HIP_WORLD / _RANK / _LOCAL_RANK / _RUN_ID / _UID_FILE /
 * _COLLECTIVE for one process per GPU, HYPHY_HIP_DEVICE_EXPM, HYPHY_HIP_TEMPLATES, HYPHY_HIP_MIXTURES, HYPHY_HIP_CAT_BATCH.)
 */

/* Number of usable gfx950 devices (0 if none / no HIP runtime). */
int hyphy_hip_device_count(void);

/*
 * Replaces the allocation half of _LikelihoodFunction::SetupLFCaches (likefunc.cpp:4163-4319)
 * for one partition: conditional-likelihood caches (conditionalInternalNodeLikelihoodCaches,
 * :4220-4223), scaling state (siteScalingFactors :4232, siteCorrections :4238-4246), the leaf
 * state table (conditionalTerminalNodeStateFlag :4235-4236, :4305) and the ambiguity vectors
 * (conditionalTerminalNodeLikelihoodCaches :4263-4311) all live on the device afterwards.
 *
 *   D,S,L,I,C       GetDimension, GetPatternCount, GetLeafCount, GetINodeCount, categoryCount
 *   flat_parents    [L+I] parent as internal index, root = -1            (tree.cpp:746-757)
 *   leaf_codes      [L*S] pattern-indexed; >= 0 state, < 0 -> -(k+1) = ambiguity vector k
 *   ambig           [n_ambig*D]
 *   pattern_freq    [S] theFrequencies
 *   device_first, device_count
 *                   patterns are sharded in contiguous ranges over devices
 *                   device_first .. device_first+device_count-1 of THIS process (the
 *                   reference's OpenMP site blocks, likefunc.cpp:10995-11044).  One rank per
 *                   GPU (torch.distributed / HYPHYMPI) passes device_count = 1 and its own
 *                   shard of the patterns.
 * Returns > 0 (unsupported) for D > 64 or D < 2 in this version.
 */
int hyphy_hip_create(hyphy_hip_partition **out, int64_t D, int64_t S, int64_t L, int64_t I, int64_t C,
                     const int64_t *flat_parents, const int64_t *leaf_codes, const double *ambig,
                     int64_t n_ambig, const int64_t *pattern_freq, int device_first, int device_count);

/* Replaces DeleteCaches (likefunc.cpp:10556-10600) for the partition. NULL is a no-op.  The partition's device and pinned host
 * blocks and its stream are kept for the next hyphy_hip_create of the same shape in this process (analyses that build one
 * likelihood function per site: FEL); HYPHY_HIP_POOL_MB caps what is kept (MiB per kind, default 1024, 0: nothing). */
void hyphy_hip_destroy(hyphy_hip_partition *p);

/*
 * One likelihood evaluation of rate class `cat` (-1 == 0 when C == 1): replaces, inside
 * ComputeBlock, ExponentiateMatrices (likefunc.cpp:10978-10980) AND the OpenMP pruning loop
 * + combine (likefunc.cpp:10995-11123).
 *
 *   update_nodes    node codes from _TheTree::DetermineNodesForUpdate (tree.cpp:3117-3331),
 *                   ascending; on the first evaluation after create: all L+I-1 branches
 *                   (likefunc.cpp:10965-10967).  The library recomputes every internal node
 *                   that is the parent of a listed node, from ALL of that node's children.
 *   q_nodes/q_dense node codes whose transition matrix changed and their numeric rate
 *                   matrices [n_q*D*D], already multiplied by the branch length, MultByFreqs
 *                   applied (what _CalcNode::RecomputeMatrix hands to SetCompExp,
 *                   calcnode.cpp:526-735).  q_is_probability = 1: q_dense already holds
 *                   P = exp(Q) (host did the exponential, e.g. explicit-form mixtures
 *                   P = sum_k w_k exp(Q_k), tree.cpp:3047-3090).
 *   root_freqs      [D] theProbs (InitializeTreeFrequencies, tree.cpp:2436-2451)
 *   logl_out        sum_s f_s log L_s - 64 ln2 * scalers — the value ComputeBlock returns
 *                   (likefunc.cpp:11123).  -INFINITY if a pattern has likelihood 0
 *                   (tree_evaluator.cpp:4094-4112); NaN propagates (adapter then calls
 *                   _TerminateAndDump as tree_evaluator.cpp:4142 does): a pattern whose likelihood is NaN or +INFINITY (a NaN in a
 *                   matrix handed over with q_is_probability = 1, in root_freqs, or in an ambiguity vector) makes log L NaN, and
 *                   NaN wins over -INFINITY when both occur.
 *                   A pattern of frequency 0 takes no part in either sum, whatever its likelihood: zero, NaN or finite, it
 *                   contributes nothing and raises neither flag (every combiner skips f_s == 0; the per-pattern outputs still
 *                   carry its values).
 *                   A matrix the device cannot exponentiate (NaN, overflow, or a rate matrix with a POSITIVE diagonal entry —
 *                   which the reference restarts its way to the identity for, matrix.cpp:5854-5864) is a hard error (< 0,
 *                   "Failed to compute a valid transition matrix"); an asynchronous evaluation's log-L is then NaN.
 *   site_lik_out    optional [S], pattern-indexed == storageVec (tree_evaluator.cpp:4080):
 *                   per-pattern likelihood l_s (NOT log), scaled so that the true value is
 *                   l_s * 2^(-64*c_s)
 *   site_scaler_out optional [S] == the siteCorrections slice: c_s.  Only differences of c_s
 *                   between rate classes and sum_s f_s c_s are observable upstream
 *                   (likefunc2.cpp:736-770, 828-853, 1484-1506).
 *
 * Reproducibility: steady-state full passes run on chain schedules whose joins multiply the children of a node in the
 * order in which their workgroups arrive, and the schedule itself is chosen by timing (HYPHY_HIP_TUNE): the same inputs can
 * give log-likelihoods that differ in the last bits (<= a few 1e-16 relative) between runs and between ranks.  The reference's
 * CPU path is deterministic for a fixed thread count; a host that needs bit-identical repeats sets
 * HYPHY_HIP_TUNE=0 HYPHY_HIP_CUT=levels (fixed order, no joins; ~25 % slower at the headline size on the plain form).  r06: with
 * HYPHY_HIP_TUNE=0 alone a partition that runs class-compressed (subtree repeats; 49-64 states from ~128 tiles of 16 patterns per
 * shard) is bit-identical from run to run too, at the speed of the tuned form — its two walks have no join whose result depends on who
 * arrives first (tests/test_gpu_fullsize.py::test_class_compressed_form_without_tuner_is_bit_reproducible); smaller partitions
 * of that mode still run chain schedules: add HYPHY_HIP_CUT=levels there.
 */
int hyphy_hip_evaluate(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                       const int64_t *q_nodes, int64_t n_q, const double *q_dense, int q_is_probability,
                       const double *root_freqs, double *logl_out, double *site_lik_out,
                       int64_t *site_scaler_out);

/*
 * hyphy_hip_evaluate for models in the reference's "explicit form" (BUSTED, BS-REL, RELAX — the model is a
 * formula of matrix exponentials, `Model M = ("Exp(Q1)*w1+Exp(Q2)*w2...", freqs, EXPLICIT_FORM_MATRIX_EXPONENTIAL)`,
 * res/TemplateBatchFiles/libv3/models/codon/BS_REL.bf:34-60): the host's ExponentiateMatrices queues the Exp() arguments
 * of every branch (variablecontainer.cpp:208-233), exponentiates each and recombines them through the formula
 * (tree.cpp:3047-3090).  Here branch q_nodes[k] comes with n_components[k] numeric rate matrices (consecutive in
 * q_dense) and their mixture weights; the device exponentiates all of them in one launch and forms
 * P_k = sum_m weights[.] exp(Q[.]) directly in the layouts the pruning kernels read.  n_components[k] is 1..16 and may differ
 * from branch to branch; the components are consecutive, branch-major.
 * A component the device cannot exponentiate (NaN, overflow, a positive diagonal entry: see hyphy_hip_evaluate) fails the whole
 * call with "Failed to compute a valid transition matrix" (< 0) WHATEVER ITS WEIGHT, weight 0 included: every listed component is
 * exponentiated and raises the status word on its own, and the NaN it leaves would reach the images through 0 * NaN anyway.  The
 * listed branches are then without usable matrices (never their previous ones): a full pass with good matrices on the same
 * partition gives the value a fresh partition gives (tests/test_gpu_mixture.py::test_a_bad_component_never_gives_a_finite_value).
 * A caller that wants a component out of the mixture leaves it out of the list.
 */
int hyphy_hip_evaluate_mixture(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                               const int64_t *q_nodes, int64_t n_q, const int64_t *n_components /* [n_q] */,
                               const double *q_dense /* [sum n_components][D*D] */, const double *weights /* [sum n_components] */,
                               const double *root_freqs, double *logl_out, double *site_lik_out, int64_t *site_scaler_out);

/*
 * hyphy_hip_evaluate_mixture with the component rate matrices formed ON THE DEVICE (r04): BS-REL / BUSTED / RELAX components
 * differ in GLOBAL parameters only (omega_m: res/TemplateBatchFiles/libv3/models/codon/BS_REL.bf:48), so component m of branch b is
 * Q_(b,m) = sum_k x_(b,m),k T_k over the templates of hyphy_hip_set_q_templates / hyphy_hip_update_q_templates — the host's
 * serial pass that evaluates every component's formulas for every branch (calcnode.cpp:526-704 behind
 * variablecontainer.cpp:208-233) and the dense matrices over PCIe both go away.  Protocol: hyphy_hip_build_q(p, n, coeffs) with
 * n = sum of n_components rows of K coefficients, branch-major (the components of q_nodes[0], then those of q_nodes[1], ...),
 * then this call; the rows are consumed inside the exponential kernel (no rate matrix is ever materialised).  At most 16
 * components per branch.  Everything else as hyphy_hip_evaluate_mixture.
 */
int hyphy_hip_evaluate_mixture_built(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                     const int64_t *q_nodes, int64_t n_q, const int64_t *n_components /* [n_q] */,
                                     const double *weights /* [sum n_components] */, const double *root_freqs, double *logl_out,
                                     double *site_lik_out, int64_t *site_scaler_out);

/*
 * The same evaluation split in two, so that the partitions of one likelihood function overlap (different devices, or
 * different streams of one device): enqueue every partition, then collect.  The reference's partition loop in
 * _LikelihoodFunction::Compute (src/core/likefunc.cpp:2524-2589) calls ComputeBlock(partID) serially and its MPI
 * partition mode (:2708-2768) farms the partitions out; the adapter's pre-pass does the former on
 * N devices.  evaluate_async copies the matrices to a pinned staging buffer (host arrays are free on return) and
 * returns as soon as everything is enqueued; collect waits and returns what hyphy_hip_evaluate returns.  Any other
 * evaluation entry point called in between finishes the pending evaluation first.
 */
int hyphy_hip_evaluate_async(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                             const int64_t *q_nodes, int64_t n_q, const double *q_dense, int q_is_probability,
                             const double *root_freqs);
int hyphy_hip_collect(hyphy_hip_partition *p, double *logl_out, double *site_lik_out, int64_t *site_scaler_out);

/*
 * The all-reduce of the partition log-likelihood over RCCL / xGMI, reachable from a C++ host (north_star: "a single RCCL
 * allreduce of the partition log-likelihood over xGMI per evaluation").  librccl.so is loaded on first use.
 *   one process per GPU:   rank 0: hyphy_hip_comm_unique_id(id) -> the host broadcasts the 128 bytes (MPI_Bcast in a
 *                          HYPHYMPI build, a file ...) -> every rank: hyphy_hip_comm_init_rank(p, id, rank, n) on the
 *                          partition that holds ITS pattern shard -> hyphy_hip_evaluate_allreduce(...) returns the
 *                          log-likelihood of the whole alignment on every rank (evaluate + one ncclAllReduce of one
 *                          double, in the partition's stream).  hyphy_hip_allreduce_device is the bare in-stream sum
 *                          for callers of hyphy_hip_evaluate_device.
 *   one process, N GPUs:   hyphy_hip_create(device_count = N) + hyphy_hip_comm_init_all(p): with HYPHY_HIP_COMBINE=rccl
 *                          hyphy_hip_evaluate / hyphy_hip_evaluate_built sum the shard partials by ONE group all-reduce
 *                          instead of on the host (default: host-side Neumaier combine, likefunc.cpp:11046-11093).
 */
int hyphy_hip_comm_unique_id(void *out128);
int hyphy_hip_comm_init_rank(hyphy_hip_partition *p, const void *unique_id, int rank, int n_ranks);
int hyphy_hip_comm_init_all(hyphy_hip_partition *p);
int hyphy_hip_allreduce_device(hyphy_hip_partition *p, double *d_value);
int hyphy_hip_evaluate_allreduce(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                 const int64_t *q_nodes, int64_t n_q, const double *q_dense, int q_is_probability,
                                 const double *root_freqs, double *logl_out);
/* ... behind hyphy_hip_build_q (template models; the step `bench.py --gpus N` times): local construction + exponentials +
 * pruning + reduction, one ncclAllReduce of one double on the partition's stream, the sum back through the host-mapped
 * record.  A rank whose local evaluation fails still joins the collective (with NaN) and then returns its error: no rank
 * is left waiting.  hyphy_hip_last_allreduce_ms: event-timed duration of the last in-stream all-reduce while
 * hyphy_hip_set_timing_detail is on (else 0). */
int hyphy_hip_evaluate_built_allreduce(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                       const int64_t *q_nodes, int64_t n_q, const double *root_freqs, double *logl_out);
double hyphy_hip_last_allreduce_ms(const hyphy_hip_partition *p);

/* The collective-free combine of one process per GPU on ONE node (r06): what the single-process form does with its shards — partials
 * back over PCIe into host-mapped records, the reference's Neumaier combine on the host (likefunc.cpp:11046-11093) — between processes,
 * through a POSIX shared-memory segment: each rank finishes its local evaluation like a one-GPU run, posts (value, epoch) into its slot and
 * reads the others' (one release store, N - 1 acquire loads; no device work).  Same bits on every rank (summed in rank order).
 *   hyphy_hip_comm_init_host            `name`: the same string on every rank, unique per run; returns when every rank has attached
 *   hyphy_hip_evaluate(_built)_exchange hyphy_hip_evaluate(_built) + one exchange; a rank whose local evaluation fails still posts (NaN)
 *                                       and then returns its own error: nobody is left waiting (HYPHY_HIP_EXCHANGE_TIMEOUT_S, default 120)
 *   hyphy_hip_xch_open / _sum / _close  the exchange alone (no partition, no device).
 * RCCL (above) stays the C-ABI's and the adapter's default collective; bench.py --gpus N times both and uses the faster (collective_ab). */
int hyphy_hip_comm_init_host(hyphy_hip_partition *p, const char *name, int rank, int n_ranks);
int hyphy_hip_evaluate_exchange(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update, const int64_t *q_nodes,
                                int64_t n_q, const double *q_dense, int q_is_probability, const double *root_freqs, double *logl_out);
int hyphy_hip_evaluate_built_exchange(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                      const int64_t *q_nodes, int64_t n_q, const double *root_freqs, double *logl_out);
int hyphy_hip_xch_open(const char *name, int rank, int n_ranks, void **handle_out);
int hyphy_hip_xch_sum(void *handle, double local, int local_failed, double *sum_out);
void hyphy_hip_xch_close(void *handle);

/*
 * Same evaluation with device-resident inputs/outputs, enqueued asynchronously on the
 * partition's stream (device_count must be 1): d_q is a DEVICE pointer [n_q*D*D];
 * d_logl_out a DEVICE pointer to one double that receives this shard's partial
 * log-likelihood (ready for an RCCL all-reduce across site-sharded ranks).  Call
 * hyphy_hip_synchronize() (or synchronise the stream) before reading it.
 */
int hyphy_hip_evaluate_device(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                              const int64_t *q_nodes, int64_t n_q, const double *d_q, int q_is_probability,
                              const double *root_freqs, double *d_logl_out);

/* Reads one double that lives in device memory and is produced by work queued on the partition's stream — the log-likelihood
 * summed over ranks by the caller's own collective (RCCL all-reduce behind hyphy_hip_evaluate_device, SURVEY 8e: the
 * reference's MPI ranks) — through the host-mapped result record: a one-thread kernel posts it, the host spins on the record's
 * sequence word.  Replaces a device-to-host copy + stream synchronisation per evaluation.  Single-device partitions. */
int hyphy_hip_fetch_device_scalar(hyphy_hip_partition *p, const double *d_value, double *value_out);

/*
 * Rate-category batch (config "BUSTED 3-rate-class"): evaluates ALL C classes in one
 * schedule (classes are an extra batch dimension on the device) and mixes them exactly as
 * PopulateConditionalProbabilities' weighted-sum mode + SumUpSiteLikelihoods do
 * (likefunc2.cpp:820-853, 1484-1506).  q_dense is [C][n_q][D*D]; weights [C].
 * The category floor: a pattern of frequency f whose MIXED likelihood is zero (impossible under every class) contributes exactly
 * -1e6 * f to logl_out, with no exponent, and no -INFINITY (myLog, likefunc.cpp:644-661); a pattern impossible under some classes
 * only is an ordinary finite term.  Only this entry point and its _built forms floor: hyphy_hip_evaluate answers -INFINITY, and so
 * does hyphy_hip_branch_trials for C > 1.  NaN still propagates, and frequency-0 patterns are skipped as in hyphy_hip_evaluate.
 */
int hyphy_hip_evaluate_categories(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                  const int64_t *q_nodes, int64_t n_q, const double *q_dense,
                                  int q_is_probability, const double *weights, const double *root_freqs,
                                  double *logl_out, double *site_lik_out, int64_t *site_scaler_out);

/* The same from rate matrices staged by hyphy_hip_build_q (n = C*n_q coefficient rows, class-major). */
int hyphy_hip_evaluate_categories_built(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                        const int64_t *q_nodes, int64_t n_q, const double *weights,
                                        const double *root_freqs, double *logl_out);
/* ... with the mixed per-pattern values: site_lik_out [S] / site_scaler_out [S] as hyphy_hip_evaluate_categories returns them (what
 * PopulateConditionalProbabilities' weighted-sum mode leaves in its buffer and scalers, likefunc2.cpp:772-859); either may be NULL.
 * The adapter's category hook answers the host's whole class loop with this one call ("rate classes"). */
int hyphy_hip_evaluate_categories_built_sites(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                              const int64_t *q_nodes, int64_t n_q, const double *weights,
                                              const double *root_freqs, double *logl_out, double *site_lik_out,
                                              int64_t *site_scaler_out);

/*
 * Rate classes OVER branch-site mixtures in one batched evaluation (BUSTED with --srv, its default: three synonymous-rate classes
 * over a model that is already an explicit-form mixture of three omega components on every branch,
 * res/TemplateBatchFiles/SelectionAnalyses/BUSTED.bf:116, :192; RELAX and aBSREL with --srv have the same shape).  Class c evolves on
 * branch q_nodes[k] under P = sum_m mix_weights[c][.] exp(Q[c][.]); the classes are then mixed by class_weights exactly as
 * hyphy_hip_evaluate_categories mixes them: the category floor of -1e6 * f, NaN propagates, frequency-0 patterns are skipped, and the
 * per-pattern outputs are the mixed (likelihood, exponent) in the caller's pattern order.
 *   n_components [n_q]      1..16 components per branch, a count of its own on each, THE SAME COUNTS IN EVERY CLASS; n_tot = their sum
 *   q_dense [C][n_tot][D*D] class-major, inside a class branch-major (the components of q_nodes[0], then those of q_nodes[1], ...)
 *   mix_weights [C][n_tot]  in the same order;  class_weights [C]
 * The device exponentiates all C * n_tot components in ONE launch (hyphy_hip_last_expm_kernel names it), forms both matrix images of
 * every (class, branch) with one workgroup each, and prunes every class in one launch.  C == 1 is accepted.  n_q == 0 is accepted (a
 * re-mix under new class weights, or a pure update list): the component arguments may then be NULL and no staged rows are consumed.
 * As for the other entry points: the first evaluation of a class lists every branch; a failed call commits nothing; the branch caches
 * of every class are invalidated; a later one-class call on any class works; the per-class values, matrices and images stay resident
 * (hyphy_hip_hmm_logl / _viterbi, hyphy_hip_download_partials, hyphy_hip_branch_cache_build, the ancestral entry points and
 * hyphy_hip_simulate work behind such a pass).  A component that cannot be exponentiated fails the call whatever its weight (< 0,
 * "Failed to compute a valid transition matrix"); the listed branches are then without usable matrices in EVERY class, and a full
 * pass with good matrices gives what a fresh partition gives.  4-state partitions run the classes one after another through the
 * staging of hyphy_hip_evaluate_mixture, as hyphy_hip_evaluate_categories does.  hyphy_hip_last_reduce_form answers what it answers
 * behind hyphy_hip_evaluate_categories.
 */
int hyphy_hip_evaluate_categories_mixture(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                          const int64_t *q_nodes, int64_t n_q, const int64_t *n_components /* [n_q] */,
                                          const double *q_dense /* [C][n_tot][D*D] */, const double *mix_weights /* [C][n_tot] */,
                                          const double *class_weights /* [C] */, const double *root_freqs, double *logl_out,
                                          double *site_lik_out /* [S] or NULL */, int64_t *site_scaler_out /* [S] or NULL */);
/* The same with the components formed on the device: hyphy_hip_build_q(p, C * n_tot, ...) stages one row per (class, branch,
 * component), in that order (the layout of the adapter's template mode, class c's row at its own template columns); up to 16 * C *
 * (L + I - 1) rows.  Refused: a different number of rows than the call consumes, and rows an evaluation of another kind — one row per
 * (class, branch), or per (branch, component) of one class — has already consumed.  MFMA partitions only, as
 * hyphy_hip_evaluate_categories_built.  With the lists and counts of the previous call the host waits once, for the result record:
 * the weights travel through pinned staging in-stream, and the offsets are uploaded only when the counts or the list change. */
int hyphy_hip_evaluate_categories_mixture_built(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update,
                                                const int64_t *q_nodes, int64_t n_q, const int64_t *n_components /* [n_q] */,
                                                const double *mix_weights /* [C][n_tot] */, const double *class_weights /* [C] */,
                                                const double *root_freqs, double *logl_out, double *site_lik_out,
                                                int64_t *site_scaler_out);

/*
 * Copies device partials back in the reference's host layout for code that reads the caches
 * directly (ReconstructAncestors likefunc2.cpp:416-449, FillInConditionals tree.cpp:3335-3371):
 *   inode_cache [I*S*D]  iNodeCache[(node*S + pattern)*D + state] (tree_evaluator.cpp:3608-3617)
 *   scaler_counts [I*S]  cumulative 2^64-exponent of the subtree below (node, pattern): the
 *                        stored vector times 2^(-64*count) is the unscaled conditional.
 * Cache policy: by default ("lazy"; environment HYPHY_HIP_CACHE=always disables it) a full pass that follows a
 * full pass — a sweep over a global parameter — does not store its conditionals in HBM; nothing can read them
 * before the next full pass overwrites them.  This call, a partial update and hyphy_hip_branch_cache_build
 * first re-run a storing pass when the resident copies are stale, so callers never observe the difference.
 */
int hyphy_hip_download_partials(hyphy_hip_partition *p, int64_t cat, double *inode_cache, int64_t *scaler_counts);

/*
 * Stand-alone batched matrix exponential: drop-in for the OpenMP loop in ExponentiateMatrices
 * (tree.cpp:3011-3037, each iteration = _Matrix::Exponentiate(1., true, storage)).
 * q_dense, p_out: host [n*D*D].  Rows of P sum to 1 (diag_populator, matrix.cpp:5837-5852).
 */
int hyphy_hip_expm_batch(int64_t D, int64_t n, const double *q_dense, double *p_out);

/*
 * Device-side rate-matrix construction for template models: every branch's
 * numeric Q is a linear combination of K fixed D x D templates,
 *       Q_b = sum_k coeff[b][k] * T_k   (off-diagonal),   Q_b[i][i] = -sum_{j != i} Q_b[i][j]
 * e.g. MG94xREV with fixed nucleotide biases: T_0 = synonymous part, T_1 = non-synonymous part,
 * coeff[b] = (t_b, omega * t_b).  Templates are uploaded once; per evaluation only the
 * n*K coefficients cross PCIe.  Replaces the serial RecomputeMatrix + MultByFreqs loop
 * (tree.cpp:2944-2969, matrix.cpp:1546-1677) for such models.  Output goes to the partition's
 * device Q buffer which hyphy_hip_evaluate_device() accepts as d_q
 * (hyphy_hip_q_buffer()).
 */
int hyphy_hip_set_q_templates(hyphy_hip_partition *p, int64_t K, const double *templates /* [K*D*D] */);
int hyphy_hip_build_q(hyphy_hip_partition *p, int64_t n, const double *coeffs /* host [n*K] */);
/* New VALUES for the K templates (K unchanged: no reallocation): for hosts whose templates depend on the global
 * parameters of the current evaluation — the HyPhy adapter derives M_k(globals) from K probe branches per
 * ExponentiateMatrices call and sends Q_b = sum_k x_bk M_k as K coefficients per branch.
 * The caller's array is copied before the call returns (pinned staging ring); the upload itself is queued on the partition's
 * stream ahead of the next exponential launch, the host does not wait for it. */
int hyphy_hip_update_q_templates(hyphy_hip_partition *p, int64_t K, const double *templates /* [K*D*D] */);
double *hyphy_hip_q_buffer(hyphy_hip_partition *p); /* device pointer, capacity (L+I-1)*C*D*D doubles */

/*
 * Per-site batched fits.  The FEL family of analyses gives every alignment site its own rate
 * multipliers — res/TemplateBatchFiles/SelectionAnalyses/FEL.bf:593-605 attaches the globals fel.alpha_scaler,
 * fel.beta_scaler_test and fel.beta_scaler_nuisance to the site model, and fel.handle_a_site (FEL.bf:609+) optimises
 * them for ONE site at a time with a single-site likelihood function: per evaluation (L+I-1) calls of
 * _Matrix::Exponentiate (matrix.cpp:5746+) and a one-pattern pruning pass (tree_evaluator.cpp:3556+), sites fanned
 * out over MPI (libv3/tasks/mpi.bf).  This entry point evaluates ALL S patterns of the partition, each under its own
 * multipliers, for n_sets candidate parameter vectors per pattern (e.g. the 12-point start.grid of FEL.bf:617-680, or
 * the simplex of a batched optimiser) in one launch:
 *
 *       Q_{b,s} = sum_k  site_mult[set][s][branch_group[b]][k] * branch_coeffs[b][k] * T_k       (off-diagonal)
 *       site_logl_out[set][s] = log L(pattern s | tree, {Q_{b,s}}_b, root_freqs)     (pattern frequency NOT applied)
 *
 * with the templates T_k of hyphy_hip_set_q_templates (K <= 4; e.g. MG94xREV: T_0 synonymous, T_1 non-synonymous,
 * branch_coeffs[b] = the branch's synonymous / non-synonymous lengths from the global fit, branch_group = 0 tested,
 * 1 nuisance, site_mult[s][g] = (alpha_s, beta_s^g)).  All multipliers, coefficients and off-diagonal template
 * entries must be >= 0.  The transition matrices are never formed: each pruning step applies exp(Q_{b,s}) to the
 * child's conditional vector by uniformisation on the FP64 matrix cores (sitefit.hip).  The result agrees with
 * "exponentiate, then multiply" to rounding (both are approximations of the same exact value; this one has
 * componentwise relative accuracy).  Cost per edge grows linearly with the site's total rate on that branch
 * (sum_k multiplier * coefficient * max_i |T_k[i][i]|); rates above 4096 are refused.  Returns 1 (unsupported) for
 * 4-state partitions, K > 4 and such rates.
 */
int hyphy_hip_site_fits_evaluate(hyphy_hip_partition *p, int64_t n_sets, int64_t n_groups,
                                 const int64_t *branch_group /* [L+I-1] */, const double *branch_coeffs /* [L+I-1][K] */,
                                 const double *site_mult /* [n_sets][S][n_groups][K] */, const double *root_freqs,
                                 double *site_logl_out /* [n_sets][S] */);
/*
 * The same with a branch-site MIXTURE per site (the "explicit form" models of SURVEY §3.4: MEME's two omega classes per
 * site, `res/TemplateBatchFiles/SelectionAnalyses/MEME.bf`; BS-REL, `libv3/models/codon/BS_REL.bf:34-60`, where
 * `tree.cpp:3047-3090` forms P = sum_m w_m exp(Q_m) on every branch): site s evolves on branch b with
 *       P_{b,s} = sum_m site_weights[set][s][m] * exp(Q^(m)_{b,s}),
 *       Q^(m)_{b,s} = sum_k site_mult[set][s][m][branch_group[b]][k] * branch_coeffs[b][k] * T_k.
 * n_mix <= 8; weights >= 0 (normally summing to 1).
 */
int hyphy_hip_site_fits_evaluate_mixture(hyphy_hip_partition *p, int64_t n_sets, int64_t n_groups, int64_t n_mix,
                                         const int64_t *branch_group, const double *branch_coeffs,
                                         const double *site_mult /* [n_sets][S][n_mix][n_groups][K] */,
                                         const double *site_weights /* [n_sets][S][n_mix] */, const double *root_freqs,
                                         double *site_logl_out /* [n_sets][S] */);
double hyphy_hip_site_fits_kernel_ms(const hyphy_hip_partition *p); /* duration of the last site-fit kernel */
/* Synchronous evaluation from the rate matrices staged by the last hyphy_hip_build_q() (n matrices,
 * in the order of q_nodes): template models never move a dense Q across PCIe — only the n*K
 * coefficients go down and one double comes back.  Same semantics as hyphy_hip_evaluate otherwise. */
int hyphy_hip_evaluate_built(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                             const int64_t *q_nodes, int64_t n_q, const double *root_freqs, double *logl_out);

/* hyphy_hip_evaluate_built + the per-pattern outputs of hyphy_hip_evaluate (storageVec / siteCorrections): what the reference's
 * category loop (likefunc.cpp:2851-2990) asks for once per rate class.  On a single-device partition the values and exponents are
 * written in the caller's pattern order into host-mapped memory by a kernel in front of the one that publishes the result record
 * (r05; HYPHY_HIP_SITE_EXPORT=0: two device-to-host copies and a host-side scatter, as hyphy_hip_evaluate did until r04). */
int hyphy_hip_evaluate_built_sites(hyphy_hip_partition *p, int64_t cat, const int64_t *update_nodes, int64_t n_update,
                                   const int64_t *q_nodes, int64_t n_q, const double *root_freqs, double *logl_out,
                                   double *site_lik_out, int64_t *site_scaler_out);

/* Blocks until all work enqueued for the partition has finished. */
int hyphy_hip_synchronize(hyphy_hip_partition *p);

/* The HIP stream (hipStream_t) work is enqueued on for shard 0 — for event timing. */
void *hyphy_hip_stream(hyphy_hip_partition *p);

/* Enqueue all further work of a single-device partition on the caller's stream (e.g. the
 * current PyTorch stream, so that an RCCL all-reduce of d_logl_out is ordered in-stream).
 * Any hipStream_t is accepted, including NULL (the legacy default stream);
 * HYPHY_HIP_OWN_STREAM restores the partition's own stream. */
#define HYPHY_HIP_OWN_STREAM ((void *)(intptr_t)-1)
int hyphy_hip_set_stream(hyphy_hip_partition *p, void *stream);

/* Per-call device timers of the last evaluation, milliseconds (SURVEY §5 tracing row):
 * out[0] = expm kernel(s), out[1] = pruning kernel, out[2] = root/site reduction.
 * out[1] is 0 when the last evaluation carried no kernel-duration stamp (one evaluation in HYPHY_HIP_TIMING_EVERY, default 16,
 * does; hyphy_hip_set_timing_detail(p, 1) stamps every evaluation) — it never reports an earlier evaluation's duration.
 * out[0] and out[2] are measured only while timing detail is on. */
int hyphy_hip_last_timings(hyphy_hip_partition *p, double out[3]);
/* out[0] and out[2] are only stamped while the detail switch is on (two more event records per evaluation; the
 * environment variable HYPHY_HIP_ALL_TIMINGS sets its initial state); out[1] comes from the ring below. */
int hyphy_hip_set_timing_detail(hyphy_hip_partition *p, int on);

/* ---- pinned node states ---------------------------------------------------------------------
 * ComputeBlock's branchIndex / branchValues ("setBranch": src/core/likefunc.cpp:10950-10957; leaf case
 * src/core/tree_evaluator.cpp:163-181, internal case :583-594 and :3624): every evaluation that follows sees
 * node `node` (node code: leaf l -> l, internal i -> L + i, the root included) fixed to states[pattern] in
 * [0, D).  node < 0 or states == NULL removes the pin.  The caller lists the node (and, after removing the pin,
 * lists it again) among update_nodes, as RecoverAncestralSequencesMarginal does with
 * AddBranchToForcedRecomputeList (src/core/likefunc2.cpp:932-1040): the node itself and its ancestors' branches, and for an
 * internal node its children (a node is recomputed when one of its children is listed).
 * A pin left behind: removing the pin changes nothing on the device, so the persisted conditionals and per-pattern values of every
 * class evaluated under it still hold it until an evaluation of that class without the pin recomputes the node that carries it (the
 * pinned internal node, or the pinned leaf's parent): a full pass, or a partial one that lists anything below that node among
 * update_nodes (a partial evaluation recomputes every ancestor of a listed node).  Until then every pass over those values
 * (hyphy_hip_marginal_ancestral, _joint_ancestral, _sample_ancestral, _branch_trials*, _branch_derivatives*, _branch_sensitivities,
 * _branch_gradient*, _nni_scores, _hmm_logl, _hmm_viterbi) returns < 0 and names the class and the node; evaluations are never
 * refused for it.  "The last evaluation of each class" in the descriptions of those passes is therefore never a pinned one.
 * NOT covered: hyphy_hip_branch_cache_build and hyphy_hip_download_partials read the same conditionals and are served as they stand
 * (a download is how a caller looks at a pinned evaluation's conditionals); the caller re-evaluates the path before a cache build. */
int hyphy_hip_set_pinned_states(hyphy_hip_partition *p, int64_t node, const int64_t *states /* [S] */);

/* ---- marginal ancestral reconstruction in one pass --------------------------------------------------------
 * Replaces the I*(D-1) pinned evaluations of RecoverAncestralSequencesMarginal (src/core/likefunc2.cpp:932-1120) with one
 * pre-order ("outside") pass over the resident conditionals: U_root = pi, U_c = P_c^T (U_p * prod of the other children's edge
 * products); the support of internal node n is in_n * U_n / L_s, that of a leaf U_l / L_s.
 *   which = 0: internal nodes (row i = internal index i, node code L + i); 1: leaves (row l, the DOLEAVES form).
 *   weights [C] (NULL when C == 1): the class weights of the last evaluation; classes are mixed by weight (the reference's
 *                   weighted-sum mode, likefunc2.cpp:772-859).
 *   support_out     [rows][S][D] or NULL.  Internal nodes: Pr(state | pattern), all D columns (the reference stores D-1, then
 *                   1 - sum); leaves: L_s(leaf = x) / L_s, unnormalised, as the reference stores it.
 *   map_state_out   [rows][S] or NULL: state of largest support (the first one on ties); map_support_out [rows][S] or NULL.
 * Call after an evaluation of every class; the pass uses the matrices, root frequencies and patterns of the last evaluation
 * of each class (persisted copies are restored first if the last full pass kept them on chip).  Patterns in the caller's order.
 * A class under which a pattern's likelihood is exactly 0, or whose weight is 0, takes no part in that pattern's rows: the support is
 * the mix of the other classes by their shares of the pattern's likelihood, whatever 2^64 exponent the zero class carries.  (In a
 * leaf row this leaves out such a class's L_s(leaf = x) at the states x that the leaf's own data exclude.)  A pattern that is
 * impossible under every class gets NaN in all D entries of each of its rows, map_state -1 and map_support NaN; the call succeeds.
 * Returns < 0 when a pin is active or left behind, a class was never evaluated, or C > 1 without weights.  Leaves no state behind: later
 * evaluations, partial updates and a branch cache built before the call give what they give without it. */
int hyphy_hip_marginal_ancestral(hyphy_hip_partition *p, int64_t which, const double *weights /* [C] or NULL */,
                                 double *support_out, int64_t *map_state_out, double *map_support_out);
/* Host-only: the pre-order program the pass walks.  flat_parents [L+I]: internal index of each node's parent (internal i = node
 * code L + i, the root last with -1), as hyphy_hip_create takes it.
 * out[0] = entries n, out[1] = most children of a node, then n entries of 4 words: a node header (0, internal index, children,
 * 1 for the root) followed by one entry per child (1, child node code, child internal index or -1 for a leaf, position).  Every
 * internal node's header comes after its parent's.  Returns the words written, -(words needed) when cap is too small (out may be
 * NULL), -1 on bad arguments. */
int64_t hyphy_hip_plan_marginal(int64_t L, int64_t I, const int64_t *flat_parents, int64_t *out, int64_t cap);

/* ---- every branch's trial likelihoods from one outside pass -------------------------------------------------
 * Replaces the one evaluation per independent parameter of _LikelihoodFunction::ComputeGradient's finite differences
 * (src/core/likefunc.cpp:7025-7109) for the parameters that are local to one branch: one pre-order pass keeps the outside vector
 * V_c = U_p * prod of the other children's edge products of EVERY branch c, after which the likelihood with the matrix of branch
 * c replaced by M is sum_i V_c[i] (M in_c)[i] per pattern, independent over (trial, pattern).
 *   nodes   [n_trials]            node codes (leaf l -> l, internal i -> L + i, never the root), any order, repeats allowed
 *   q_dense [n_trials][C][D*D]    the branch's matrix in every rate class: rate matrices, or transition matrices when
 *                                 q_is_probability; hyphy_hip_branch_trials_built takes coeffs [n_trials][C][K] over the
 *                                 templates of hyphy_hip_set_q_templates instead (Q = sum_k coeffs_k T_k, as hyphy_hip_build_q)
 *   weights [C] (NULL when C == 1) class weights; the classes of a trial are mixed by weight
 *   logl_out [n_trials]           what hyphy_hip_evaluate (C == 1) / hyphy_hip_evaluate_categories (C > 1) would return with the
 *                                 matrix of branch nodes[t] replaced by trial t in every class and everything else as at the last
 *                                 evaluation of each class; -INFINITY when the trial makes a pattern impossible (for C > 1 too:
 *                                 there is no floor on the logarithm here)
 *   site_lik_out / site_scaler_out [n_trials][S] or NULL: per pattern (l, c) in the caller's pattern order, meaning as in
 *                                 hyphy_hip_evaluate; l = 0 where the trial makes the pattern impossible
 * Call after an evaluation of every class.  Leaves no state behind: the device's matrices and images, the schedules, the tuner's
 * state, the class tables, the branch-cache slots and hyphy_hip_last_expm_kernel are what they were (persisted copies are restored
 * first if the last full pass kept them on chip, as before a marginal reconstruction).  Two identical calls give identical bits.
 * The outside vectors take B x tiles x 16 DP doubles: the pass runs over chunks of tiles that keep them within HYPHY_HIP_TRIALS_MB
 * (default 1024, read at every call, at least one tile); all scratch comes from the pool and is returned before the call returns.
 * Returns < 0 when a pin is active or left behind, a class was never evaluated, C > 1 without weights, a node code is out of range or the root's,
 * or a trial matrix cannot be exponentiated; n_trials == 0 returns 0 and writes nothing. */
int hyphy_hip_branch_trials(hyphy_hip_partition *p, int64_t n_trials, const int64_t *nodes, const double *q_dense,
                            int q_is_probability, const double *weights /* [C] or NULL */, double *logl_out,
                            double *site_lik_out, int64_t *site_scaler_out);
int hyphy_hip_branch_trials_built(hyphy_hip_partition *p, int64_t n_trials, const int64_t *nodes, const double *coeffs,
                                  const double *weights /* [C] or NULL */, double *logl_out, double *site_lik_out,
                                  int64_t *site_scaler_out);

/* ---- every nearest-neighbour interchange's log-likelihood from one outside pass -------------------------------
 * Replaces the one rebuilt tree and full evaluation per swap of the reference's doNNISwap.bf / branchSwappingFunctions.bf.  A move is
 * a pair of node codes (x, y): c = parent(x) must be an internal node other than the root, y a sibling of c (parent(y) ==
 * parent(c) == p, y != c).  The neighbour tree is the one in which x and y exchange parents; every branch keeps its own matrix
 * (P_x travels with x, P_y with y, P_c stays on the edge c -> p).  Only the child sets of c and p change, so with E_k = P_k in_k the
 * edge product of child k and U_n the outside vector at node n (U_root = pi), per pattern and class
 *   R     = U_p * prod E_k   over the children k of p other than c and y
 *   inner = E_y * prod E_k   over the children k of c other than x
 *   l     = sum_i R[i] E_x[i] (P_c inner)[i],      2^64 exponent = exponent(R) + exponent(E_x) + exponent(inner).
 * Nothing assumes binary nodes; on a binary tree every internal non-root branch has two moves.
 *   moves   [n][2]               x, y; any order, repeats allowed
 *   weights [C] (NULL when C == 1) class weights; the classes of a move are mixed by weight as hyphy_hip_branch_trials mixes them
 *   logl_out [n]                 what hyphy_hip_evaluate (C == 1) / hyphy_hip_evaluate_categories (C > 1) would return on the neighbour
 *                                tree with everything else as at the last evaluation of each class; -INFINITY when the move makes a
 *                                pattern of positive frequency impossible, NaN where one has a NaN
 *   site_lik_out / site_scaler_out [n][S] or NULL: per pattern (l, c) in the caller's pattern order, meaning as in hyphy_hip_evaluate
 * Call after an evaluation of every class.  Leaves no state behind, as hyphy_hip_branch_derivatives: the device's matrices and images,
 * the schedules, the tuner's state, the class tables, the branch-cache slots, hyphy_hip_last_expm_kernel and
 * hyphy_hip_last_reduce_form are what they were (persisted copies are restored first if the last full pass kept them on chip).  Two
 * identical calls give identical bits: fixed-order compensated sums per shard, combined over shards as the log-likelihoods are.
 * Chunks of tiles and scratch as hyphy_hip_branch_trials, under the same budget (HYPHY_HIP_TRIALS_MB).  4-state partitions are served.
 * Returns < 0 for a NULL partition, move list or output, a pin active or left behind, a class never evaluated, C > 1 without weights, or a pair that
 * is not a move (hyphy_hip_last_error names it: its index, the pair and the rule it breaks); the partition stays usable.  n == 0
 * returns 0 and writes nothing.
 * Out of scope: subtree pruning and regrafting, trial matrices for the central branch, re-fitting inside the call. */
int hyphy_hip_nni_scores(hyphy_hip_partition *p, int64_t n, const int64_t *moves /* [n][2]: x, y */,
                         const double *weights /* [C] or NULL */, double *logl_out /* [n] */,
                         double *site_lik_out, int64_t *site_scaler_out /* [n][S] or NULL, caller's pattern order */);
/* Host-only: every move of a tree in ascending (c, y, x).  flat_parents [L+I] as hyphy_hip_create takes it.
 * out[0] = moves n, then n pairs x, y.  Returns the words written (1 + 2 n), -(words needed) when cap is too small (out may be NULL),
 * -1 on bad arguments.  (A tree without a move needs one word: ask with cap >= 1 to tell it from bad arguments.) */
int64_t hyphy_hip_plan_nni(int64_t L, int64_t I, const int64_t *flat_parents, int64_t *out, int64_t cap);
/* Host-only: the refusal of hyphy_hip_nni_scores without a partition.  0 when every pair of moves [n][2] is a move of the tree; < 0
 * with hyphy_hip_last_error naming the first that is not, in the words hyphy_hip_nni_scores uses ("move t (x, y): ..."), or on bad
 * arguments.  One function holds the rule: this entry point and hyphy_hip_nni_scores refuse by it, hyphy_hip_plan_nni lists by it. */
int hyphy_hip_check_nni(int64_t L, int64_t I, const int64_t *flat_parents, int64_t n, const int64_t *moves /* [n][2]: x, y */);

/* ---- every branch's first and second log-L derivatives from one outside pass ---------------------------------
 * The exact derivatives an optimiser moves branch lengths with, all branches in one call and without an exponential.  With V the
 * outside vector of branch b and E = P_b in_b its edge product (both exactly what the pass above forms), per pattern and class
 *   l0 = sum_i V[i] E[i]     l1 = sum_i V[i] (G E)[i]     l2 = sum_i V[i] (G (G E))[i]
 * carry one 2^64 exponent, exponent(V) + exponent(in_b).  For C > 1 the three are mixed over the classes by weight with their
 * exponents aligned on the smallest (a class whose three values are exactly 0, a weight of 0 among them, takes no part in the
 * alignment) into L0, L1, L2; for C == 1 they are l0, l1, l2.  Per pattern r1 = L1 / L0 and r2 = L2 / L0 - r1^2, and
 *   d1_out[t] = sum_s f_s r1     d2_out[t] = sum_s f_s r2:
 * the first and second derivative at theta = 0 of log L under P_b(theta) = exp(theta G) P_b, P_b the resident matrix.  With
 * G = Q_b, the scaled rate matrix the branch was last evaluated with, they are the derivatives in a multiplier lambda on the
 * branch's matrix at lambda = 1; in theta = log t_b the first derivative is d1 and the second is d2 + d1.  This is a model
 * parameter's derivative exactly when that parameter scales the whole matrix (a branch length, a class's rate multiplier); for a
 * mixture branch only if the caller accepts G P for it.
 *   nodes    [n]            node codes (leaf l -> l, internal i -> L + i, never the root), any order, repeats allowed
 *   g_dense  [n][C][D*D]    row-major generators, one per class; hyphy_hip_branch_derivatives_built takes coeffs [n][C][K] over the
 *                           templates of hyphy_hip_set_q_templates instead (G = sum_k coeffs_k T_k, diagonal -(row sum), formed as
 *                           hyphy_hip_build_q forms it but into scratch of the call, not into the partition's Q buffer)
 *   weights  [C] (NULL when C == 1)
 *   d1_out, d2_out [n]; skipped_out [n] or NULL; site_d1_out, site_d2_out [n][S] or NULL: r1, r2 in the caller's pattern order
 * A pattern with f_s == 0 takes no part.  A pattern of positive frequency whose mixed L0 is exactly 0 takes no part, is counted in
 * skipped_out[t], and its per-pattern values are NaN.  A NaN in L0, L1 or L2 of a pattern of positive frequency makes both totals
 * NaN.  G == 0 gives exactly 0.0 and 0.0.  4-state partitions are served; there is no "unsupported" return.
 * Call after an evaluation of every class.  Leaves no state behind: the device's matrices and images, the schedules, the tuner's
 * state, the class tables, the branch-cache slots and hyphy_hip_last_expm_kernel are what they were (persisted copies are restored
 * first if the last full pass kept them on chip, as before a marginal reconstruction); hyphy_hip_last_reduce_form is what it was
 * too.  Two identical calls give identical bits: the totals are fixed-order compensated sums per shard, combined over shards as
 * the log-likelihoods are.  Chunks of tiles and scratch as hyphy_hip_branch_trials, under the same budget (HYPHY_HIP_TRIALS_MB).
 * Returns < 0 for a NULL partition or output, a pin active or left behind, a class never evaluated, C > 1 without weights, a node code out of
 * range or the root's, templates not set (_built); n == 0 returns 0 and writes nothing. */
int hyphy_hip_branch_derivatives(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *g_dense,
                                 const double *weights /* [C] or NULL */, double *d1_out, double *d2_out, int64_t *skipped_out,
                                 double *site_d1_out, double *site_d2_out);
int hyphy_hip_branch_derivatives_built(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *coeffs,
                                       const double *weights /* [C] or NULL */, double *d1_out, double *d2_out, int64_t *skipped_out,
                                       double *site_d1_out, double *site_d2_out);

/* ---- the gradient of log L in every matrix entry, rate-matrix entry and template coefficient, one outside pass ----
 * The exact first derivatives of everything that does not merely scale a branch's matrix (omega, kappa, the nucleotide rates, a
 * per-branch (alpha, beta) pair, a mixture component's omega).  With V the outside vector of branch b, in_b the conditional below
 * the branch (the persisted vector of an internal child, the state or ambiguity vector of a leaf) and L_s the pattern's likelihood
 * (mixed over the classes when C > 1), per branch and class c
 *   W_b[i][j] = d log L / d P_b[i][j] = sum_s f_s w_c V_{b,s}[i] in_{b,s}[j] / L_s          (hyphy_hip_branch_sensitivities)
 * whatever P_b was made from (plain, template, mixture or trial matrices).  Where P_b = exp(Q_b), the chain rule is the adjoint of
 * the exponential's Frechet derivative L(A, E) = int_0^1 e^{sA} E e^{(1-s)A} ds:
 *   S_b = d log L / d Q_b = L(Q_b^T, W_b)                                                   (hyphy_hip_branch_gradient)
 * with the entries of Q_b taken as independent, the diagonal included; and for Q_b = sum_k x_bk T_k off the diagonal, diagonal
 * -(row sum),
 *   d log L / d x_bk = sum_{i != j} T_k[i][j] (S_b[i][j] - S_b[i][i])                       (hyphy_hip_branch_gradient_built)
 * from which the host chains any parameter by a K-term dot product per branch.
 *   nodes    [n]            node codes (leaf l -> l, internal i -> L + i, never the root), any order, repeats allowed
 *   weights  [C] (NULL when C == 1)
 *   q_dense  [n][C][D*D]    the scaled rate matrices the branches were last evaluated with, row-major
 *   coeffs   [n][C][K]      their coefficient rows over the templates of hyphy_hip_set_q_templates (the matrices are formed as
 *                           hyphy_hip_build_q forms them, into scratch of the call, not into the partition's Q buffer)
 *   dp_out, dq_out [n][C][D*D] row-major; grad_out [n][C][K]; skipped_out [n] or NULL
 * Class c's block of an output is the derivative in class c's matrix: it already contains the weight w_c and the mixed L_s.  The
 * 2^64 exponents of V, in_b and the mixed likelihood are aligned as hyphy_hip_branch_derivatives aligns them; a class that is exactly
 * zero at a pattern, or has weight 0, contributes nothing there and does not move the alignment.  A pattern with f_s == 0 takes no
 * part.  A pattern of positive frequency whose mixed L_s is exactly 0 takes no part and is counted in skipped_out[t].  A NaN in a
 * value used by a pattern of positive frequency makes the request's whole output block NaN.
 * Mixture branches: hyphy_hip_branch_sensitivities is exact for them; for hyphy_hip_branch_gradient the caller passes component m's
 * rate matrix and multiplies the result by that component's mixture weight.
 * A rate matrix that cannot be handled (a NaN, an infinity-norm of 2^40 or more, an overflow) is a hard error of the two gradient
 * entry points, with hyphy_hip_last_error set.
 * Call after an evaluation of every class.  Leaves no state behind, as hyphy_hip_branch_derivatives: the device's matrices and images,
 * the Q buffer, the schedules, the tuner's state, the class tables, the branch-cache slots, the lazy-persistence flags,
 * hyphy_hip_last_expm_kernel and hyphy_hip_last_reduce_form are what they were.  Two identical calls give identical bits: every
 * (branch, class, segment of 512 patterns) leaves one partial, the partials are summed in ascending segment order and the shards in
 * shard order; the order may depend on the budget, the allowances do not.  (L_s is formed at the requested branch of lowest node code:
 * calls that request different sets of branches may differ in the last bits of a branch they share.)  Chunks of tiles and scratch as hyphy_hip_branch_trials,
 * under the same budget (HYPHY_HIP_TRIALS_MB); with C > 1 the walk runs twice (the mixed L_s must be complete before any class's sum).
 * 4-state partitions are served; there is no "unsupported" return.  Returns < 0 for a NULL partition or output, a pin active or left behind, a class
 * never evaluated, C > 1 without weights, a node code out of range or the root's, templates not set (_built); n == 0 returns 0 and
 * writes nothing.
 * Out of scope: the derivatives in the class weights and in the root frequencies (the host has both from the per-class per-pattern
 * values), an adapter hook, and second derivatives. */
int hyphy_hip_branch_sensitivities(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *weights /* [C] or NULL */,
                                   double *dp_out, int64_t *skipped_out);
int hyphy_hip_branch_gradient(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *q_dense,
                              const double *weights /* [C] or NULL */, double *dq_out, int64_t *skipped_out);
int hyphy_hip_branch_gradient_built(hyphy_hip_partition *p, int64_t n, const int64_t *nodes, const double *coeffs,
                                    const double *weights /* [C] or NULL */, double *grad_out, int64_t *skipped_out);
/* Stand-alone, as hyphy_hip_expm_batch is for the exponential: out[m] = L(q[m]^T, w[m]), n matrices of D x D (2 <= D <= 64), row-major.
 * Scaling X = q^T / 2^p with ||X||_inf <= 1/4, the degree-13 Taylor pair of exp and its derivative (remainder < 2.5e-18 ||w / 2^p||),
 * p squarings L <- P L + L P, P <- P P; no row-sum correction is applied.  A matrix that cannot be handled gives NaN output. */
int hyphy_hip_expm_frechet_adjoint_batch(int64_t D, int64_t n, const double *q_dense, const double *w_dense, double *out);

/* ---- joint maximum-likelihood ancestral reconstruction ------------------------------------------------------
 * Replaces _TheTree::RecoverAncestralSequences (src/core/tree.cpp:4209-4510), the max-product pass behind
 * `ReconstructAncestors (lf)` without MARGINAL: per pattern an upward pass over the nodes in ascending node code
 * (msg[p] = max_c P[p][c] v[c] with the FIRST maximising c as backpointer, strict > starting from 0; a child whose vector is
 * exactly all ones is completely unresolved: backpointer -1, no contribution), the root state as the first argmax of
 * pi[c] m_root[c] (every node -1 when m_root is exactly all ones), and a traceback state[n] = arg_n[state[parent]] (-1 below -1).
 * Factors are multiplied in the reference's order as plain products, rescaled by exact powers of 2^64 after every factor, so the
 * states are those of unbounded-range arithmetic where the reference's single rescaling would underflow.
 *   do_leaves          also reconstruct the leaves (the DOLEAVES form)
 *   class_of_pattern   [S] rate class of each pattern (the reference's catAssignments), caller's pattern order; NULL: class 0
 *                      everywhere (NULL or all zero when C == 1)
 *   states_out         [I (+ L)][S]: rows 0 .. I-1 the internal nodes by internal index (the root last), with do_leaves rows
 *                      I .. I+L-1 the leaves; patterns in the caller's order; values in [0, D) or -1
 * Uses the matrices and leaf data of the last evaluation of each class that is referenced (a class no pattern refers to need not
 * have been evaluated) and the root frequencies currently on the device (one vector for every class, those of the last
 * evaluation).  Reads the matrix images and the leaf table only — no conditionals — so it works whatever form the last pass ran
 * in, and leaves no state behind.  Scratch (about I x 16 x DP x 9 bytes per 16-pattern tile) comes from the pool and is returned
 * before the call returns; the pass runs over chunks of tiles that keep it within HYPHY_HIP_JOINT_MB (default 1024, read at every
 * call, at least one tile).  Two identical calls give identical arrays.
 * Returns < 0 on a NULL partition or output, a pin active or left behind, a class id out of range, or a referenced class never evaluated. */
int hyphy_hip_joint_ancestral(hyphy_hip_partition *p, int do_leaves, const int64_t *class_of_pattern /* [S] or NULL */,
                              int64_t *states_out /* [I (+ L)][S] */);

/* ---- sampled ancestral reconstruction ------------------------------------------------------------------------
 * Replaces _TheTree::SampleAncestorsBySequence (src/core/tree.cpp:4086-4205), the `sample == true` mode of ReconstructAncestors
 * (HBL's SampleAncestors): posterior draws of the states of the internal nodes, root first; leaves are never sampled.
 * A draw is (replicate r, site j, internal node n).  Site j shows pattern s = pattern_of_site[j], which belongs to rate class
 * c = class_of_pattern[s].  With in_n the stored conditional of node n at pattern s in class c:
 *   root (n = I-1): w[i] = pi[i] * in_n[i];  otherwise: w[i] = P_n^(c)[state of the parent][i] * in_n[i]   (one rounded product)
 *   total = w[0] + ... + w[D-1] in ascending i, every addition rounded (no fused multiply-add, no reassociation);  x = u * total
 *   state = the smallest i with cum_i >= x and cum_i > 0, cum_i the same running sum
 * The 2^64 scaler of a stored conditional cancels within a draw and is not applied.
 * Two deviations from the reference: total == 0 or NaN (an impossible pattern) gives state -1, and every descendant of a -1 node
 * is -1 (the reference would index row -1); u == 0 picks the first state of positive weight (the reference's
 * `while (totalSum < randVal)` returns -1 there).
 *   pattern_of_site    [n_sites] pattern of each site, caller's pattern order; NULL: site j = pattern j, n_sites == S
 *   class_of_pattern   [S] rate class of each pattern; NULL: class 0 everywhere
 *   uniforms           [n_rep][I][n_sites], each in [0, 1): the uniform of every draw (an adapter can hand over the reference's own
 *                      Mersenne-Twister stream in the reference's order: node in pre-order, then pattern, then site).  NULL: the
 *                      device generates them with Philox4x32-10, key = (seed low 32 bits, seed high 32 bits), counter =
 *                      (j, n, r, 0), u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53 from the first two output words (multipliers
 *                      0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85): a draw depends on (seed, r, j, n) only,
 *                      not on chunking, shards, device count or the device's pattern order
 *   states_out         [n_rep][I][n_sites] signed bytes (D <= 64), internal index, the root last; -1 or [0, D)
 * Uses the matrices, leaf data and conditionals of the last evaluation of each class that is referenced and the root frequencies of
 * the last evaluation; conditionals a lazy pass did not keep are restored first (as hyphy_hip_download_partials does).  Leaves no
 * state behind: later evaluations, partial updates, branch-cache slots and hyphy_hip_last_expm_kernel are unchanged, and two
 * identical calls give identical arrays.  Scratch (a byte, and with `uniforms` a double, per draw) comes from the pool and is
 * returned before the call returns; the pass runs over chunks (replicates x 16-pattern tiles) that keep it within
 * HYPHY_HIP_SAMPLE_MB (default 1024, read at every call, at least one tile x one replicate).
 * Returns < 0 on a NULL partition or output, a pin active or left behind, a pattern or class index out of range, a referenced class never
 * evaluated, or a supplied uniform outside [0, 1); n_rep == 0 or n_sites == 0 returns 0 and writes nothing. */
int hyphy_hip_sample_ancestral(hyphy_hip_partition *p, int64_t n_rep, int64_t n_sites,
                               const int64_t *pattern_of_site /* [n_sites] or NULL */,
                               const int64_t *class_of_pattern /* [S] or NULL */, uint64_t seed,
                               const double *uniforms /* [n_rep][I][n_sites] or NULL */,
                               int8_t *states_out /* [n_rep][I][n_sites] */);
/* host-only, no device: the uniforms the call above would use with uniforms == NULL, out[n_rep][I][n_sites] */
int hyphy_hip_sample_uniforms(uint64_t seed, int64_t n_rep, int64_t I, int64_t n_sites, double *out);

/* ---- simulation down the tree --------------------------------------------------------------------------------
 * Replaces _LikelihoodFunction::Simulate with BuildLeafProbs / SingleBuildLeafProbs (src/core/likefunc.cpp:12584-13259) and
 * DrawFromDiscrete (src/core/include/function_templates.h:404-413): HBL's SimulateDataSet, the draw behind every parametric
 * bootstrap.  A column is (replicate r, site j); its rate class is c = class_of_site[r][j].  Sites are free: n_sites has nothing
 * to do with the partition's pattern count.  Nodes are visited parent-first; per node n of a column:
 *   row:    the root (node code L+I-1) uses row = pi; any other node uses row = P_n^(c)[state of the parent]
 *   sum:    cum_i = row[0] + ... + row[i] in ascending i, every addition rounded;  total = cum_{D-1};  x = u * total
 *   state:  the smallest i with cum_i >= x and cum_i > 0
 *   total <= 0 or NaN gives -1, and every descendant of a -1 node is -1
 *   with root_states the root takes the given state (validated to lie in [0, D)); the root's uniform is then unused
 * (the device searches the running maximum max(cum_0..cum_i), which gives the same i, also for rows with tiny negative entries).
 * Three deviations from the reference:
 *   1. x = u * total instead of x = u.  Rows sum to 1 within a few ulp; the reference returns index D, past the row, when u
 *      exceeds the rounded sum.
 *   2. u == 0 picks the first state of positive weight.
 *   3. -1 (and -1 below it) replaces indexing with a bad state when a row has no positive total.
 *   class_of_site   [n_rep][n_sites] rate class of each column; NULL: class 0 everywhere.  Category draws and HMM paths are the
 *                   caller's: this call does not draw classes.
 *   root_states     [n_rep][n_sites] state of the root of each column (the reference's spawnValues); NULL: drawn from pi
 *   uniforms        [n_rep][L+I][n_sites] by node code (leaf l -> l, internal i -> L + i), each in [0, 1), validated before anything
 *                   runs.  NULL: Philox4x32-10 as in hyphy_hip_sample_ancestral, key = (seed low 32 bits, seed high 32 bits),
 *                   counter = (j, node code, r, 1), the same 53-bit conversion; the last counter word (sample_ancestral: 0) keeps
 *                   the two streams disjoint under one seed.  A draw depends on (seed, r, j, node) only, not on chunks, slices
 *                   or the sort of the columns by class
 *   with_internal   0: states_out has the L leaf rows; otherwise the I internal rows follow them
 *   states_out      [n_rep][L (+ I)][n_sites] signed bytes by node code; -1 or [0, D)
 * Reads only the matrix images of the last evaluation of each referenced class (a class no column refers to need not have been
 * evaluated) and the root frequencies currently on the device: no conditionals and no leaf data.  So it works behind a plain,
 * lazy, class-compressed, re-rooted, generated, mixture or template pass, with a pin active, and after
 * hyphy_hip_branch_cache_evaluate (the device keeps that trial matrix: it is the one simulated).  Which image: 4 states the
 * row-major matrices; otherwise a leaf's branch from its column-gather image and an internal node's from its A-operand image,
 * the image every writer of matrices leaves for that branch.  Multi-shard partitions use shard 0 (every shard holds every matrix).
 * Leaves no state behind: matrices, images, schedules, tuner state, class tables, branch-cache slots, lazy-persistence flags and
 * hyphy_hip_last_expm_kernel are unchanged, and two identical calls give identical arrays.  Scratch comes from the pool and is
 * returned before the call returns: one table of cumulative rows per referenced class ((L+I) x DP x (DP+1) doubles, about 4 MB at
 * 64 taxa x 61 states), and per column L+I bytes (plus L+I doubles with `uniforms`, and 4 bytes when more than one class is
 * referenced); HYPHY_HIP_SIMULATE_MB (default 1024, read at every call) bounds the per-column part: a chunk is as many whole
 * replicates as fit, otherwise site ranges of one replicate, at least one column.
 * Returns < 0 on a NULL partition or output, a negative count or one above 2^31 - 1, a class id out of range, a referenced class
 * never evaluated, a supplied uniform outside [0, 1) or a root state out of range; n_rep == 0 or n_sites == 0 returns 0 and
 * writes nothing. */
int hyphy_hip_simulate(hyphy_hip_partition *p, int64_t n_rep, int64_t n_sites,
                       const int64_t *class_of_site /* [n_rep][n_sites] or NULL: class 0 */,
                       const int64_t *root_states /* [n_rep][n_sites] or NULL: drawn from pi */, uint64_t seed,
                       const double *uniforms /* [n_rep][L+I][n_sites] by node code, or NULL */, int with_internal,
                       int8_t *states_out /* [n_rep][L (+ I)][n_sites] by node code */);
/* host-only, no device: the uniforms the call above would use with uniforms == NULL, out[n_rep][n_nodes][n_sites] */
int hyphy_hip_simulate_uniforms(uint64_t seed, int64_t n_rep, int64_t n_nodes, int64_t n_sites, double *out);

/* ---- Hidden-Markov rate classes --------------------------------------------------------------------------------------------------------
 * A category variable that carries an HMM model (`--srv HMM` of BUSTED / RELAX, libv3/models/rate_variation.bf:38-74): the likelihood
 * is a chain over the sites in alignment order instead of sum_s f_s log sum_c w_c L_{s,c}.  Replaces, over the per-class per-pattern
 * values that stay on the device behind any evaluation of a class, _LikelihoodFunction::SumUpHiddenMarkov (likefunc2.cpp:1166-1280)
 * and RunViterbi (likefunc2.cpp:1284-1399, what ConstructCategoryMatrix (.., SHORT) returns).
 *   e_i[m] = l[m][s(i)] * 2^(-64 c[m][s(i)]): site i (pattern s(i) of the site list) under class m, from the resident (l, c) of class m
 *   transition [C*C] row-major, T[k][m] = Pr(class m at a site | class k before it); initial [C]
 * Forward sum:   L = initial^T [ prod_{i=0}^{N-2} T diag(e_i) ] e_{N-1}, the product in site order — the reference's recursion, which
 *   reads site i < N-1 in the state AFTER its transition and the last site without one; N = 1: sum_k initial[k] e_0[k].  logl_out = log L.
 * Viterbi path:  z_0 .. z_{N-1} maximising log(initial[z_0] e_0[z_0]) + sum_{i>=1} log(T[z_{i-1}][z_i] e_i[z_i]), exponents entering
 *   as -64 ln2 c for every state.  Among exact ties the lowest state wins each comparison of the blocked recursion: the path is fixed
 *   by the inputs alone.  No path of positive probability, or a NaN among the values used: every entry is -1 and the call succeeds.
 * Deviations from the reference:
 *   - L == 0 answers -INFINITY (the reference: -INFINITY when a step's maximum is 0, myLog's floor when only the last dot product is);
 *   - NaN in a value a listed site uses, in transition or in initial answers NaN (forward) / all -1 (Viterbi);
 *   - RunViterbi ADDS the exponent term for state 0 at its last step (likefunc2.cpp:1364-1368) and in its single-site branch, where
 *     every other state subtracts it; here every state subtracts it;
 *   - the matrix ConstructCategoryMatrix hands out is not this path but the path read through the duplicate map once more (RemapMatrix,
 *     likefunc.cpp:1608-1649: printed[i] = path[pattern_of_site[i]]).  hyphy_hip_hmm_viterbi stands where RunViterbi stands and
 *     returns RunViterbi's path; what the host does with it afterwards is the host's (tests/golden/hmm_*.npz hold both).
 * Patterns no site refers to take no part, whatever their values; pattern frequencies take no part either (the site list is the
 * reference's duplicateMap).  Row sums of `transition` are NOT checked: IsValidTransitionMatrix is the host's business.
 * Arithmetic (hyphy_amd/csrc/hmm.h): rows of the running product carry one integer exponent each and are rescaled by exact powers of
 * two; products of blocks align per output row on that row's largest term.  CONTRACT: a term more than 2^-900 below the largest term
 * of the SAME row of a product is dropped — the limit for chains whose classes do not communicate (block-diagonal transition) yet
 * trade dominance inside one row; rows of different blocks may lie arbitrarily far apart.  The class values of a site enter
 * with their own 2^64 exponents and fall under the same contract — unlike the reference, which puts them on the smallest exponent of
 * the site first (acquireScalerMultiplier) and so zeroes a class 17 exponents above another.
 * The parenthesisation depends on (n_sites, C) alone (hyphy_hip_plan_hmm): two identical calls give identical bits, whatever
 * HYPHY_HIP_TUNE says.  Host and device results are NOT bit-identical (-ffp-contract=fast contracts differently on the two sides).
 * Returns: 0; 1 "use the CPU path" for C == 1 or C > 8; < 0 (hyphy_hip_last_error): a NULL argument, a negative or infinite entry of
 * transition / initial, no site list, a pin active or left behind (hyphy_hip_set_pinned_states), a class that has never been evaluated,
 * or (hmm_logl, hmm_viterbi) a class whose last evaluation ran under other root frequencies than the partition's last one: its
 * per-pattern values still carry the old frequencies (one class evaluated alone under new ones leaves the others behind).  The
 * rule is kept per change, not per value: ANY evaluation under other frequencies than the one before marks every other class, also
 * when it returns to frequencies those classes were combined under; evaluating them again (no matrices needed) clears it.
 * The calls leave no state behind: matrices, images, schedules, tuner state, class tables, branch-cache slots, lazy-persistence flags,
 * the mixed per-pattern values, the cached weights and hyphy_hip_last_expm_kernel are what they were; scratch comes from the pool and
 * is back before the call returns.  A multi-shard partition brings every shard's values to shard 0 by device-to-device copies behind
 * events on the shards' streams and runs there.  hyphy_hip_last_reduce_form answers "hmm sites=<n> segments=<k> levels=<d>" (the host
 * takes no part: nothing is appended for a multi-shard partition). */
/* The site list: pattern of each site in alignment order, caller's pattern order, 1 <= n_sites <= 2^31-1, every index validated;
 * NULL: site j = pattern j, n_sites == S.  Kept on the device with the partition until replaced or the partition is destroyed. */
int hyphy_hip_hmm_set_sites(hyphy_hip_partition *p, int64_t n_sites, const int64_t *pattern_of_site);
/* From the RESIDENT per-class per-pattern values (the last evaluation of each class, by any entry point): no tree work at all — the
 * call a line search on the switching rate makes.  One wait, through the host-mapped result record. */
int hyphy_hip_hmm_logl(hyphy_hip_partition *p, const double *transition /* [C*C] */, const double *initial /* [C] */, double *logl_out);
int hyphy_hip_hmm_viterbi(hyphy_hip_partition *p, const double *transition, const double *initial, int8_t *path_out /* [n_sites] */);
/* hyphy_hip_evaluate_categories / hyphy_hip_evaluate_categories_built with the hidden-Markov combine in place of the weighted mix
 * (which is skipped altogether: no category floor, no mixed values): ONE wait per call. */
int hyphy_hip_evaluate_categories_hmm(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update, const int64_t *q_nodes,
                                      int64_t n_q, const double *q_dense, int q_is_probability, const double *transition,
                                      const double *initial, const double *root_freqs, double *logl_out);
int hyphy_hip_evaluate_categories_built_hmm(hyphy_hip_partition *p, const int64_t *update_nodes, int64_t n_update, const int64_t *q_nodes,
                                            int64_t n_q, const double *transition, const double *initial, const double *root_freqs,
                                            double *logl_out);
/* host-only, no device: the launches of a forward sum.  out[0] = G (sites per segment = blocks per combine, a compile-time constant),
 * out[1] = levels, out[2 .. 2+levels) = work items of each level: (segment, row) pairs — segment j holds the factors
 * [jG, min((j+1)G, n_sites-1)) —, then (block of G blocks, row) pairs while more than G blocks are left, then 1.  Returns the entries
 * needed (at most `cap` are written), -1: bad arguments. */
int64_t hyphy_hip_plan_hmm(int64_t n_sites, int64_t C, int64_t *out, int64_t cap);
/* host-only, no device: the same plan and the same block algebra run serially over values the caller holds (pattern_of_site NULL:
 * site j = pattern j, n_sites == S); what a host without the device entry points computes, at C speed. */
int hyphy_hip_hmm_host(int64_t C, int64_t S, int64_t n_sites, const int64_t *pattern_of_site, const double *lik /* [C][S] */,
                       const int64_t *cnt /* [C][S] */, const double *transition, const double *initial,
                       double *logl_out /* or NULL */, int8_t *path_out /* or NULL */);

/* ---- branch cache ---------------------------------------------------------------------
 * Replaces _TheTree::ComputeBranchCache (src/core/tree_evaluator.cpp:4286-4845) and
 * _TheTree::ComputeLLWithBranchCache (src/core/tree.cpp:3383-3936), driven by the policy code of
 * _LikelihoodFunction::ComputeBlock (src/core/likefunc.cpp:10886-10948, 11125-11258): while the optimiser
 * varies ONE branch length, every evaluation is a single [D x D] x [D x S] contraction.
 *
 * build: after an ordinary hyphy_hip_evaluate* call (conditionals and transition matrices resident, all
 * parameters at the values the line search keeps fixed), prepare the cache for branch `node` (node code:
 * leaf l -> l, internal i -> L + i; not the root).  Works for any model (the tree is re-rooted with
 * transposed transition matrices, no reversibility needed).  Returns 1 for the 4-state path.
 * evaluate: log-likelihood with this branch's matrix replaced by exp(q) (or q itself when
 * q_is_probability); all other parameters as at build time.  The device keeps the new matrix, as the host
 * tree does; the next ordinary evaluation of the class invalidates its cache.  One cache per rate class.
 * site_lik_out / site_scaler_out: per-pattern (l_s, c_s) as hyphy_hip_evaluate returns them. */
int hyphy_hip_branch_cache_build(hyphy_hip_partition *p, int64_t cat, int64_t node);
int hyphy_hip_branch_cache_evaluate(hyphy_hip_partition *p, int64_t cat, int64_t node, const double *q_dense,
                                    int q_is_probability, double *logl_out, double *site_lik_out /* [S] or NULL */,
                                    int64_t *site_scaler_out /* [S] or NULL */);

/* Durations (ms) of the pruning launches of the last `n` evaluations, oldest first, from a ring of HIP
 * event pairs recorded on the partition's stream (shard 0).  Nothing is queried while evaluations run —
 * call this after the timed region.  Returns the number of entries written (<= n, <= 1024).
 * "Evaluations" here are the STAMPED ones: the library stamps one evaluation in k (environment HYPHY_HIP_TIMING_EVERY=k,
 * default 16; the first evaluation of a partition is always stamped) — an event pair costs ~5 us of stream time. */
int64_t hyphy_hip_prune_timings(hyphy_hip_partition *p, double *out_ms, int64_t n);
/* Pruning-kernel launches per evaluation under the current schedule (forest scheduling cuts a full
 * evaluation into levels of subtree fragments, one launch per level; partial updates use one). */
int hyphy_hip_prune_launches(hyphy_hip_partition *p);
/* Name of the pruning kernel this partition's evaluations launch (chosen by shard size and state count;
 * as it appears in a rocprofv3 kernel trace).  Static string.  Class-compressed partitions (subtree repeats, below) run
 * "class_table_team_kernel" in front of it, and answer "trunk_walk_kernel" once their full passes run the trunk as one
 * row-split walk per tile (r06; first passes, partial updates and pinned states keep the pruning kernels). */
const char *hyphy_hip_prune_kernel_name(const hyphy_hip_partition *p);
/* Form of the pruning launch of this partition's last evaluation (the schedule tuner's own passes leave it alone), written down where
 * the launcher picks the instantiation — a launch that could not be served by the instantiation asked for says which one ran:
 *   "prune_wave_kernel NW=<row blocks> park=<0|1|2 parking slots> <occ2|occ3|occ3+pre>; <cut>[; re-rooted]"
 *   "prune_mfma_kernel NW=<row blocks> T=<tiles per workgroup>[ on-chain]; <cut>[; re-rooted]"
 * with <cut> "levels" (level-peeled fragments, and every partial update) or "chain m=<source size limit>".  The instantiation may be
 * followed by " trunk" (class-compressed partitions) or " trace" (HYPHY_HIP_TIMELINE); a trunk walked by trunk_walk_kernel answers
 * "trunk_walk_kernel NW=<row blocks>".  "" before the first evaluation, for 4-state partitions and after an evaluation that had
 * nothing to prune.  Valid until the calling thread's next call of this function. */
const char *hyphy_hip_last_prune_form(const hyphy_hip_partition *p);
/* Which final combine turned the per-pattern values of this partition's last evaluation (hyphy_hip_evaluate and its kin, the category
 * entry points, hyphy_hip_branch_cache_evaluate, hyphy_hip_branch_trials) into log L, written down where the launcher picks it:
 *   "fused n=<partials>"          the last arriver of the pruning launch summed the n per-workgroup partial sums itself
 *   "wave n=<partials>"           wave_reduce_kernel (fewer than 2048 partials, or HYPHY_HIP_REDUCE=wave); for branch trials: one wave
 *                                 per trial over that trial's n partials
 *   "multi_wave<8> n=<partials>"  multi_wave_reduce_kernel<8> (from 2048 partials)
 *   "block n=<partials>"          wg_reduce_kernel (HYPHY_HIP_REDUCE=block)
 *   "site S_pad=<padded patterns>[ floor]"  site_reduce_kernel over the stored per-pattern values (an evaluation that recomputed
 *                                 nothing; " floor": behind the category mix, with the category floor)
 *   "hmm sites=<n> segments=<k> levels=<d>"  the hidden-Markov combine (hyphy_hip_hmm_logl / _viterbi and the two fused entry points):
 *                                 the plan of hyphy_hip_plan_hmm; shard 0 runs it alone, so nothing follows for a multi-shard partition
 * "" before the first evaluation.  A multi-shard partition reports shard 0, followed by "; host x<shards>" (the shard records meet in
 * the host's compensated sum).  Valid until the calling thread's next call of this function. */
const char *hyphy_hip_last_reduce_form(const hyphy_hip_partition *p);
/* Name of the matrix-exponential kernel the calling thread's last launch ran, as it appears in a rocprofv3 kernel trace:
 * "expm_nuc_kernel" (4 states, row-major images), "expm_mfma_kernel<1,1>" / "<2,2>" / "<3,1>" (up to 16 / 32 / 48 states),
 * "expm64_kernel<1>" / "<2>" / "<4>" (49-64 states: 1, 2 or 4 workgroups per matrix, by batch size and compute-unit count) or
 * "expm_mfma_kernel<4,2>" (49-64 states under HYPHY_HIP_EXPM=0).  "" before the first launch and when the exponentials
 * were folded into a 4-state pruning launch.  Static string. */
const char *hyphy_hip_last_expm_kernel(void);

/* What the schedule tuner measured for this partition ("" before it ran): on the first steady-state full pass the
 * library times the (idempotent) pruning pass under each candidate cut of the tree — level-peeled fragments, or chains
 * with source subtrees of at most m internal nodes — and keeps the fastest.  HYPHY_HIP_TUNE=0 disables it. */
/* Host-only planning helpers (no device is touched): decisions hyphy_hip_create takes from the topology / the leaf table alone,
 * exposed for inspection and for tests that run without a GPU.
 *   hyphy_hip_plan_reroot       the path (internal indices, given root first) to the `candidate`-th (0, 1) height-minimising
 *                               node the steady-state passes may be rooted at (re-rooted schedules); returns the
 *                               number of nodes on the path, 0 if there is no such candidate, < 0 on bad arguments.
 *   hyphy_hip_plan_pattern_order  the device-side pattern order (order_out[j] = caller's pattern stored j-th).
 *   hyphy_hip_plan_schedule     compiles the steady-state full-pass schedule of a 61-state partition with `ntiles` 16-pattern
 *                               tiles for `kernel` (0 workgroup per tile, 1 wave per tile, 2 row-split workgroups on chain
 *                               schedules) and cut `chain_m` (> 0: chain schedule with sources of at most chain_m nodes, -1:
 *                               level-peeled fragments, 0: the library's heuristic), optionally re-rooted, and decodes its join
 *                               table the way the kernels do.  info_out[8] = {chain schedule (0/1), programs, schedule entries,
 *                               largest matrix-image slot in the join table, most arrivals a node waits for, records that do not
 *                               decode to the topology (must be 0), re-rooted (0/1), trunk nodes}.  Trees the packed join table
 *                               cannot describe (> 65 535 internal nodes, image slots >= 2^15, > 255 internal children of one node)
 *                               get a schedule without chains. */
int64_t hyphy_hip_plan_reroot(int64_t L, int64_t I, const int64_t *flat_parents, int64_t candidate, int64_t *path_out, int64_t cap);
int hyphy_hip_plan_pattern_order(int64_t D, int64_t L, int64_t S, const int64_t *leaf_codes, int64_t *order_out);
int hyphy_hip_plan_schedule(int64_t L, int64_t I, const int64_t *flat_parents, int64_t kernel, int64_t chain_m, int64_t ntiles,
                            int64_t reroot, int64_t *info_out);

const char *hyphy_hip_schedule_info(const hyphy_hip_partition *p);

/* Subtree repeats — the device form of the reference's `tcc` traversal masks (src/core/tree.cpp:2801-2858 populates them,
 * src/core/likefunc.cpp:10854 passes them on every ComputeBlock, src/core/tree_evaluator.cpp:57-76, 240-256 skip a subtree
 * whose leaf states repeat the previous site's).  At hyphy_hip_create the library groups, per internal node, the patterns
 * whose leaves below the node carry the same states into CLASSES; subtrees with few classes are evaluated once per class
 * (class tables, one MFMA product per 16 classes) and enter the rest of the tree as generalised leaves.  Results are the same
 * with and without; partial updates, rate classes, shards and mixtures all run on the compressed form, pinned states and the
 * branch cache on the plain one.  49-64 states: on where a measurement on the first steady-state pass says it pays; 4 states: built
 * and tested but slower than the plain kernel, so only with HYPHY_HIP_REPEATS=1 / 2 in the environment.
 *   hyphy_hip_set_repeats   on = 0: this partition walks every node at every pattern; 1: back on (default where it pays;
 *                           HYPHY_HIP_REPEATS=0 in the environment turns it off for every partition created afterwards).
 *   hyphy_hip_repeat_stats  first shard: out[0] compression available, [1] class tables, [2] table rows (classes padded to
 *                           tiles of 16 = edge products of the lower phase), [3] / [4] internal nodes / leaves of the trunk,
 *                           [5] edge products of one full pass with repeats on, [6] ... off, [7] in use. */
int hyphy_hip_set_repeats(hyphy_hip_partition *p, int on);
/*   hyphy_hip_plan_repeats  host-only (no device): classes of every internal node over the S patterns as given (classes_out[I]), the
 *                           compressed set for `theta` (compressed_out[I]; theta <= 0: the default 0.35); returns the edge products
 *                           of a full pass with one table per compressed node, < 0 on bad arguments. */
int64_t hyphy_hip_plan_repeats(int64_t L, int64_t I, const int64_t *flat_parents, int64_t S, const int64_t *leaf_codes, double theta,
                               int64_t *classes_out, int64_t *compressed_out);
int hyphy_hip_repeat_stats(const hyphy_hip_partition *p, int64_t out[8]);
/* Host-only (no device): the program trunk_walk_kernel would run for a trunk given as a tree over generalised leaves — node codes
 * 0 .. L - 1 leaves, L + i internal node i (children before parents, the root last), parents[c] = node code of c's parent.
 * out: [nodes, inputs, stack depth, two chains?, first / end node of the one-chain form, of chain 0, of chain 1], then per walked node
 * (internal index, or -1: the chain's end at the root; leaf children; first input; flags 1: push the running product and start from
 * ones, 2: multiply the waiting product back in behind the edge product), then the inputs (leaf codes).  Returns the words written
 * (< 0: -words needed).  Restates nothing of the reference: it is the order in which src/core/tree_evaluator.cpp:3556-4171 visits the
 * nodes above the class tables, cut for one or two workgroups per tile. */
int64_t hyphy_hip_plan_trunk_walk(int64_t L, int64_t I, const int64_t *parents, int64_t *out, int64_t cap);
/* Host-only (no device, reads no environment): everything hyphy_hip_create would put on the device for the class-compressed form of
 * a partition of D states (4: the stack-walk form) and C rate classes — the plan of csrc/repeats_plan.h with its switches as
 * arguments.  leaf_codes: shard after shard, [L][S_pad[k]] as padded for the device (a multiple of 16 patterns unless D = 4; codes
 * < 0: ambiguity codes).  mode: HYPHY_HIP_REPEATS (-1 not given, 1, 2); theta <= 0, rho < 0, min_gain < 0, inline_chains < 0: not
 * given; variant: the pruning kernel the partition starts with (1: wave per tile).
 * Returns 0 when the plan declines (`reason` says why), -1 on bad arguments, -words needed when cap is too small, else the words
 * written.  out: [descriptors ND, view L, view I, shards, walk?]; then lists, each as its length followed by its entries:
 * compressed[I], rep_desc_of[L + I]; per descriptor node, level, path, flags and per path node kids, kid_desc; the view's parents,
 * slot, leaf_has_ambig, leaf_nodes and per view-internal node its children; per shard: rows, per table (U, rows, row0, map0 list),
 * then the words exactly as uploaded: maps, desc (x y z w per entry), ct, lt (x y), the trunk walk's program (x y z w; empty: none). */
int64_t hyphy_hip_plan_repeat_layout(int64_t L, int64_t I, const int64_t *flat_parents, int64_t D, int64_t C, int64_t n_shards,
                                     const int64_t *S_pad, const int64_t *leaf_codes, int64_t mode, double theta, double rho, double min_gain,
                                     int64_t inline_chains, int64_t variant, int64_t *out, int64_t cap, char *reason, int64_t reason_cap);

/* 4 states: schedules as run-time generated straight-line kernels (nucgen.hip; replaces the interpretation of the reference's
 * 4-state loop, src/core/tree_evaluator.cpp:2253-2273, 3556-4171, entry by entry).  A 4-state partition whose full-pass schedule
 * keeps coming back (HYPHY_HIP_NUCGEN_AFTER evaluations, default 8) has it compiled by hiprtc on a background thread and runs it
 * from the evaluation that finds it ready; code objects are shared per process by schedule.  HYPHY_HIP_NUCGEN=0: off (always the
 * interpreter); =2: compile synchronously at the first full pass.  hyphy_hip_prune_kernel_name() answers "nucgen_kernel" once the
 * last launch ran one.
 *   hyphy_hip_plan_nucgen   host-only (needs libhiprtc, no device): the source the library would compile for the steady-state full
 *                           pass of a 4-state partition over this tree (leaf_has_ambig[L] or NULL: leaves that carry ambiguity
 *                           codes; small != 0: the form for shards of at most two workgroups per CU — every matrix in LDS, the
 *                           evaluation's exponentials and the final combine inside the launch); returns its length (src_out, if given, receives at most cap - 1 bytes + NUL), 0 when the
 *                           generator does not cover the schedule, < 0 on bad arguments; *compiled_out = 1 when it compiled for gfx950. */
int64_t hyphy_hip_plan_nucgen(int64_t L, int64_t I, const int64_t *flat_parents, const int64_t *leaf_has_ambig, int64_t small, char *src_out,
                              int64_t cap, int64_t *compiled_out);

/*   hyphy_hip_plan_switches  host-only (no device): the table of the library's environment switches (see the top of this file,
 * docs/switches.md), one line per switch: NAME<TAB>kind<TAB>when<TAB>audience<TAB>default<TAB>value, NAME without the prefix, `when` one of
 * process | create | call, `audience` integrator | diagnostic, `value` what the switch parses to in the environment as it is NOW (a fresh
 * read, also of the switches the library caches per process; sizes in bytes).  Behind the switches, the predicates the library forms from
 * groups of them (kind "predicate").  Returns the bytes needed, the terminating zero included; with out = NULL or cap too small nothing
 * is written and the negated requirement is returned. */
int64_t hyphy_hip_plan_switches(char *out, int64_t cap);

const char *hyphy_hip_last_error(void);
const char *hyphy_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HYPHY_HIP_H */
