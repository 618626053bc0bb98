// Every environment switch of libhyphy_hip.so, in one table, and the one place in the library that calls getenv.
// Host-only.  A row says what a switch is called, how its value is parsed, what it means when unset, WHEN it is read and
// for whom it is meant; the accessors below the table are what the library's code calls.  docs/switches.md is this table
// as a page, hyphy_hip_plan_switches (include/hyphy_hip.h) is this table with what every switch parses to right now.
//
// Read times:
//   Process   on first use, then cached for the life of the process (the accessor holds the cache): setting the variable
//             later in the same process changes nothing — a test needs a child process
//   Create    while a partition is created and set up (hyphy_hip_create, the set-up of subtree repeats)
//   Call      by every call or launch that consults it: a change takes effect at the next one
// The parsing primitives restate the library's rules as they have always been, malformed values included (atoi / atof:
// "abc" is 0); nothing here validates.
#pragma once
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

namespace hyhip {
namespace sw {

enum Id {
  // for a host integrator
  VERBOSE, POOL_MB, CACHE, TUNE, CUT, REPEATS, NUCGEN, NUCGEN_AFTER, COMBINE, EXCHANGE_TIMEOUT_S, TIMING_EVERY, ALL_TIMINGS,
  TRIALS_MB, JOINT_MB, SAMPLE_MB, SIMULATE_MB,
  // diagnostics: the partition and its evaluation (api.hip, partition.h)
  TRACE, POISON, NOPOISON_, SPIN, FORCE_SHARDS, TILES, SORT_PATTERNS, KERNEL, SLOTS, WAVE_VARIANT, FUSED_REDUCE, TIMELINE, SITE_EXPORT,
  MATERIALIZE_Q, EXPM_PROF, EXPM_MASK, NUCGEN_SMALL,
  // ... the schedule compiler and the tuner (schedule.hip, tuner.hip)
  CHAIN_M, FRAGMENT, REROOT, TINY_FIRST, ABLATE, TUNE_CACHE, TEAM, TRUNK_TEAM,
  // ... the kernels' launchers (expm.hip, prune.hip, nucgen.hip)
  COEF_INLINE, EXPM, EXPM_DEGREE, XCD_PAD, NUC, NUC_LP, NUC_FOLD, REDUCE, NUCGEN_DUMP,
  // ... subtree repeats (repeats.hip)
  REP_THETA, REP_RHO, REP_MIN_GAIN, REP_INLINE, REP_MAX_MB, REP_WAVES, REP_LPT, REP_LEVELS, REP_STATIC, REP_TEAM, REP_NODEPS, REP_TIMELINE,
  TRUNK_KERNEL, TRUNK_WALK, WALK_CHAINS, WALK_TIMELINE,
  kCount
};

enum Kind {
  OnUnlessZero,  // on when unset; off when set and atoi(value) == 0 ("", "abc", "00" and " 0" all turn it off)
  Present,       // on when set to anything, the empty string included
  PresentLevel,  // Present, and atoi(value) as a level (VERBOSE: two parsers, both kept)
  Force01,       // unset: the library decides; set: atoi(value) != 0 forces on, else off
  Int,           // atoi, clamped to [lo, hi]
  Real,          // atof
  Megabytes,     // a size in MiB, by the row's own rule (MbRule)
  Word,          // strcmp against the words the row names; any other value reads as `otherwise`
  Path,          // a file or directory name, used as given
  Prefix         // a family of names: the prefix followed by whatever the site appends
};
enum When { Process, Create, Call };
enum Audience { Integrator, Diagnostic };
enum MbRule { Scratch = 1, Pool, RepMax };  // (in Row::lo)
// groups of diagnostics that switch something else off by being given at all (any value); NOT the same sets
enum Group : unsigned {
  PerPattern = 1,  // forces a per-pattern kernel, instantiation or cut: subtree repeats are not set up (unless REPEATS says so)
  Schedule = 2,    // forces the schedule: the tuner does not run
  WaveForm = 4     // forces the wave kernel's instantiation: the tuner's second stage does not run
};

struct Row {
  Id id;
  const char *name, *env;  // without and with the prefix
  Kind kind;
  When when;
  Audience audience;
  unsigned groups;
  int lo, hi;                        // Int: the clamp; Megabytes: lo = the rule
  const char *dflt;                  // what unset means
  const char *words, *otherwise;     // Word
  const char *where;                 // the file(s) that consult it
  const char *desc;
};

#define SW_(N) N, #N, "HYPHY_HIP_" #N
constexpr Row on0(Id id, const char *n, const char *e, When w, Audience a, const char *where, const char *desc) {
  return {id, n, e, OnUnlessZero, w, a, 0, 0, 0, "on", nullptr, nullptr, where, desc};
}
constexpr Row flag(Id id, const char *n, const char *e, When w, Audience a, unsigned g, const char *where, const char *desc) {
  return {id, n, e, Present, w, a, g, 0, 0, "off", nullptr, nullptr, where, desc};
}
constexpr Row force(Id id, const char *n, const char *e, When w, const char *where, const char *desc) {
  return {id, n, e, Force01, w, Diagnostic, 0, 0, 0, "auto", nullptr, nullptr, where, desc};
}
constexpr Row num(Id id, const char *n, const char *e, When w, Audience a, unsigned g, int lo, int hi, const char *dflt, const char *where,
                  const char *desc) {
  return {id, n, e, Int, w, a, g, lo, hi, dflt, nullptr, nullptr, where, desc};
}
constexpr Row real(Id id, const char *n, const char *e, When w, Audience a, const char *dflt, const char *where, const char *desc) {
  return {id, n, e, Real, w, a, 0, 0, 0, dflt, nullptr, nullptr, where, desc};
}
constexpr Row mb(Id id, const char *n, const char *e, When w, Audience a, MbRule r, const char *dflt, const char *where, const char *desc) {
  return {id, n, e, Megabytes, w, a, 0, (int)r, 0, dflt, nullptr, nullptr, where, desc};
}
constexpr Row word(Id id, const char *n, const char *e, When w, Audience a, unsigned g, const char *words, const char *otherwise,
                   const char *dflt, const char *where, const char *desc) {
  return {id, n, e, Word, w, a, g, 0, 0, dflt, words, otherwise, where, desc};
}
constexpr Row path(Id id, const char *n, const char *e, When w, unsigned g, const char *where, const char *desc) {
  return {id, n, e, Path, w, Diagnostic, g, 0, 0, "-", nullptr, nullptr, where, desc};
}
constexpr int kAny = INT_MAX;  // (no clamp on that side: lo = -kAny)

// One row per switch, in the order of Id.
constexpr Row kRows[] = {
    {SW_(VERBOSE), PresentLevel, Call, Integrator, 0, 0, 0, "off", nullptr, nullptr, "api.hip, tuner.hip, schedule.hip, repeats.hip, nucgen.hip",
     "what was decided and why (schedule tuner, subtree repeats on / off, generated kernels) on stderr.  Two parsers, both kept: set to "
     "anything is on (every site but one); atoi(value) >= 2 also prints the item placement of the lower phase (repeats.hip)"},
    mb(SW_(POOL_MB), Process, Integrator, Pool, "1024", "pool.hip",
       "device / pinned blocks of destroyed partitions kept for the next one of the same shape, MiB per kind (atol; 0 or negative: nothing is kept)"),
    word(SW_(CACHE), Create, Integrator, 0, "always", "lazy", "lazy", "api.hip",
         "always: every pass stores every node's conditionals (default: lazy persistence, see hyphy_hip_download_partials)"),
    on0(SW_(TUNE), Call, Integrator, "api.hip, repeats.hip",
        "0: no run-time schedule measurement (with CUT=levels: bit-identical repeats).  Read by every evaluation, and once more when subtree "
        "repeats are set up (create): without a tuner the trunk starts on the walk"),
    word(SW_(CUT), Call, Integrator, PerPattern | Schedule, "levels", "chains", "tuned", "schedule.hip, api.hip, repeats.hip",
         "levels: fixed multiplication order, no arrival-order joins (level-peeled fragments); any value forces the schedule"),
    num(SW_(REPEATS), Create, Integrator, 0, -kAny, kAny, "measured", "repeats.hip, api.hip",
        "subtree repeats (the reference's `tcc`) 0: never, 1: always, 2: always and past the size rules, instead of decided by measurement.  "
        "Also read per evaluation for its presence alone: given, nothing is measured"),
    num(SW_(NUCGEN), Call, Integrator, 0, -kAny, kAny, "1", "api.hip",
        "4 states: 0 never generate straight-line kernels, 1 compile them in the background, 2 compile synchronously at the first full pass"),
    num(SW_(NUCGEN_AFTER), Call, Integrator, 0, 1, kAny, "8", "api.hip", "... evaluations under one schedule before its kernel is compiled in the background"),
    word(SW_(COMBINE), Call, Integrator, 0, "rccl", "host", "host", "comm.hip",
         "rccl: one process, several devices: sum the shard partials by one RCCL group all-reduce instead of on the host"),
    real(SW_(EXCHANGE_TIMEOUT_S), Call, Integrator, "120", "comm.hip",
         "one process per GPU, host-side exchange: seconds a rank waits for the others (atof: a malformed value is 0)"),
    num(SW_(TIMING_EVERY), Process, Integrator, 0, 1, kAny, "16", "api.hip",
        "one evaluation in n carries the kernel-duration stamp (hyphy_hip_prune_timings, hyphy_hip_last_timings)"),
    flag(SW_(ALL_TIMINGS), Create, Integrator, 0, "partition.h", "initial state of hyphy_hip_set_timing_detail: also stamp expm / reduction (2 more event records)"),
    mb(SW_(TRIALS_MB), Call, Integrator, Scratch, "1024", "trials.hip", "scratch budget of hyphy_hip_branch_trials, MiB (atof; anything not positive: 1024)"),
    mb(SW_(JOINT_MB), Call, Integrator, Scratch, "1024", "joint.hip", "scratch budget of hyphy_hip_joint_ancestral, MiB (as TRIALS_MB)"),
    mb(SW_(SAMPLE_MB), Call, Integrator, Scratch, "1024", "sample.hip", "scratch budget of hyphy_hip_sample_ancestral, MiB (as TRIALS_MB)"),
    mb(SW_(SIMULATE_MB), Call, Integrator, Scratch, "1024", "simulate.hip", "scratch budget of hyphy_hip_simulate, MiB (as TRIALS_MB)"),

    flag(SW_(TRACE), Call, Diagnostic, 0, "partition.h", "host-side lap times of an entry point's stages on stderr"),
    flag(SW_(POISON), Create, Diagnostic, 0, "api.hip, repeats.hip",
         "(tests) fill every fresh allocation with 0xff bytes (NaN / -1), so that anything read before it is written shows up.  Also read by "
         "the call that first allocates the chain schedules' deposits"),
    {SW_(NOPOISON_), Prefix, Create, Diagnostic, 0, 0, 0, "-", nullptr, nullptr, "api.hip", "followed by an allocation's pointer name (s.codes, ...): that block is not poisoned"},
    on0(SW_(SPIN), Process, Diagnostic, "api.hip", "0: a synchronous evaluation waits for its stream instead of spinning on the result record's sequence word"),
    num(SW_(FORCE_SHARDS), Create, Diagnostic, 0, -kAny, kAny, "0", "api.hip", "n > 0: n shards, all on the first device (multi-shard paths on one GPU)"),
    num(SW_(TILES), Create, Diagnostic, PerPattern, -kAny, kAny, "0", "api.hip", "1..4: 16-pattern tiles per workgroup of the row-split kernel, instead of by the grid limit"),
    on0(SW_(SORT_PATTERNS), Create, Diagnostic, "api.hip", "0: the patterns stay in the caller's order on the device"),
    num(SW_(KERNEL), Create, Diagnostic, PerPattern, 0, 2, "by shard size", "api.hip",
        "pruning kernel 0: workgroup per tile, 1: wave per tile, 2: workgroup per tile on chain schedules; the tuner keeps to it"),
    num(SW_(SLOTS), Create, Diagnostic, PerPattern | WaveForm, 2, 4, "by LDS use", "api.hip, tuner.hip", "slot budget of the wave-per-tile kernel"),
    num(SW_(WAVE_VARIANT), Call, Diagnostic, PerPattern | WaveForm, -kAny, kAny, "tuned", "api.hip, tuner.hip", "instantiation of the wave-per-tile kernel (0 / 2: three waves per SIMD)"),
    force(SW_(FUSED_REDUCE), Call, "api.hip", "the final combine inside the pruning launch: 0 / 1 forces either (default: small shards).  The 4-state stage only takes 0"),
    path(SW_(TIMELINE), Call, PerPattern, "api.hip, repeats.hip", "(tracing only) synchronous dump of the pruning launches' time stamps, in the form of the kernel that ran"),
    on0(SW_(SITE_EXPORT), Call, Diagnostic, "api.hip",
        "0: per-pattern results by two device-to-host copies and a host-side scatter instead of the export kernel (the tests run both paths in one process)"),
    flag(SW_(MATERIALIZE_Q), Call, Diagnostic, 0, "api.hip", "hyphy_hip_build_q keeps the stand-alone kernel so that the Q buffer can be read back"),
    flag(SW_(EXPM_PROF), Process, Diagnostic, 0, "api.hip",
         "phase cycles of the exponential kernel on stderr.  Read at two times, both kept: cached per process where the result is collected, per "
         "call where the kernel is launched"),
    on0(SW_(EXPM_MASK), Process, Diagnostic, "api.hip", "0: the exponential kernel writes every matrix image, not only those a branch's consumers read"),
    force(SW_(NUCGEN_SMALL), Call, "api.hip", "the generated 4-state kernel's small-shard form: 0 / 1 forces either (up to 1024 branches)"),

    num(SW_(CHAIN_M), Call, Diagnostic, PerPattern | Schedule, 1, kAny, "tuned", "schedule.hip, api.hip", "chain schedules with source subtrees of at most m internal nodes"),
    num(SW_(FRAGMENT), Call, Diagnostic, PerPattern | Schedule, 1, kAny, "by shard size", "schedule.hip, api.hip", "largest fragment of a level-peeled cut, internal nodes"),
    num(SW_(REROOT), Call, Diagnostic, PerPattern, -kAny, kAny, "tuned", "schedule.hip, tuner.hip",
        "re-rooted schedules 1: always, 0: never, unset: the tuner decides (given at all: its third stage does not run)"),
    num(SW_(TINY_FIRST), Call, Diagnostic, 0, -kAny, kAny, "0", "schedule.hip", "largest source size dispatched in front of the long chains"),
    num(SW_(ABLATE), Call, Diagnostic, PerPattern, -kAny, kAny, "0", "tuner.hip", "PruneArgs::ablate: a phase of the wave kernel left out for an A/B run (results invalid)"),
    on0(SW_(TUNE_CACHE), Process, Diagnostic, "tuner.hip, repeats.hip", "0: every partition measures for itself instead of taking over an earlier one's choice"),
    on0(SW_(TEAM), Process, Diagnostic, "tuner.hip", "0: the tuner does not offer the row-split kernel on chain schedules"),
    on0(SW_(TRUNK_TEAM), Call, Diagnostic, "tuner.hip", "0: the tuner does not offer the trunk under row-split workgroups (the tests run both)"),

    num(SW_(COEF_INLINE), Process, Diagnostic, 0, -kAny, kAny, "1", "expm.hip", "0: the fused rate-matrix construction reads its coefficients from the ring slot, never from the kernel-argument block"),
    num(SW_(EXPM), Process, Diagnostic, 0, -kAny, kAny, "-1", "expm.hip", "49-64 states 0: the r02 kernel; 1 / 2 / 4: that many workgroups per matrix"),
    num(SW_(EXPM_DEGREE), Process, Diagnostic, 0, -kAny, kAny, "adaptive", "expm.hip", "12: fixed Taylor degree 12"),
    on0(SW_(XCD_PAD), Call, Diagnostic, "prune.hip", "0: chain grids with the bare tile count, not padded to a multiple of 8 (the tests run both placements in one process)"),
    num(SW_(NUC), Process, Diagnostic, 0, -kAny, kAny, "-1", "prune.hip", "4 states 0: the r02 kernel, 1 / 2: patterns per thread"),
    force(SW_(NUC_LP), Call, "prune.hip", "4 states: the LDS-schedule instantiation 0 / 1 (default: shards of at most two workgroups per CU)"),
    on0(SW_(NUC_FOLD), Call, Diagnostic, "prune.hip", "0: the 4-state pruning launch never takes the exponentials along"),
    word(SW_(REDUCE), Process, Diagnostic, 0, "block|wave", "auto", "auto", "prune.hip", "final reduction block: the one-block kernel; wave: never the multi-wave one"),
    path(SW_(NUCGEN_DUMP), Call, 0, "nucgen.hip", "directory for the generated 4-state source (and, beside it, the code object)"),

    real(SW_(REP_THETA), Create, Diagnostic, "0.35 (4 states: 0.9)", "repeats.hip", "share of the patterns below which a node's classes are worth a table"),
    real(SW_(REP_RHO), Create, Diagnostic, "0 (from 2048 tiles: 0.5)", "repeats.hip", "a path goes on into the heaviest compressed child while it keeps this share of the node's classes"),
    real(SW_(REP_MIN_GAIN), Create, Diagnostic, "0.15", "repeats.hip", "share of the edge products compression has to save to be set up"),
    force(SW_(REP_INLINE), Create, "repeats.hip", "side chains walked inline 0 / 1 (default: where rho is 0)"),
    mb(SW_(REP_MAX_MB), Create, Diagnostic, RepMax, "a quarter of the free device memory", "repeats.hip", "the caller's bound on the class tables, MiB (atol, negative: 0)"),
    num(SW_(REP_WAVES), Call, Diagnostic, 0, 1, kAny, "by item count", "repeats.hip", "waves of a lower-phase launch (at most one per item)"),
    on0(SW_(REP_LPT), Call, Diagnostic, "repeats.hip", "0: items in descriptor order, not longest-processing-time-first"),
    on0(SW_(REP_LEVELS), Call, Diagnostic, "repeats.hip", "0: one launch with the ticket protocol instead of one launch per dependency level"),
    on0(SW_(REP_STATIC), Call, Diagnostic, "repeats.hip", "0: no item is dealt by position (ticket protocol everywhere; no levels, no row-split walks)"),
    on0(SW_(REP_TEAM), Call, Diagnostic, "repeats.hip", "0: the lower phase never runs as row-split walks"),
    flag(SW_(REP_NODEPS), Call, Diagnostic, 0, "repeats.hip", "nobody waits for a table of the same pass (results invalid)"),
    path(SW_(REP_TIMELINE), Call, 0, "repeats.hip", "synchronous trace of the lower phase, one file per launch"),
    num(SW_(TRUNK_KERNEL), Create, Diagnostic, 0, -kAny, kAny, "-", "repeats.hip", "0 / 2: the trunk under the row-split workgroup kernel (whole trunk per workgroup / on chain schedules)"),
    on0(SW_(TRUNK_WALK), Call, Diagnostic, "repeats.hip",
        "0: never the trunk as one row-split walk per tile (tests and A/B runs switch it).  Read at create too, with another parser, both kept: "
        "atoi(value) == 1 starts the trunk on the walk without asking the tuner, any other value does not"),
    num(SW_(WALK_CHAINS), Call, Diagnostic, 0, -kAny, kAny, "by shard size", "repeats.hip", "2: two workgroups per tile for the walk where its plan has two chains; anything else: one"),
    path(SW_(WALK_TIMELINE), Call, 0, "repeats.hip, api.hip", "synchronous trace of the trunk walk (the lower phase's format)"),
};
#undef SW_
constexpr bool rows_in_order(int i = 0) { return i == kCount ? true : (kRows[i].id == (Id)i && rows_in_order(i + 1)); }
static_assert(sizeof kRows / sizeof kRows[0] == kCount && rows_in_order(), "one row per Id, in the order of Id");

// ---- the parsing primitives: each is ONE lookup --------------------------------------------------------------------------------
inline const char *raw(Id id) { return getenv(kRows[id].env); }
inline bool given(Id id) { return raw(id) != nullptr; }  // Present
inline bool on_unless_zero(Id id) {
  const char *e = raw(id);
  return !(e && atoi(e) == 0);
}
inline int integer(Id id, int unset) {  // Int: the clamped value, `unset` when not given
  const char *e = raw(id);
  return e ? std::max(kRows[id].lo, std::min(kRows[id].hi, atoi(e))) : unset;
}
inline int force01(Id id) {  // Force01: -1 not given, else 0 / 1
  const char *e = raw(id);
  return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}
inline double real_or(Id id, double unset, bool *was_given = nullptr) {
  const char *e = raw(id);
  if (was_given) *was_given = e != nullptr;
  return e ? atof(e) : unset;
}
inline bool word_is(Id id, const char *w) {
  const char *e = raw(id);
  return e && !strcmp(e, w);
}
inline double scratch_bytes(const char *mb) { return (mb && atof(mb) > 0. ? atof(mb) : 1024.) * 1048576.; }  // MbRule::Scratch
inline size_t pool_bytes(const char *e) {                                                                   // MbRule::Pool
  const long mb = e ? atol(e) : 1024;
  return (size_t)(mb < 0 ? 0 : mb) << 20;  // (a negative value means "off", not 2^64 bytes)
}
inline size_t rep_max_bytes(const char *e) { return (size_t)std::max(0L, atol(e)) << 20; }  // MbRule::RepMax (given)

inline bool any_given(unsigned group) {
  for (const Row &r : kRows)
    if ((r.groups & group) && given(r.id)) return true;
  return false;
}

// ---- the accessors: what the library calls.  Process ones hold their cache; the others never cache. -----------------------------
inline bool verbose() { return given(VERBOSE); }
inline int verbose_level() {  // (0 when not given: the one site that asks compares with 2)
  const char *e = raw(VERBOSE);
  return e ? atoi(e) : 0;
}
inline size_t pool_cap_bytes() { static const size_t v = pool_bytes(raw(POOL_MB)); return v; }
inline bool cache_always() { return word_is(CACHE, "always"); }
inline bool tune() { return on_unless_zero(TUNE); }
inline bool cut_levels() { return word_is(CUT, "levels"); }
inline int repeats() {  // -1 not given, 0 never, 2 always and past the size rules, 1 for every other value (always)
  const char *e = raw(REPEATS);
  return !e ? -1 : (atoi(e) == 0 ? 0 : (atoi(e) == 2 ? 2 : 1));
}
inline int nucgen() { return integer(NUCGEN, 1); }
inline int nucgen_after() { return integer(NUCGEN_AFTER, 8); }
inline bool combine_rccl() { return word_is(COMBINE, "rccl"); }
inline double exchange_timeout_s() { return real_or(EXCHANGE_TIMEOUT_S, 120.); }
inline int timing_every() { static const int v = integer(TIMING_EVERY, 16); return v; }
inline bool all_timings() { return given(ALL_TIMINGS); }
inline double scratch_budget(Id id) { return scratch_bytes(raw(id)); }  // TRIALS_MB, JOINT_MB, SAMPLE_MB, SIMULATE_MB: bytes

inline bool trace() { return given(TRACE); }
inline bool poison() { return given(POISON); }
inline bool nopoison(const char *ptr_name) { return getenv((std::string(kRows[NOPOISON_].env) + ptr_name).c_str()) != nullptr; }
inline bool spin() { static const bool v = on_unless_zero(SPIN); return v; }
inline int force_shards() { return integer(FORCE_SHARDS, 0); }
inline int tiles() { return integer(TILES, 0); }
inline bool sort_patterns() { return on_unless_zero(SORT_PATTERNS); }
inline int kernel() { return integer(KERNEL, -1); }  // -1 not given
inline int slots() { return integer(SLOTS, 0); }     // 0 not given
inline int wave_variant(int unset) { return integer(WAVE_VARIANT, unset); }
inline int fused_reduce() { return force01(FUSED_REDUCE); }
inline const char *timeline() { return raw(TIMELINE); }
inline bool site_export() { return on_unless_zero(SITE_EXPORT); }
inline bool materialize_q() { return given(MATERIALIZE_Q); }
inline bool expm_prof() { static const bool v = given(EXPM_PROF); return v; }  // (where the result is collected)
inline bool expm_prof_now() { return given(EXPM_PROF); }                       // (where the kernel is launched)
inline bool expm_mask() { static const bool v = on_unless_zero(EXPM_MASK); return v; }
inline int nucgen_small() { return force01(NUCGEN_SMALL); }

inline int chain_m() { return integer(CHAIN_M, 0); }    // 0 not given
inline int fragment() { return integer(FRAGMENT, 0); }  // 0 not given
inline int reroot() { return integer(REROOT, -1); }     // (-1 not given — and whatever else is neither 0 nor 1)
inline int tiny_first() { return integer(TINY_FIRST, 0); }
inline int ablate() { return integer(ABLATE, 0); }
inline bool tune_cache() { static const bool v = on_unless_zero(TUNE_CACHE); return v; }
inline bool team() { static const bool v = on_unless_zero(TEAM); return v; }
inline bool trunk_team() { return on_unless_zero(TRUNK_TEAM); }

inline int coef_inline() { static const int v = integer(COEF_INLINE, 1); return v; }
inline int expm() { static const int v = integer(EXPM, -1); return v; }
inline bool expm_degree12() { static const bool v = integer(EXPM_DEGREE, 0) == 12; return v; }
inline bool xcd_pad() { return on_unless_zero(XCD_PAD); }
inline int nuc() { static const int v = integer(NUC, -1); return v; }
inline int nuc_lp() { return force01(NUC_LP); }
inline bool nuc_fold() { return on_unless_zero(NUC_FOLD); }
inline int reduce_form() {  // 0 by size, 1 block, 2 wave
  static const int v = [] {
    const char *e = raw(REDUCE);
    return !e ? 0 : (!strcmp(e, "block") ? 1 : (!strcmp(e, "wave") ? 2 : 0));
  }();
  return v;
}
inline const char *nucgen_dump() { return raw(NUCGEN_DUMP); }

inline double rep_theta(double unset, bool *was_given) { return real_or(REP_THETA, unset, was_given); }
inline double rep_rho(double unset) { return real_or(REP_RHO, unset); }
inline double rep_min_gain() { return real_or(REP_MIN_GAIN, 0.15); }
inline int rep_inline() { return force01(REP_INLINE); }
inline bool rep_max_mb(size_t *bytes) {  // true and the bound when given
  const char *e = raw(REP_MAX_MB);
  if (e) *bytes = rep_max_bytes(e);
  return e != nullptr;
}
inline int rep_waves(int n, int unset) {  // (the clamp's upper end is the launch's item count)
  const char *e = raw(REP_WAVES);
  return e ? std::max(1, std::min(n, atoi(e))) : unset;
}
inline bool rep_lpt() { return on_unless_zero(REP_LPT); }
inline bool rep_levels() { return on_unless_zero(REP_LEVELS); }
inline bool rep_static() { return on_unless_zero(REP_STATIC); }
inline bool rep_team() { return on_unless_zero(REP_TEAM); }
inline bool rep_nodeps() { return given(REP_NODEPS); }
inline const char *rep_timeline() { return raw(REP_TIMELINE); }
inline int trunk_kernel() { return integer(TRUNK_KERNEL, -1); }
inline bool trunk_walk() { return on_unless_zero(TRUNK_WALK); }
inline int trunk_walk_at_create() {  // -1 not given, 1 the walk without asking the tuner, 0 any other value
  const char *e = raw(TRUNK_WALK);
  return e ? (atoi(e) == 1 ? 1 : 0) : -1;
}
inline int walk_chains() {  // 0 not given, 2 two chains, 1 any other value
  const char *e = raw(WALK_CHAINS);
  return e ? (atoi(e) == 2 ? 2 : 1) : 0;
}
inline const char *walk_timeline() { return raw(WALK_TIMELINE); }

// the predicates that replace lists of names kept by hand (the Group column of the table)
inline bool per_pattern_forced() { return any_given(PerPattern); }  // a diagnostic that forces a per-pattern kernel, instantiation or cut is set
inline bool schedule_forced() { return any_given(Schedule); }       // the schedule is forced: CHAIN_M, CUT, FRAGMENT
inline bool wave_form_forced() { return any_given(WaveForm); }      // the tuner's own: WAVE_VARIANT, SLOTS (REROOT: given(REROOT))

// "[hyphy_hip] " and the message on stderr under VERBOSE
__attribute__((format(printf, 1, 2))) inline void note(const char *fmt, ...) {
  if (!verbose()) return;
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, (std::string("[hyphy_hip] ") + fmt).c_str(), ap);
  va_end(ap);
}

// ---- hyphy_hip_plan_switches: NAME<TAB>kind<TAB>when<TAB>audience<TAB>default<TAB>value per row; the value is a fresh read through
// the row's primitive (no Process cache).  Behind the rows, the predicates above as rows of kind "predicate".
inline std::string value_now(const Row &r) {
  const char *e = raw(r.id);
  char b[64];
  switch (r.kind) {
    case OnUnlessZero: return on_unless_zero(r.id) ? "on" : "off";
    case Present: return e ? "on" : "off";
    case PresentLevel: return e ? "on," + std::to_string(atoi(e)) : "off";
    case Force01: return e ? (force01(r.id) ? "on" : "off") : r.dflt;
    case Int: return e ? std::to_string(integer(r.id, 0)) : r.dflt;
    case Real: snprintf(b, sizeof b, "%g", e ? atof(e) : 0.); return e ? b : r.dflt;
    case Megabytes:  // bytes
      if (r.lo == RepMax) return e ? std::to_string(rep_max_bytes(e)) : r.dflt;
      if (r.lo == Pool) return std::to_string(pool_bytes(e));
      snprintf(b, sizeof b, "%.0f", scratch_bytes(e));
      return b;
    case Word:
      if (!e) return r.dflt;
      for (const char *w = r.words; w && *w;) {
        const size_t n = strcspn(w, "|");
        if (strlen(e) == n && !strncmp(e, w, n)) return e;
        w += n + (w[n] ? 1 : 0);
      }
      return r.otherwise;
    case Path: return e ? e : r.dflt;
    case Prefix: break;
  }
  return r.dflt;
}
inline std::string plan_text() {
  static const char *const kinds[] = {"on-unless-zero", "present", "present+level", "force01", "int", "real", "megabytes", "word", "path", "prefix"};
  static const char *const whens[] = {"process", "create", "call"};
  std::string t;
  for (const Row &r : kRows)
    t += std::string(r.name) + "\t" + kinds[r.kind] + "\t" + whens[r.when] + "\t" + (r.audience == Integrator ? "integrator" : "diagnostic") + "\t" +
         r.dflt + "\t" + value_now(r) + "\n";
  const struct { const char *name, *when; bool on; } preds[] = {{"per_pattern_forced", "create", per_pattern_forced()},
                                                                {"schedule_forced", "call", schedule_forced()},
                                                                {"wave_form_forced", "call", wave_form_forced()}};
  for (const auto &q : preds) t += std::string(q.name) + "\tpredicate\t" + q.when + "\tdiagnostic\toff\t" + (q.on ? "on" : "off") + "\n";
  return t;
}

}  // namespace sw
}  // namespace hyhip
