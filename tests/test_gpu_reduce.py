"""The last step of every evaluation — per-pattern (l_s, c_s) -> log L = sum f_s log l_s - 64 ln2 sum f_s c_s — through every
route the library has to it, at the partial counts where each route changes its path (tests/reduce_cases.py), with the impossible and
the NaN pattern in the first and the last partial, frequencies that carry sum f_s c_s past 2^31, and frequency-0 patterns.

Every evaluation is held twice (tests/reduce_child.py): (a) per pattern and total against the scale-free reference, (b) the returned
log L against an exact sum of the per-pattern values of the same call, at 8 x 2^-53 of the summed magnitudes (derived in
reduce_cases.exact_sum, not measured).  Every test asserts ``reduce_form()``: a test that ran another combiner, or another n, fails.

Pattern order: wide-state tests run with HYPHY_HIP_SORT_PATTERNS=0 and HYPHY_HIP_TILES=1, so partial k is the caller's patterns
[16 k, 16 k + 16); 4-state patterns are never sorted, partial k is [256 k, 256 k + 256).  4 states give even partial counts only
(the pattern count is padded to 512): 2, 66, 514 and 2050 stand where 1, 65, 513 and 2049 cannot be reached.

Measured worst ratios of (b) per combiner and the hand mutations: profiles/reduce_tests_and_mutations.md."""
import math

import numpy as np
import pytest

from tests import reduce_cases as rc
from tests import reduce_child as ch
from tests import scalefree as sf

pytestmark = pytest.mark.gpu

WIDE = dict(HYPHY_HIP_TILES="1", HYPHY_HIP_SORT_PATTERNS="0", HYPHY_HIP_REPEATS="0")
FOUR = dict(HYPHY_HIP_REPEATS="0")
NONE = np.zeros(0, dtype=np.int64)
# An evaluation that exports its per-pattern values into host-mapped memory never fuses (api.hip: fused_combine_allowed), and the
# comparisons need those values: the fused tests fetch them by copies instead (HYPHY_HIP_SITE_EXPORT=0).
NO_EXPORT = dict(HYPHY_HIP_SITE_EXPORT="0")


def _env(monkeypatch, env):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k in ("HYPHY_HIP_FUSED_REDUCE", "HYPHY_HIP_KERNEL", "HYPHY_HIP_TRIALS_MB", "HYPHY_HIP_FORCE_SHARDS", "HYPHY_HIP_SITE_EXPORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _separate(n):
    return ("multi_wave<8>" if n >= 2048 else "wave") + f" n={n}"


def _ids(x):
    return str(x)


# ---- 1, 2: the separate kernels, by size ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,variant", rc.size_list(5, rc.WIDE5_N), ids=_ids)
def test_wave_and_multi_wave_kernels_five_states(S, variant, monkeypatch):
    _env(monkeypatch, WIDE)
    cs = rc.make(5, S, variant)
    ch.run_passes(cs, _separate(cs["n"]))


@pytest.mark.parametrize("S,variant", rc.size_list(4, rc.FOUR_N), ids=_ids)
def test_wave_and_multi_wave_kernels_four_states(S, variant, monkeypatch):
    """The 4-state kernels leave one partial per workgroup of 256 patterns; the largest case has 524 800 patterns."""
    _env(monkeypatch, dict(FOUR, HYPHY_HIP_FUSED_REDUCE="0", HYPHY_HIP_NUCGEN="0"))
    cs = rc.make(4, S, variant)
    ch.run_passes(cs, _separate(cs["n"]))


# ---- 3: HYPHY_HIP_REDUCE, read once per process: one child per value and size -------------------------------------------------------

@pytest.mark.parametrize("form,n", [("wave", 2049), ("wave", 4097), ("block", 1), ("block", 65), ("block", 513), ("block", 2049)], ids=_ids)
def test_reduce_switch_in_a_fresh_process(form, n, monkeypatch):
    _env(monkeypatch, WIDE)
    rcode, out, rec = ch.run_child(form, 5, n)
    print("\n".join(out.strip().splitlines()[-40:]))
    assert rcode == 0 and rec is not None, out[-2000:]
    names = rec["cases"]
    assert any(x.endswith("minus_inf@last") for x in names) and any(x.endswith("freq0") for x in names), names
    assert all(f"_n{n}_" in x for x in names)
    assert set(rec["worst"]) == {form}, rec


# ---- 4: the fused combine of the row-split kernels (49-64 states) --------------------------------------------------------------------

_ROWSPLIT = {"workgroup": dict(HYPHY_HIP_KERNEL="0"), "team": dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="2")}
_N61 = rc.WIDE61_N + (529,)      # (513 and 529: beyond 2 x the compute units, where the default no longer fuses)


@pytest.mark.parametrize("kernel", sorted(_ROWSPLIT))
@pytest.mark.parametrize("S,variant", rc.size_list(61, _N61), ids=_ids)
def test_fused_combine_of_the_row_split_kernels(S, variant, kernel, monkeypatch):
    """Four passes on one partition: consecutive fused evaluations find the arrival word back at zero (a word left at 1 makes the
    next launch publish early, from n - 1 partials, or never).  The team form fuses on chain schedules, which the first passes may
    not run yet: they may answer ``wave``; the last pass must be fused."""
    _env(monkeypatch, dict(WIDE, HYPHY_HIP_FUSED_REDUCE="1", **NO_EXPORT, **_ROWSPLIT[kernel]))
    cs = rc.make(61, S, variant)
    n = cs["n"]
    ch.run_passes(cs, f"fused n={n}", passes=4, forms_before=[f"wave n={n}"] if kernel == "team" else None, combiner=f"fused {kernel}")


@pytest.mark.parametrize("kernel", sorted(_ROWSPLIT))
def test_default_flips_from_fused_to_separate_at_two_tiles_per_compute_unit(kernel, monkeypatch):
    """HYPHY_HIP_FUSED_REDUCE unset: the row-split kernels fuse up to 2 x CUs tiles and launch the separate kernel beyond.  (The
    kernel is named: without the tuner a partition of this size would run the wave-per-tile kernel, which never fuses.)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _env(monkeypatch, dict(WIDE, **NO_EXPORT, **_ROWSPLIT[kernel]))
    for n, form in ((2 * cus, f"fused n={2 * cus}"), (2 * cus + 1, f"wave n={2 * cus + 1}")):
        for variant in ("plain", "minus_inf@last"):
            cs = rc.make(61, 16 * n, variant)
            ch.run_passes(cs, form, passes=4, forms_before=[f"wave n={n}"], combiner=f"fused {kernel}" if form[0] == "f" else None)


# ---- 5: the fused combine of the class-compressed trunk walk ------------------------------------------------------------------------

@pytest.mark.parametrize("chains", ["1", "2"])
@pytest.mark.parametrize("n,variant", [(2, "plain"), (65, "plain"), (65, "heavy"), (65, "freq0"), (65, "minus_inf@last"), (65, "nan@last"),
                                       (513, "plain"), (513, "minus_inf@last"), (513, "both")], ids=_ids)
def test_fused_combine_of_the_trunk_walk(n, variant, chains, monkeypatch):
    """Class-compressed partitions walk their trunk in one kernel per lazy full pass, which carries the combine (``red_n``).  The
    first passes run the pruning kernels behind the separate combine."""
    _env(monkeypatch, dict(HYPHY_HIP_TILES="1", HYPHY_HIP_SORT_PATTERNS="0", HYPHY_HIP_REPEATS="2", HYPHY_HIP_TRUNK_WALK="1",
                           HYPHY_HIP_WALK_CHAINS=chains, HYPHY_HIP_FUSED_REDUCE="1", **NO_EXPORT))
    cs = rc.make(61, 16 * n, variant)
    ch.run_passes(cs, f"fused n={n}", passes=4, forms_before=[f"wave n={n}", f"fused n={n}"], expect_kernel="trunk_walk_kernel",
                  combiner="fused trunk walk")


# ---- 6, 7: 4 states: the LDS-schedule interpreter and the generated small-shard kernel, fused and not ---------------------------------

_FOUR_FUSED = {"interpreter": dict(HYPHY_HIP_NUCGEN="0", HYPHY_HIP_NUC_LP="1"),
               "generated-small": dict(HYPHY_HIP_NUCGEN="2", HYPHY_HIP_NUCGEN_SMALL="1")}


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("mode", sorted(_FOUR_FUSED))
@pytest.mark.parametrize("S,variant", rc.size_list(4, (2, 66, 514)), ids=_ids)
def test_four_state_fused_combine(S, variant, mode, fused, monkeypatch):
    """n = 2, 66, 514: none a multiple of 4, so the combine's 16-byte flag loads reach past the flags (towards the arrival word)."""
    _env(monkeypatch, dict(FOUR, HYPHY_HIP_FUSED_REDUCE=fused, **NO_EXPORT, **_FOUR_FUSED[mode]))
    cs = rc.make(4, S, variant)
    n = cs["n"]
    form = f"fused n={n}" if fused == "1" else f"wave n={n}"
    ch.run_passes(cs, form, passes=4, forms_before=[f"wave n={n}", f"fused n={n}"],
                  expect_kernel="nucgen_kernel" if mode == "generated-small" else "prune_nuc2_kernel", combiner=f"{form.split()[0]} 4-state {mode}")


# ---- 8: site_reduce_kernel ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "heavy", "minus_inf@last", "nan@last", "minus_inf@first", "both", "both_r", "freq0"])
@pytest.mark.parametrize("S", [sp - d for sp in rc.SITE_S_PAD for d in (0, 9)])
def test_site_reduce_when_nothing_is_recomputed(S, variant, monkeypatch):
    """A full pass, then an evaluation with an empty update list: the stored per-pattern values are reduced by site_reduce_kernel."""
    _env(monkeypatch, WIDE)
    if variant == "heavy" and S < 1000:
        variant = "plain"                                  # (16 patterns cannot carry the count sum into the stated range)
    cs = rc.make(5, S, variant)
    want = rc.expected(cs)
    s_pad = (S + 15) // 16 * 16
    with ch.mk(cs) as part:
        first = ch.full(cs, part)
        got = part.evaluate(NONE, NONE, None, cs["root_freqs"], per_site=True)
        ch.check(f"{cs['name']} nothing to recompute", part, got, cs, want, f"site S_pad={s_pad}", "site")
        assert np.array_equal(got[1], first[1], equal_nan=True) and np.array_equal(got[2], first[2])


def _three_classes(cs, open_class):
    """[3, B, D, D]: the case's block-zero matrices, a second block-zero set, and a third that is block-zero too unless
    ``open_class``: then the cut-off state is reachable under it."""
    D, B = int(cs["D"]), len(cs["flat_parents"]) - 1
    rng = np.random.default_rng(4242)
    P1 = sf._block_zero(sf.near_identity(rng, B, D, 1e-2), D)
    P2 = sf.near_identity(rng, B, D, 1e-4)
    if not open_class:
        P2 = sf._block_zero(P2, D)
    return np.stack([cs["P"], P1, P2])


@pytest.mark.parametrize("S,kind", [(1040, "plain"), (1031, "plain"), (1031, "heavy"), (1031, "freq0")], ids=_ids)
def test_category_floor_and_branch_trials_without_it(S, kind, monkeypatch):
    """evaluate_categories with three classes (include/hyphy_hip.h, at hyphy_hip_evaluate_categories: "The category floor"): a
    pattern impossible under one class only is finite; impossible under all three it contributes exactly -1e6 f and no -inf.
    branch_trials with C = 3 on the same case answers -inf (its header: "there is no floor on the logarithm here")."""
    _env(monkeypatch, WIDE)
    cs = rc.make(5, S, "heavy" if kind == "heavy" else "plain", at=dict(minus_inf=S - 1), zero=("minus_inf",) if kind == "freq0" else ())
    s = cs["special"]["minus_inf"]
    f = cs["pattern_freq"]
    assert (f[s] == 0) == (kind == "freq0")                # (frequency 0: the floor contributes -1e6 x 0, the trials stay finite)
    w = np.array([0.5, 0.3, 0.2])
    n = ch.nodes_of(cs)
    s_pad = (S + 15) // 16 * 16
    with ch.mk(cs, C=3) as part:
        for open_class in (True, False):
            P = _three_classes(cs, open_class)
            ref = sf.prune(5, cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], np.ones(S), P, cs["root_freqs"], weights=w)
            site = ref["site_logl"]
            assert np.isfinite(site[s]) == open_class and np.all(np.isfinite(np.delete(site, s)))
            fin = np.isfinite(site) & (f > 0)
            total = math.fsum((site[fin] * f[fin]).tolist()) + (0.0 if open_class else -1e6 * float(f[s]))
            got = part.evaluate_categories(n, n, P, w, cs["root_freqs"], q_is_probability=True, per_site=True)
            what = f"{cs['name']} three classes, the pattern {'possible under one' if open_class else 'impossible under all'}"
            assert part.reduce_form() == f"site S_pad={s_pad} floor", part.reduce_form()
            assert math.isfinite(got[0]), (what, got[0])
            ch.hold_reference(what, got, site, total, f)
            ch.hold_exact(what, got, f, total, "site floor", floor_at=() if open_class else (s,))
            if not open_class:
                rest = np.array(f)
                rest[s] = 0
                others, _, _ = rc.exact_sum(got[1], got[2], rest)
                assert abs(float(np.longdouble(got[0]) - others) + 1e6 * float(f[s])) <= 1e-6, "the floor is -1e6 f"
        # (the partition now holds the all-block-zero classes) a trial that changes nothing: -inf, not the floor
        ll = part.branch_trials(np.array([0, 3]), np.stack([P[:, 0], P[:, 3]]), weights=w, q_is_probability=True)
        assert part.reduce_form() == f"wave n={s_pad // 16}", part.reduce_form()
        assert np.all(ll == -np.inf) if kind != "freq0" else np.all(np.isfinite(ll)), ll


# ---- 9, 10: branch cache and branch trials --------------------------------------------------------------------------------------------

def _opened(cs):
    """The case with the matrix of leaf branch 0 replaced by one that lets the cut-off state through: the impossible pattern of a
    ``minus_inf@last`` case is possible under it, and impossible again under a trial matrix that is block-zero."""
    D = int(cs["D"])
    rng = np.random.default_rng(99)
    P = cs["P"].copy()
    P[0] = sf.near_identity(rng, 1, D, 1e-3)[0]
    trial_open = sf.near_identity(rng, 1, D, 1e-5)[0]
    trial_shut = sf._block_zero(sf.near_identity(rng, 1, D, 1e-4), D)[0]
    return P, trial_open, trial_shut


def _ref_with(cs, P, M=None):
    P = P.copy()
    if M is not None:
        P[0] = M
    S = cs["leaf_codes"].shape[1]
    site = sf.prune(int(cs["D"]), cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], np.ones(S), P, cs["root_freqs"])["site_logl"]
    f = cs["pattern_freq"]
    live = f > 0
    total = -math.inf if np.isneginf(site[live]).any() else math.fsum((site[live] * f[live]).tolist())
    return site, total


def _special_last(n, kind):
    """A case whose last pattern (last partial) carries the cut-off state at leaf 0: plain, heavy, or with frequency 0."""
    S = 16 * n - 9
    at = dict(minus_inf=S - 1)
    return rc.make(5, S, "heavy" if kind == "heavy" else "plain", at=at, zero=("minus_inf",) if kind == "freq0" else ())


@pytest.mark.parametrize("n,kind", [(65, "plain"), (513, "plain"), (513, "heavy"), (513, "freq0"), (2049, "plain")], ids=_ids)
def test_branch_cache_evaluate(n, kind, monkeypatch):
    """bc_eval_kernel leaves one partial per tile behind launch_wg_reduce(..., ntiles, ...): a trial matrix under which the last
    tile's last pattern is impossible answers -inf (a finite sum when that pattern has frequency 0), an open one a finite sum."""
    _env(monkeypatch, WIDE)
    cs = _special_last(n, kind)
    P, trial_open, trial_shut = _opened(cs)
    form = _separate(n)
    with ch.mk(cs) as part:
        ch.check(f"{cs['name']} full pass, branch 0 open", part, ch.full(cs, part, P), cs, _ref_with(cs, P), form)
        part.branch_cache_build(0)
        for tag, M in (("open", trial_open), ("shut", trial_shut), ("open again", trial_open)):
            got = part.branch_cache_evaluate(0, M, q_is_probability=True, per_site=True)
            want = _ref_with(cs, P, M)
            if tag == "shut":
                assert want[0][-1] == -np.inf and (want[1] == -np.inf) == (kind != "freq0")
            ch.check(f"{cs['name']} branch cache, trial {tag}", part, got, cs, want, form, "branch cache " + form.split()[0])


@pytest.mark.parametrize("n,kind", [(513, "plain"), (513, "heavy"), (513, "freq0"), (2049, "plain")], ids=_ids)
def test_branch_trials_flags_stay_with_their_trial(n, kind, monkeypatch):
    """Three trials on one branch, the middle one making the last tile's last pattern impossible: -inf for that trial alone (the
    per-trial partials lie ``stride`` apart in one buffer); then the same call under a HYPHY_HIP_TRIALS_MB that cuts the tiles into
    at least three chunks: identical bits."""
    _env(monkeypatch, WIDE)
    cs = _special_last(n, kind)
    P, trial_open, trial_shut = _opened(cs)
    mats = np.stack([trial_open, trial_shut, P[0]])
    nodes = np.zeros(3, dtype=np.int64)
    tile_bytes = (len(P)) * 16 * 16 * 8                    # one tile of outside vectors over every branch (5 states pad to 16)
    assert n // max(1, (1 << 20) // tile_bytes) >= 3, "1 MB must cut the tiles into at least three chunks"
    with ch.mk(cs) as part:
        ch.full(cs, part, P)
        whole = part.branch_trials(nodes, mats, q_is_probability=True, per_site=True)
        assert part.reduce_form() == f"wave n={n}", part.reduce_form()
        for t in range(3):
            want = _ref_with(cs, P, mats[t])
            what = f"{cs['name']} trial {t}"
            got = (float(whole[0][t]), whole[1][t], whole[2][t])
            ch.hold_reference(what, got, want[0], want[1], cs["pattern_freq"])
            ch.hold_exact(what, got, cs["pattern_freq"], want[1], "trials wave")
        assert (whole[0][1] == -np.inf) == (kind != "freq0") and np.isfinite(whole[0][0]) and np.isfinite(whole[0][2])
        monkeypatch.setenv("HYPHY_HIP_TRIALS_MB", "1")
        chunked = part.branch_trials(nodes, mats, q_is_probability=True, per_site=True)
        monkeypatch.delenv("HYPHY_HIP_TRIALS_MB")
        for a, b in zip(whole, chunked):
            assert a.tobytes() == b.tobytes()


# ---- 11: shards: the host's combine of the shard records ------------------------------------------------------------------------------

@pytest.mark.parametrize("shard,variant", [(0, "plain"), (0, "heavy")] + [(k, v) for k in (0, 1, 2) for v in ("minus_inf", "nan", "both", "freq0")],
                         ids=_ids)
def test_three_shards_meet_in_the_host_combine(shard, variant, monkeypatch):
    """HYPHY_HIP_FORCE_SHARDS=3 over 1029 patterns: 343 a shard, 21 tiles and 7 patterns, so every shard ends in a partly padded tile;
    the special pattern is the last one of each shard in turn (the NaN one, where there are two, the first of the same shard).
    (b) with 2 x 2^-53 x sum |shard totals| more for the host's compensated sum of the three records."""
    _env(monkeypatch, dict(WIDE, HYPHY_HIP_FORCE_SHARDS="3"))
    S, per = 1029, 343
    last, first = shard * per + per - 1, shard * per
    at = {"plain": {}, "heavy": {}, "minus_inf": dict(minus_inf=last), "nan": dict(nan=last), "both": dict(minus_inf=last, nan=first),
          "freq0": dict(minus_inf=last, nan=first)}[variant]
    cs = rc.make(5, S, "heavy" if variant == "heavy" else "plain", at=at, zero=("minus_inf", "nan") if variant == "freq0" else ())
    want = rc.expected(cs)
    f = cs["pattern_freq"]
    with ch.mk(cs) as part:
        for k in range(2):
            got = ch.full(cs, part)
            what = f"{cs['name']} three shards pass {k}"
            assert part.reduce_form() == "wave n=22; host x3", part.reduce_form()
            ch.hold_reference(what, got, want[0], want[1], f)
            extra = 0.0
            if math.isfinite(want[1]):
                for j in range(3):
                    fj = np.zeros_like(f)
                    fj[j * per:(j + 1) * per] = f[j * per:(j + 1) * per]
                    extra += 2 * rc.U * abs(float(rc.exact_sum(got[1], got[2], fj)[0]))
            ch.hold_exact(what, got, f, want[1], "wave + host x3", extra=extra)


# ---- the other outputs of the same kernels --------------------------------------------------------------------------------------------

def test_async_and_device_outputs_carry_the_flags(monkeypatch):
    """evaluate_async + collect and evaluate_device + fetch_device_scalar at n = 513 with the impossible pattern in the last partial:
    -inf through both; then an open matrix on branch 0: the finite total through both, held by (b)."""
    import torch
    _env(monkeypatch, WIDE)
    cs = _special_last(513, "plain")
    P, _, _ = _opened(cs)
    n = ch.nodes_of(cs)
    d_out = torch.zeros(2, dtype=torch.float64, device="cuda")
    with ch.mk(cs) as part:
        for tag, mats in (("shut", cs["P"]), ("open", P)):
            want = _ref_with(cs, mats)
            assert (want[1] == -math.inf) == (tag == "shut")
            part.evaluate_async(n, n, mats, cs["root_freqs"], q_is_probability=True)
            got = part.collect(per_site=True)
            ch.check(f"{cs['name']} async, branch 0 {tag}", part, got, cs, want, "wave n=513", "wave (async)")
            d_q = torch.tensor(np.ascontiguousarray(mats), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            part.evaluate_device(n, n, d_q.data_ptr(), cs["root_freqs"], d_out.data_ptr(), q_is_probability=True)
            assert part.reduce_form() == "wave n=513", part.reduce_form()
            ll = part.prepare_fetch(d_out.data_ptr())()
            assert ll == got[0] or (math.isnan(ll) and math.isnan(got[0])), (tag, ll, got[0])
