"""The call sequences of tests/sequence_cases.py are what tests/test_gpu_sequences.py needs them to be.  CPU only.

1  Shape: every committed seed expands to the step list recorded next to it (EXPANDS), has 14 - 20 steps, at most one refused step in
   five and at least ten held steps.
2  Coverage: over the committed seeds every step kind of the vocabulary occurs, and every pass kind directly after each of
   sequence_cases.PREDECESSORS.
3  Legality: a tracker written here from include/hyphy_hip.h alone (what is evaluated, the pin and what it left behind, what is
   pending, which cache is built) agrees with ``refusal`` at every step: no legal step breaks a rule, and the refused steps are the
   ones the rules refuse.  Move lists pass the host-only ``hip.check_nni``.
4  The model is right: the oracle (oracle/hyphy_oracle.c), given the model's matrices, frequencies and pin at every evaluation-like
   step, stays within scalefree.ORACLE_MAX_REL of ``reference``, with -inf in the same places.
5  Sensitivity: each planted model mistake (sequence_cases.MISTAKES) puts a later held step more than 1000 allowances from the
   correct reference in every sequence where it changes the model.
"""
import numpy as np
import pytest

from tests import scalefree as sf
from tests import sequence_cases as sq

ALL = sq.all_sequences()
DRAWN = [(p, s) for p, s in ALL if s not in sq.FIXED]
IDS = [f"{p}-{s}" for p, s in ALL]
EVALUATIONS = ("full", "lazy_full", "partial", "again", "pi_only", "pinned", "unpinned", "async", "class_partial", "mixture", "catmix",
               "built_full", "built_lazy_full", "built_partial")
VOCABULARY = EVALUATIONS + sq.PASSES + ("collect", "download", "set_repeats", "pin", "unpin", "bc_build", "bc_eval", "hmm_sites", "set_templates",
                                        "update_templates")


def _labels(steps):
    return [sq.label(s) for s in steps]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("profile,seed", DRAWN, ids=[f"{p}-{s}" for p, s in DRAWN])
def test_committed_seeds_expand_as_recorded(profile, seed):
    steps = sq.sequence(profile, seed)
    assert _labels(steps) == list(sq.EXPANDS[(profile, seed)]), (profile, seed, _labels(steps))
    assert sq.draw(seed, profile) is not steps and _labels(sq.draw(seed, profile)) == _labels(steps)      # (seeded: the same again)
    n_refused = sum(s["kind"] == "refused" for s in steps)
    n_held = sum(sq.held(s) for s in steps)
    assert 14 <= len(steps) <= 20 and 5 * n_refused <= len(steps) and n_held >= 10, (profile, seed, len(steps), n_refused, n_held)


def test_profiles_are_the_shapes_they_claim():
    for profile in sq.PROFILES:
        cs = sq.case(profile)
        S = cs["leaf_codes"].shape[1]
        P = np.asarray(cs["P"])
        assert P.min() >= 0.0 and np.allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14), profile
        assert (P.ndim == 4) == (sq.classes(profile) > 1), profile
        env = sq.environment(profile)
        assert env["HYPHY_HIP_TUNE"] == "0" and env["HYPHY_HIP_POISON"] == "1", profile
        if int(cs["D"]) == 4:
            assert S >= 200, (profile, S)                          # several 64-pattern waves
        else:
            assert S % 16 != 0 and S > 32 or profile in ("rerooted", "classes", "classes20"), (profile, S)
    cs, env = sq.case("chunks"), sq.environment("chunks")
    B, I, tiles, DP = len(cs["flat_parents"]) - 1, len(cs["flat_parents"]) - int(cs["L"]), 3, 64
    assert cs["leaf_codes"].shape[1] == 40 and int(cs["D"]) == 61      # three tiles of 16 patterns, 64 padded states
    # (a budget below what the whole shard takes cuts it into at least two chunks of tiles: include/hyphy_hip.h gives the sizes)
    assert float(env["HYPHY_HIP_TRIALS_MB"]) * 2 ** 20 < B * tiles * 16 * DP * 8
    assert float(env["HYPHY_HIP_JOINT_MB"]) * 2 ** 20 < I * 16 * DP * 9 * tiles
    assert float(env["HYPHY_HIP_SAMPLE_MB"]) * 2 ** 20 < 2 * I * 40 * 9


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------

def _predecessor(step):
    k, lab = step["kind"], sq.label(step)
    if k in sq.PASSES:
        return "pass"
    return {"lazy_full": "lazy_full", "partial": "partial", "class_partial": "partial", "built_lazy_full": "lazy_full", "built_partial": "partial", "unpinned": "unpin_reeval", "set_repeats": "repeats_toggle",
            "pi_only": "pi_only", "class_pi_only": "pi_only", "async": "async", "bc_build": "bc_build"}.get(lab)


def test_coverage_of_the_committed_seeds():
    seen, pairs, refused = set(), set(), set()
    for profile, seed in ALL:
        steps = sq.sequence(profile, seed)
        drawn = seed not in sq.FIXED
        if drawn:
            seen.update(_labels(steps))
            refused.update(s["why"] for s in steps if s["kind"] == "refused")
        for before, step in zip(steps, steps[1:]):
            # (the two rate passes run behind templates alone: three drawn sequences cannot hold their sixteen pairs, so for them, and
            #  for them only, the fixed sequence of that profile counts as well)
            if step["kind"] in sq.PASSES and _predecessor(before) and (drawn or step["kind"] in sq.RATE_PASSES):
                pairs.add((_predecessor(before), step["kind"]))
    assert not set(VOCABULARY) - seen, sorted(set(VOCABULARY) - seen)
    want = {(p, k) for p in sq.PREDECESSORS for k in sq.PASSES}
    assert not want - pairs, sorted(want - pairs)
    for profile in sq.PROFILES:                                     # what the issue asks of single profiles
        labels = [l for seed in sq.SEEDS for l in _labels(sq.sequence(profile, seed))]
        if sq.expectations(profile).get("in_use"):
            assert "pinned" in labels and "set_repeats" in labels, (profile, labels)
        if sq.expectations(profile).get("templates"):
            assert "update_templates" in labels and "gradient" in labels and "gradient_built" in labels, (profile, labels)
        if sq.classes(profile) > 1:
            assert "class_partial" in labels and "hmm_logl" in labels, (profile, labels)
    assert refused >= {"pin_active", "unevaluated", "no_weights", "nothing_pending"}, refused
    fixed = set()
    for profile, which in ALL:
        if which in sq.FIXED:
            fixed.update(s["why"] for s in sq.sequence(profile, which) if s["kind"] == "refused")
    assert fixed >= {"pin_left", "pi_stale", "nothing_pending"}, fixed


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------

class _Rules:
    """include/hyphy_hip.h restated for the calls of the vocabulary: what each needs, and what it changes."""

    def __init__(self, cs, C):
        self.fp, self.L, self.C = np.asarray(cs["flat_parents"]), int(cs["L"]), C
        self.B, self.D = len(self.fp) - 1, int(cs["D"])
        self.evaluated, self.pi_of = set(), {}
        self.pin, self.left = None, {c: set() for c in range(C)}
        self.pending, self.cache, self.pi = False, {}, None
        self.templates, self.mixed = False, set()

    def check(self, step):
        """The refusal the header prescribes (None: the call goes through), and assertions on what a legal call may be."""
        k = step["kind"]
        if k == "simulate":
            return None if len(self.evaluated) == self.C else "unevaluated"
        if k in sq.PASSES:
            assert not self.mixed, "a pass over matrices the device exponentiated for a mixture: no reference holds it"
            if k in sq.BUILT_PASSES:
                assert self.templates, "the built forms need templates"
            if self.pin is not None:
                return "pin_active"
            if any(self.left.values()):
                return "pin_left"
            if self.C > 1 and k in sq.NEED_WEIGHTS and step.get("weights") is None:
                return "no_weights"
            if len(self.evaluated) < self.C:
                return "unevaluated"
            if k in sq.HMM_PASSES and any(v is None or not np.array_equal(v, self.pi) for v in self.pi_of.values()):
                return "pi_stale"
        if k == "collect" and not self.pending:
            return "nothing_pending"
        return None

    def advance(self, step):
        k = step["kind"]
        if k == "evaluate":
            e = step["entry"]
            cls = range(self.C) if e in ("categories", "catmix") else [e[1] if isinstance(e, tuple) else max(step.get("cat", 0), 0)]
            if e == "built":
                assert self.templates, "evaluate_built needs templates"
            if self.pi is not None and not np.array_equal(self.pi, step["pi"]):
                self.pi_of = {c: None for c in self.pi_of}          # (any change of the frequencies marks every class)
            up = set(int(u) for u in step["update"])
            above = set()
            for u in up:                                            # a partial evaluation recomputes every ancestor of a listed node
                a = int(self.fp[u])
                while a >= 0:
                    above.add(self.L + a)
                    a = int(self.fp[self.L + a])
            for c in cls:
                for b in (step["q_nodes"] if step["M"] is not None else ()):
                    (self.mixed.add if e in ("mixture", "catmix") else self.mixed.discard)((c, int(b)))
                if c not in self.evaluated:
                    assert len(step["q_nodes"]) == self.B, "the first evaluation of a class supplies every matrix"
                self.evaluated.add(c)
                self.pi_of[c] = step["pi"]
                self.cache.pop(c, None)
                for n in list(self.left[c]):
                    carrier = self.L + int(self.fp[n]) if n < self.L else n
                    if (self.pin is None or self.pin[0] != n) and (len(up) >= self.B or carrier in above):
                        self.left[c].discard(n)
                if self.pin is not None:
                    self.left[c].add(self.pin[0])
            self.pi = step["pi"]
            self.pending = e == "async"
        elif k in sq.PASSES or k in ("collect", "set_repeats", "bc_eval"):
            if k == "bc_eval":
                assert self.cache.get(step["cat"]) == step["node"], "a cache evaluation needs the cache of that branch"
            self.pending = False
        elif k in ("set_templates", "update_templates"):
            assert k == "set_templates" or self.templates, "update_q_templates needs templates"
            self.templates = True
        elif k == "pin":
            assert 0 <= step["node"] < self.B + 1 and np.all((step["states"] >= 0) & (step["states"] < self.D))
            self.pin, self.cache = (step["node"],), {}
        elif k == "unpin":
            self.pin = None
        elif k == "bc_build":
            assert self.D >= 5 and step["cat"] in self.evaluated and self.pin is None and not any(self.left.values())
            self.cache[step["cat"]] = step["node"]
        elif k == "download":
            assert step["cat"] in self.evaluated and self.pin is None and not any(self.left.values()) and not self.pending


@pytest.mark.parametrize("profile,which", ALL, ids=IDS)
def test_every_sequence_is_legal(profile, which):
    from hyphy_amd import hip
    cs, C = sq.case(profile), sq.classes(profile)
    rules, m = _Rules(cs, C), sq.Model(cs, C)
    steps = sq.sequence(profile, which)
    dirty_cache = None
    for i, step in enumerate(steps):
        inner = step["inner"] if step["kind"] == "refused" else step
        why = rules.check(inner)
        assert why == (step["why"] if step["kind"] == "refused" else None), (profile, which, i, sq.describe(step), why)
        assert why == sq.refusal(m, inner), (profile, which, i)
        if inner["kind"] == "nni":
            hip.check_nni(cs["flat_parents"], int(cs["L"]), inner["moves"])
        if step["kind"] != "refused":
            if any(rules.left.values()) and rules.pin is None:         # after removing a pin the node is listed again before anything else
                assert step["kind"] == "evaluate" and step["entry"] != "async", (profile, which, i, sq.describe(step))
            if dirty_cache is not None:                                 # a cache evaluation rewrote the branch's image: the branch comes next
                assert step["kind"] == "evaluate" and dirty_cache in step["q_nodes"], (profile, which, i)
            dirty_cache = step["node"] if step["kind"] == "bc_eval" else None
            rules.advance(step)
        sq.apply(m, step)
    assert rules.pin is None and not any(rules.left.values()) and not rules.pending and m.repeats, (profile, which)
    assert sq.label(steps[-1]).endswith("full")


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------

_worst = {}


def _oracle(cs, P, pi, pin):
    from oracle import oracle
    nodes = np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)
    op = oracle.OraclePartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"])
    op.set_P(nodes, P)
    if pin is not None:
        op.set_branch(pin[0], pin[1])
    try:
        with np.errstate(divide="ignore"):
            return op.site_log_likelihoods(nodes, pi)
    finally:
        op.set_branch(None)                                         # (the oracle's pin is the library's, not the partition's)


@pytest.mark.parametrize("profile,which", ALL, ids=IDS)
def test_oracle_stays_within_the_allowance_at_every_evaluation(profile, which):
    cs, C = sq.case(profile), sq.classes(profile)
    m = sq.Model(cs, C)
    worst, at, n = 0.0, "", 0
    for i, step in enumerate(sq.sequence(profile, which)):
        if step["kind"] != "evaluate" or step["entry"] == "async":
            sq.apply(m, step)
            continue
        ref = sq.expected(m, step)
        e = step["entry"]
        for c in (range(C) if e in sq.BATCH else [e[1] if isinstance(e, tuple) else 0]):
            want = m.prune(cls=c, pinned=m.pin)["site_logl"]
            got = _oracle(cs, m.P[c], m.pi, m.pin)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), (profile, which, i, c)
            fin = np.isfinite(want)
            rel = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0
            n += 1
            if rel > worst:
                worst, at = rel, f"step {i} ({sq.describe(step)}) class {c}"
        if e not in sq.BATCH:
            assert np.array_equal(ref["site"], want)                 # (``reference`` is that prune)
    _worst[(profile, which)] = worst
    print(f"{profile} {which}: oracle against reference over {n} evaluations, largest relative deviation {worst:.3e} at {at} "
          f"(largest so far {max(_worst.values()):.3e})")
    assert worst <= sf.ORACLE_MAX_REL, (profile, which, at, worst)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------

_least = {}


def _same_state(a, b):
    return np.array_equal(a.P, b.P, equal_nan=True) and np.array_equal(a.pi, b.pi) and (a.pin is None) == (b.pin is None)


@pytest.mark.parametrize("mistake", sq.MISTAKES)
def test_a_planted_mistake_shows(mistake):
    occurs = 0
    for profile, which in ALL:
        cs, C = sq.case(profile), sq.classes(profile)
        right, wrong = sq.Model(cs, C), sq.Model(cs, C)
        best, diverged = 0.0, False
        for i, step in enumerate(sq.sequence(profile, which)):
            if step["kind"] == "refused":
                continue
            if diverged and best < 1000.0 and sq.held(step) and step["kind"] not in sq.HMM_PASSES:
                r, w = sq.expected(right, step), sq.expected(wrong, step, mistake)
                best = max(best, sq.distance(step, w, r))
            else:
                sq.apply(right, step)
                sq.apply(wrong, step, mistake)
            if not diverged and not _same_state(right, wrong):
                diverged = True
                if sq.held(step):                                    # the step that went wrong is itself held
                    best = max(best, sq.distance(step, sq.reference(wrong, step), sq.reference(right, step)))
        if diverged:
            occurs += 1
            _least[mistake] = min(_least.get(mistake, np.inf), best)
            assert best >= 1000.0, (mistake, profile, which, best)
    print(f"{mistake}: occurs in {occurs} of {len(ALL)} sequences; the furthest held step behind it is at least {_least.get(mistake, np.nan):.3g} allowances away")
    assert occurs > 0, mistake
