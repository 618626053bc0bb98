"""Call sequences across the library's entry points, held step by step to the references the single-feature tests already use.

A *model* (``Model``) keeps on the host what the library is supposed to hold on the device: the current matrix of every (class,
branch), the current root frequencies, the pin and the pins left behind, whether subtree repeats are on, the pending asynchronous
evaluation, the branch caches, the hidden-Markov site list.  ``apply(model, step)`` advances it, ``refusal(model, step)`` says whether
the header (include/hyphy_hip.h) makes the library refuse the step, ``reference(model, step)`` gives what a legal step must return,
``play(part, step)`` makes the call on a ``hip.HipPartition`` and ``hold_step`` compares the two.  No numerical reference is written
here: every one is ``scalefree.prune`` or the module the entry point's own test uses, at that test's allowance.

  step                                         reference                                                  held by
  evaluate (full, partial, nothing dirty,      scalefree.prune on the model (the pin included)            hold._hold
    pi only, one class, all classes, async
    + collect)
  download                                     prune(conditionals=True)                                   hold.hold_download
  bc_build + bc_eval                           prune with the branch's matrix replaced                    hold._hold
  marginal (internal, leaves)                  prune(posteriors=True)                                     marginal_cases.hold_support, hold_map
  nni                                          nni_cases.reference                                        hold._hold
  trials                                       prune with the branch's matrix replaced in every class     hold._hold
  derivatives                                  deriv_cases.outside / values                               deriv_cases.miss
  sensitivities                                grad_cases.outside / sensitivities                         grad_cases.miss_w
  joint                                        joint_ref.joint_ref                                        equality
  sample                                       sample_ref.sample_ref on the device's own download,        equality; the download: hold_download
                                               the download held to the model
  hmm_logl, hmm_viterbi                        hmm_ref.forward_mp / viterbi_mp / path_score on the        HMM_ALLOWANCE below
                                               model's per-class values
  simulate                                     simulate_ref.simulate_ref                                  equality
  mixture (evaluate_mixture), catmix           the construction of mixture_cases.enclosure /              mixture_cases.hold_enclosure
    (evaluate_categories_mixture), and every   catmix_cases.enclosure: prune at both ends of the
    evaluation while such a branch is resident interval mixture_cases.matrices gives each matrix
  set_templates, update_templates, built       template_cases' replay: expm_ref.reference of              hold._hold
    (build_q + evaluate_built)                 template_cases.rate_matrix(T, row), kept per branch
  trials_built, derivatives_built              the dense forms' references on those matrices              as trials / derivatives
  gradient, gradient_built                     grad_cases.gradient (S, the chain to the coefficients),    allow_S, allow_grad, and the device's own
                                               on the rate matrix each branch was built from              d1 of the same rows (test_gpu_gradient.py)

Matrices are row-stochastic (``q_is_probability``) wherever the entry point takes them: the exponential adds no allowance of its own.
Rate matrices go in where the entry point needs them: mixtures (named matrices of tests/expm_ref.py; those branches carry
mixture_cases' allowance until they are replaced, and no pass is drawn while one is resident) and the profile ``templates``, where
every matrix is built on the device from a coefficient row; that profile leaves out the passes that compare states exactly or hold
the conditionals themselves to a relative bar (NOT_BEHIND_EXPM), as their own tests do behind the device's exponential:
``derivatives_built`` as a step of its own is one of them (deriv_cases' allowance is GPU_RTOL relative to the magnitudes A1, A2 formed
from the conditionals, and tests/test_gpu_branch_derivatives.py puts the device's own exponentials into the reference behind a template
pass; a sequence's model has expm_ref's), so behind templates it is held the way tests/test_gpu_gradient.py holds it there: every
``gradient_built`` step also calls ``branch_derivatives_built`` with the same rows and holds sum_k x_k grad_k to its d1 at
deriv_cases' allow_d1 plus the chained allowance.  The other profiles hold ``derivatives_built`` against deriv_cases directly.  A change
step swaps a branch between ``scalefree.ordinary`` and ``scalefree.near_identity`` at 1e-10 .. 1e-30 (behind templates: between a
row and one a thousand times smaller), so that a stale matrix or conditional is far away.  Every pass is called twice and must
return identical bytes.

HMM_ALLOWANCE.  The single-feature test holds ``hmm_logl`` on the device's own per-class values at ``hmm_ref.bar``; a sequence has no
call that reads those values without changing state, so the reference runs on the model's ``class_site_logl`` instead.  The device's
values may deviate from those by what ``hold._hold`` allows per pattern, d_s = GPU_RTOL |log l_s| + 1e-9 (largest over the classes);
the forward sum is a sum of products with one emission per site in every term and the Viterbi score a maximum of such products, so
both move by at most sum over the listed sites of d_s in the logarithm.  The allowance is ``hmm_ref.bar`` plus that sum.

The oracle (oracle/hyphy_oracle.c) played over every evaluation-like step of every committed sequence stays within
scalefree.ORACLE_MAX_REL = 3.1e-15 of ``reference`` (tests/test_sequence_cases_cpu.py prints the largest deviation: 2.347e-15, the
first full pass of profile ``shards``; at most 5.7e-16 elsewhere), so ``scalefree.GPU_RTOL`` holds on these sequences as it stands.

Not in the vocabulary: ``evaluate_mixture_built`` / ``evaluate_categories_mixture_built`` (mixture_cases builds their components from
templates that ARE named matrices; the profiles' templates are not).

``python -m tests.sequence_cases PROFILE SEED`` (or a fixed sequence's name in place of SEED) prints the steps.
"""
import functools
import sys

import numpy as np

from tests import branchcache_cases as bc
from tests import common
from tests import compressed_cases as cc
from tests import deriv_cases as dc
from tests import grad_cases as gc
from tests import hold
from tests import marginal_cases as mc
from tests import nni_cases as nc
from tests import scalefree as sf

NONE = np.zeros(0, dtype=np.int64)
TINY_EPS = (1e-10, 1e-20, 1e-30)
PASSES = ("marginal", "marginal_leaves", "nni", "trials", "derivatives", "sensitivities", "joint", "sample", "hmm_logl", "hmm_viterbi",
          "trials_built", "derivatives_built", "gradient", "gradient_built", "simulate")
HMM_PASSES = ("hmm_logl", "hmm_viterbi")
BUILT_PASSES = ("trials_built", "derivatives_built", "gradient_built")       # need templates (hyphy_hip_set_q_templates)
RATE_PASSES = ("gradient", "gradient_built")                                 # need resident matrices that are exp of known rate matrices
EXACT_PASSES = ("joint", "sample", "simulate")                               # equality of states: not behind the device's exponential
# what the profile whose matrices go through the device's exponential does not hold: the exact passes, and the passes whose allowance
# is a relative one on the conditionals themselves (their own tests take the device's exponentials into the reference there)
NOT_BEHIND_EXPM = EXACT_PASSES + ("derivatives", "sensitivities", "derivatives_built")
NEED_WEIGHTS = ("marginal", "marginal_leaves", "nni", "trials", "derivatives", "sensitivities", "trials_built", "derivatives_built",
                "gradient", "gradient_built")
BATCH = ("categories", "catmix")            # the entries that evaluate every class in one call
MIXTURE_D = (4, 20, 33, 61)                 # state counts at which mixture_cases draws its named components
PREDECESSORS = ("lazy_full", "partial", "pass", "unpin_reeval", "repeats_toggle", "pi_only", "async", "bc_build")
SHORT = ("partial", "pass", "repeats_toggle", "pi_only", "async")      # the predecessors that are one step
REFUSALS = ("pin_active", "pin_left", "unevaluated", "no_weights", "nothing_pending", "pi_stale")
MISTAKES = ("stale_partial", "slot_table", "pin_survives", "old_pi", "compressed_view", "async_dropped")


# ---- cases and profiles -----------------------------------------------------------------------------------------------------------

def _bal(name, D, S, seed):
    """branchcache_cases' patterns and matrices on the 16-taxon binary tree with ``S`` patterns (an even seed: no impossible pattern)."""
    return bc._make(name, "bal2x4", D, seed, tree=sf.balanced_tree(2, 4), S=S)


def _compressible(D, seed):
    """common.compressible_case without its rates; near-identity matrices at compressed_cases' eps per branch instead."""
    fx = dict(common.compressible_case(D, seed), name=f"seq_compressible_D{D}", seed=seed, eps=1e-12)
    del fx["Q"]
    rng = np.random.default_rng([seed, 2])
    B = len(fx["flat_parents"]) - 1
    fx["P"] = sf.near_identity(rng, B, D, rng.choice(cc.EPS_LIST, size=B))
    return fx


def _built(D, K):
    cs, T, x, _ = gc.built_case(D, K)
    return dict(cs, T=T, x=x, eps=1e-12)


def _one_class(cs):
    return dict(cs, P=cs["P"][0], name=cs["name"] + "_class0")


_ENV0 = dict(HYPHY_HIP_TUNE="0", HYPHY_HIP_POISON="1")
PROFILES = {
    # name: (case, classes, environment beside TUNE=0 POISON=1, what the device test asserts beside the steps)
    "wave_lazy": (lambda: _bal("seq_bal2x4_D61", 61, 40, 7502), 1, dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REPEATS="0"), {}),
    "workgroup": (lambda: _bal("seq_bal2x4_D17", 17, 40, 7504), 1, dict(HYPHY_HIP_KERNEL="0", HYPHY_HIP_REPEATS="0"), {}),
    "rerooted": (lambda: bc.cases_by_name()["ladder40_D33"], 1,
                 dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REROOT="1", HYPHY_HIP_CHAIN_M="2", HYPHY_HIP_REPEATS="0"), dict(rerooted=True)),
    "compressed": (lambda: _compressible(61, 7), 1, dict(HYPHY_HIP_REPEATS="1", HYPHY_HIP_KERNEL="1"), dict(in_use=True)),
    "compressed_nuc": (lambda: _compressible(4, cc.SEEDS[4]), 1, dict(HYPHY_HIP_REPEATS="1"), {}),
    "classes": (lambda: bc.class_cases()[1], 3, {}, {}),
    "classes20": (lambda: bc.class_cases()[0], 3, {}, {}),
    "shards": (lambda: _one_class(bc.chunked_class_case(33, 70)), 1, dict(HYPHY_HIP_FORCE_SHARDS="2"), {}),
    "nuc": (lambda: _bal("seq_bal2x4_D4", 4, 200, 7506), 1, dict(HYPHY_HIP_NUCGEN="0"), {}),
    "nucgen": (lambda: _bal("seq_bal2x4_D4", 4, 200, 7506), 1, dict(HYPHY_HIP_NUCGEN="1"), {}),
    # the outside vectors of the case take 30 x 3 x 16 x 64 x 8 = 737 280 bytes, the joint pass 15 x 16 x 64 x 9 = 138 240 per tile, a
    # sample of 2 x 15 x 40 draws 10 800 with supplied uniforms: every pass runs in at least two chunks of tiles
    "chunks": (lambda: _bal("seq_bal2x4_D61", 61, 40, 7502), 1,
               dict(HYPHY_HIP_KERNEL="1", HYPHY_HIP_REPEATS="0", HYPHY_HIP_TRIALS_MB="0.3", HYPHY_HIP_JOINT_MB="0.2", HYPHY_HIP_SAMPLE_MB="0.004"), {}),
    # every matrix is exp of a rate matrix built on the device from coefficient rows over two templates (grad_cases.built_case)
    "templates": (lambda: _built(20, 2), 1, {}, dict(templates=True)),
}
SEEDS = (1, 2, 3)
WEIGHTS = np.array([0.5, 0.3, 0.2])
WEIGHTS_ZERO = np.array([0.6, 0.0, 0.4])


@functools.lru_cache(maxsize=None)
def case(profile):
    cs = dict(PROFILES[profile][0]())
    cs.setdefault("eps", 1e-12)
    cs.setdefault("seed", 7500)
    return cs


def classes(profile):
    return PROFILES[profile][1]


def environment(profile):
    return dict(_ENV0, **PROFILES[profile][2])


def expectations(profile):
    return PROFILES[profile][3]


# ---- the model --------------------------------------------------------------------------------------------------------------------

_models = [0]


class Model:
    def __init__(self, base, C=1):
        self.base, self.C = base, int(C)
        _models[0] += 1
        self.uid = _models[0]                                        # (the reference modules cache by case name: see ``cs``)
        self.D, self.L = int(base["D"]), int(base["L"])
        self.fp = np.asarray(base["flat_parents"], dtype=np.int64)
        self.B, self.S = len(self.fp) - 1, int(np.asarray(base["leaf_codes"]).shape[1])
        self.P = np.full((self.C, self.B, self.D, self.D), np.nan)
        self.PL = self.P.astype(np.longdouble)                       # the same before rounding (a mixture is summed in longdouble)
        self.allow = np.zeros((self.C, self.B))                      # entrywise allowance of a matrix the device exponentiated (mixtures)
        self.Q = np.full((self.C, self.B, self.D, self.D), np.nan)   # the rate matrix a branch's matrix is the exponential of (NaN: none)
        self.templated = "T" in base                                 # every matrix is built on the device from coefficient rows
        self.T = None                                                # the template set on the device
        self.rows = None                                             # [C, B, K] the row each branch was last built from under T (NaN: none)
        self.kind = np.zeros((self.C, self.B), dtype=np.int64)       # 0: ordinary, 1: near-identity (what a change step swaps)
        self.evaluated = [False] * self.C
        self.pi = None
        self.pin = None                                              # (node, states)
        self.pin_left = [set() for _ in range(self.C)]               # nodes whose pin the class's stored values still hold
        self.repeats = True
        self.pi_at = [None] * self.C                                 # the frequencies of each class's own last evaluation
        self.pending = None                                          # the class of an uncollected evaluate_async
        self.last_async = 0
        self.batch = None                                            # whether the last evaluation was a class batch
        self.bc = {}                                                 # class -> branch with a cache
        self.bc_dirty = None                                         # (class, branch) whose image a bc_eval rewrote
        self.sites = None
        self.after_pass = False                                      # the last step was a pass over the plain view
        self.version = 0
        self.memo = {}                                               # references of the current version

    def touch(self):
        self.version += 1
        self.memo = {}

    def cs(self, weights=None):
        """The model as a case dict of the shape the reference modules take."""
        out = dict(self.base, P=self.P[0] if self.C == 1 else self.P, root_freqs=self.pi,
                   name=f"{self.base['name']}#{self.uid}@{self.version}")
        if self.C > 1:
            out["weights"] = WEIGHTS if weights is None else weights
            out["name"] += "/" + ",".join(str(x) for x in out["weights"])     # (the reference modules cache by name)
        return out

    def prune(self, cls=None, weights=None, P=None, pinned=None, **kw):
        b = self.base
        P = self.P if P is None else P
        if cls is not None:
            P, weights = P[cls], None
        elif self.C == 1:
            P = P[0]
        return sf.prune(self.D, self.fp, self.L, b["leaf_codes"], b["ambig"], b["pattern_freq"], P, self.pi,
                        weights=weights if P.ndim == 4 else None, pinned=pinned, **kw)

    def children(self, code):
        return [c for c in range(self.B) if self.fp[c] == code - self.L]

    def pass_kinds(self):
        """The passes this partition can be asked for at all (whether one is legal NOW is ``refusal``'s and the builder's business)."""
        out = [k for k in PASSES if k not in HMM_PASSES or 2 <= self.C <= 8]
        if self.templated:
            return [k for k in out if k not in NOT_BEHIND_EXPM]
        return [k for k in out if k not in RATE_PASSES]

    def site_reference(self, cls=None, weights=None, pinned=None):
        """dict(site, total) of scalefree.prune, and where some resident matrix carries an allowance of the device's exponential the
        enclosure of mixture_cases.enclosure / catmix_cases.enclosure beside it: the reference at both ends of every matrix's interval,
        each end moved outwards by one more ulp (lo, mid, hi, width and the totals)."""
        r = self.prune(cls=cls, weights=weights, pinned=pinned)
        out = dict(site=r["site_logl"], total=r["logl"])
        if self.allow.any():
            U, al = 2.0 ** -53, self.allow.astype(np.longdouble)[:, :, None, None]
            lo = self.prune(cls=cls, weights=weights, pinned=pinned, P=np.maximum(self.PL - al, 0).astype(np.float64) * (1.0 - 2 * U))
            hi = self.prune(cls=cls, weights=weights, pinned=pinned, P=(self.PL + al).astype(np.float64) * (1.0 + 2 * U))
            out.update(lo=lo["site_logl"], mid=r["site_logl"], hi=hi["site_logl"], width=hi["site_logl"] - lo["site_logl"],
                       lo_total=lo["logl"], mid_total=r["logl"], hi_total=hi["logl"])
        return out


def label(step):
    """The name of a step in a printed sequence and in the coverage count."""
    k = step["kind"]
    if k == "evaluate":
        return step["label"]
    if k == "refused":
        return f"refused[{step['why']}:{label(step['inner'])}]"
    return k


def describe(step):
    k = step["kind"]
    if k == "refused":
        return f"refused ({step['why']}): {describe(step['inner'])}"
    if k == "evaluate":
        e = step["entry"]
        entry = e if isinstance(e, str) else f"evaluate(cat={e[1]})"
        what = "" if step["M"] is None else " matrices " + ",".join(str(int(c)) for c in step["q_nodes"][:6]) + ("..." if len(step["q_nodes"]) > 6 else "")
        return f"{step['label']}: {entry}, {len(step['update'])} update nodes{what}"
    if k in ("pin", "bc_build", "bc_eval"):
        return f"{k} node {step['node']}"
    if k == "set_repeats":
        return f"set_repeats({step['on']})"
    if k in ("trials", "derivatives", "sensitivities", "trials_built", "derivatives_built", "gradient", "gradient_built"):
        return f"{k} at {[int(x) for x in step['nodes']]}"
    if k == "nni":
        return f"nni {[tuple(int(v) for v in mv) for mv in step['moves']]}"
    return k


def _is_pass(step):
    return step["kind"] in PASSES


def held(step):
    """Whether the step returns something that is compared with a reference."""
    k = step["kind"]
    if k == "evaluate":
        return step["entry"] != "async"
    return k in PASSES or k in ("collect", "download", "bc_eval")


def refusal(m, step):
    """None when the header lets the step through, else which of REFUSALS stops it (in the order the library checks)."""
    k = step["kind"]
    if k == "simulate":                                  # (draws down the tree from the matrices alone: no conditionals, no pin)
        return None if all(m.evaluated) else "unevaluated"
    if k in PASSES:
        if m.pin is not None:
            return "pin_active"
        if any(m.pin_left):
            return "pin_left"
        if m.C > 1 and k in NEED_WEIGHTS and step.get("weights") is None:
            return "no_weights"
        if not all(m.evaluated):
            return "unevaluated"
        if k in HMM_PASSES and any(p is None or not np.array_equal(p, m.pi) for p in m.pi_at):
            return "pi_stale"
    if k == "collect" and m.pending is None:
        return "nothing_pending"
    return None


def _note_pins(m, cls, update):
    """include/hyphy_hip.h, hyphy_hip_set_pinned_states: a pin left behind goes when an evaluation without it lists the leaf, or a node
    below the internal node, or every branch."""
    up = set(int(u) for u in update)
    above = set()                                        # the internal nodes the evaluation recomputes: every ancestor of a listed node
    for u in up:
        a = int(m.fp[u])
        while a >= 0 and m.L + a not in above:
            above.add(m.L + a)
            a = int(m.fp[m.L + a])
    for c in cls:
        for n in list(m.pin_left[c]):
            if m.pin is not None and m.pin[0] == n:
                continue
            if len(up) >= m.B or (m.L + int(m.fp[n]) if n < m.L else n) in above:   # (a leaf's pin sits in its parent's conditional)
                m.pin_left[c].discard(n)
        if m.pin is not None:
            m.pin_left[c].add(m.pin[0])


def apply(m, step, mistake=None):
    """Advance the model by a step the library lets through.  ``mistake``: one of MISTAKES, the planted model errors of the CPU test."""
    k = step["kind"]
    was_pass, m.after_pass = m.after_pass, False
    if k == "refused":
        m.after_pass = was_pass
        return
    if k == "evaluate":
        e = step["entry"]
        batch = e in BATCH
        cls = list(range(m.C)) if batch else [e[1] if isinstance(e, tuple) else max(int(step.get("cat", 0)), 0)]
        partial = step["M"] is not None and len(step["q_nodes"]) < m.B
        drop = step["M"] is None or (mistake == "stale_partial" and partial) or (mistake == "async_dropped" and e == "async") or \
            (mistake == "compressed_view" and partial and was_pass)
        if not drop:
            qn = step["q_nodes"]
            M = step["M"] if batch else step["M"][None]
            into = [0] if (mistake == "slot_table" and isinstance(e, tuple) and e[1] > 0 and m.batch and partial) else cls
            for j, c in enumerate(into):
                m.PL[c][qn] = M[j]                       # (``M``: the matrices the branches hold afterwards, longdouble for a mixture)
                m.P[c][qn] = np.asarray(M[j], dtype=np.float64)
                m.allow[c][qn] = step["allow"][j] if "allow" in step else 0.0
                m.Q[c][qn] = step["Q"] if "Q" in step else np.nan
                if m.rows is not None:
                    m.rows[c][qn] = step["rows"] if "rows" in step else np.nan
        if step["M"] is not None:
            for c in cls:
                m.kind[c][step["q_nodes"]] = step["kinds"] if np.ndim(step["kinds"]) == 1 else step["kinds"][cls.index(c)]
        if mistake != "old_pi" or m.pi is None:
            if m.pi is not None and not np.array_equal(m.pi, step["pi"]):
                m.pi_at = [None] * m.C                   # (the library marks every class at any change of the frequencies)
            m.pi = step["pi"]
        for c in cls:
            m.evaluated[c] = True
            m.pi_at[c] = m.pi
            m.bc.pop(c, None)
        m.batch = batch
        if m.bc_dirty is not None and m.bc_dirty[0] in cls:
            m.bc_dirty = None
        _note_pins(m, cls, step["update"])
        m.pending = cls[0] if e == "async" else None
        if e == "async":
            m.last_async = cls[0]
        m.touch()
        return
    if k in PASSES:
        m.pending, m.after_pass = None, True
    elif k == "collect":
        m.pending = None
    elif k == "set_repeats":
        m.repeats, m.pending = bool(step["on"]), None
    elif k == "pin":
        m.pin = (int(step["node"]), np.asarray(step["states"], dtype=np.int64))
        m.bc = {}
        m.touch()
    elif k == "unpin":
        if mistake != "pin_survives":
            m.pin = None
        m.touch()
    elif k == "bc_build":
        m.bc[step["cat"]] = int(step["node"])
        m.pending = None
    elif k in ("set_templates", "update_templates"):
        m.T = np.asarray(step["T"], dtype=np.float64)
        m.rows = np.full((m.C, m.B, len(m.T)), np.nan)   # (a row says what a branch holds only under the templates it was built from)
        m.pending = None
    elif k == "bc_eval":
        m.P[step["cat"]][step["node"]] = m.PL[step["cat"]][step["node"]] = step["M"]
        m.allow[step["cat"]][step["node"]] = 0.0
        m.Q[step["cat"]][step["node"]] = step["Q"] if "Q" in step else np.nan
        if m.rows is not None:
            m.rows[step["cat"]][step["node"]] = np.nan
        m.kind[step["cat"]][step["node"]] = step["kinds"]
        m.bc_dirty = (step["cat"], int(step["node"]))
        m.pending = None
        m.touch()
    elif k == "hmm_sites":
        m.sites = np.asarray(step["sites"], dtype=np.int64)
        m.touch()
    elif k == "download":
        m.pending = None


# ---- references -------------------------------------------------------------------------------------------------------------------

def _memo(m, key, make):
    if key not in m.memo:
        m.memo[key] = make()
    return m.memo[key]


def _emissions(m):
    """The model's per-class per-pattern values as (l, c): l in (2^-64, 1] and the 2^64 exponent, (0, 0) for an impossible pattern."""
    sl = m.prune(weights=WEIGHTS)["class_site_logl"]
    fin = np.isfinite(sl)
    c = np.where(fin, np.floor(np.where(fin, -sl, 0.0) / sf.LOG_SCALER), 0.0).clip(min=0.0)
    l = np.where(fin, np.exp(np.where(fin, sl, 0.0) + c * sf.LOG_SCALER), 0.0)
    return l, c.astype(np.int64), sl


def hmm_allowance(m, sl, logl):
    from tests import hmm_ref
    sites = np.arange(m.S) if m.sites is None else m.sites
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(sl), hold.RTOL * np.abs(sl) + hold.ATOL, 0.0).max(axis=0)
    return hmm_ref.bar(len(sites), m.C, logl) + float(d[sites].sum())


def reference(m, step):
    """What the step must return on the model as it stands BEFORE the step for passes, downloads and cache evaluations, and AFTER it
    for evaluations (``apply`` is the caller's: ``expected`` does both in the right order)."""
    k = step["kind"]
    w = step.get("weights")
    if k == "evaluate" or k == "collect":
        e = step["entry"] if k == "evaluate" else ("class", m.last_async) if m.C > 1 else "evaluate"
        if e in BATCH:
            return _memo(m, ("site", "mix", tuple(w)), lambda: m.site_reference(weights=w, pinned=m.pin))
        c = e[1] if isinstance(e, tuple) else 0
        return _memo(m, ("site", c), lambda: m.site_reference(cls=c, pinned=m.pin))
    if k == "download":
        r = _memo(m, ("cond", step["cat"]), lambda: m.prune(cls=step["cat"], conditionals=True))
        return dict(cond=r["cond"], log_mag=r["log_mag"])
    if k == "bc_eval":
        P = m.P.copy()
        P[step["cat"]][step["node"]] = step["M"]
        r = m.prune(cls=step["cat"], P=P)
        return dict(site=r["site_logl"], total=r["logl"])
    if k in ("trials_built", "derivatives_built"):       # the dense call's reference on the matrices build_q forms from the rows
        from tests import expm_ref as er, template_cases as tc
        G = np.stack([np.stack([tc.rate_matrix(m.T, row) for row in rows]) for rows in step["coeffs"]])
        if k == "derivatives_built":
            return reference(m, dict(step, kind="derivatives", G=G))
        return reference(m, dict(step, kind="trials", M=np.stack([np.stack([er.reference(q) for q in qs]) for qs in G])))
    if k in RATE_PASSES:
        cs = m.cs(w)
        outs = _memo(m, "gc.outside", lambda: [gc.outside(cs, m.P[c]) for c in range(m.C)])
        douts = _memo(m, "dc.outside", lambda: [dc.outside(cs, m.P[c]) for c in range(m.C)])
        out = []
        for node in step["nodes"]:
            Qs = [m.Q[c][int(node)] for c in range(m.C)]
            r = gc.gradient(cs, outs, int(node), Qs, weights=w, T=m.T)
            r["allow_d1"] = float(dc.values(cs, douts, int(node), Qs, w)["allow_d1"])
            out.append(r)
        return out
    if k == "simulate":
        from tests import simulate_ref as mr
        n_rows = len(m.fp)
        P = m.P if m.C > 1 else m.P[0]
        return dict(supplied=mr.simulate_ref(m.fp, m.L, P, m.pi, step["u"], step.get("cls"), None),
                    philox=mr.simulate_ref(m.fp, m.L, P, m.pi, mr.uniforms(step["seed"], step["n_rep"], n_rows, step["n_sites"]), step.get("cls"), None))
    if k in ("marginal", "marginal_leaves"):
        with np.errstate(invalid="ignore"):
            r = _memo(m, ("post", None if w is None else tuple(w)), lambda: m.prune(weights=w, posteriors=True))
        return dict(post=r["post" if k == "marginal" else "leaf_post"], site=r["site_logl"])
    if k == "nni":
        cs = m.cs(w)
        return [dict(site=r["site_logl"], total=r["logl"]) for r in (nc.reference(cs, int(x), int(y)) for x, y in step["moves"])]
    if k == "trials":
        out = []
        for node, M in zip(step["nodes"], step["M"]):
            P = m.P.copy()
            P[:, int(node)] = M
            r = m.prune(weights=w, P=P)
            out.append(dict(site=r["site_logl"], total=r["logl"]))
        return out
    if k == "derivatives":
        cs = m.cs(w)
        outs = _memo(m, "dc.outside", lambda: [dc.outside(cs, m.P[c]) for c in range(m.C)])
        return [dc.values(cs, outs, int(node), list(G), w) for node, G in zip(step["nodes"], step["G"])]
    if k == "sensitivities":
        cs = m.cs(w)
        outs = _memo(m, "gc.outside", lambda: [gc.outside(cs, m.P[c]) for c in range(m.C)])
        return [gc.sensitivities(cs, outs, int(node), w) for node in step["nodes"]]
    if k == "joint":
        from tests import joint_ref as jr
        b = m.base
        return jr.joint_ref(m.D, m.fp, m.L, b["leaf_codes"], b["ambig"], m.P if m.C > 1 else m.P[0], m.pi,
                            class_of_pattern=step.get("cls"))[0]
    if k == "sample":
        used = sorted(set(int(c) for c in step["cls"])) if step.get("cls") is not None else [0]
        return dict(download={c: reference(m, dict(kind="download", cat=c)) for c in used})
    if k in HMM_PASSES:
        from tests import hmm_ref
        l, c, sl = _memo(m, "emissions", lambda: _emissions(m))
        T, f = step["T"], step["f"]
        logl = hmm_ref.to_float(hmm_ref.forward_mp(l, c, T, f, m.sites))
        if k == "hmm_logl":
            return dict(logl=logl, allow=hmm_allowance(m, sl, logl) if np.isfinite(logl) else 0.0)
        path = hmm_ref.viterbi_mp(l, c, T, f, m.sites)
        score = float(hmm_ref.path_score(l, c, T, f, m.sites, path)) if path[0] >= 0 else -np.inf
        return dict(path=path, score=score, allow=hmm_allowance(m, sl, score) if np.isfinite(score) else 0.0, l=l, c=c)
    return None


def expected(m, step, mistake=None):
    """Apply the step and return its reference (None for a step that returns nothing, or is refused)."""
    if step["kind"] == "refused":
        return None
    if step["kind"] == "evaluate":
        apply(m, step, mistake)
        return reference(m, step) if held(step) else None
    ref = reference(m, step) if held(step) else None
    apply(m, step, mistake)
    return ref


def distance(step, wrong, right):
    """How far the reference ``wrong`` lies from ``right`` in allowances of the step's own comparison (the CPU test's measure of
    what a planted model mistake does to a later held step); inf where nothing finite compares them."""
    k = step["kind"]
    if k in ("evaluate", "collect", "bc_eval"):
        return hold.miss(wrong["site"], right["site"])
    if k in ("nni", "trials", "trials_built"):
        return max(hold.miss(a["site"], b["site"]) for a, b in zip(wrong, right))
    if k in RATE_PASSES:
        return max(float(np.max(np.abs(a["S"] - b["S"]) / b["allow_S"])) for a, b in zip(wrong, right))
    if k == "simulate":
        return 0.0 if np.array_equal(wrong["supplied"], right["supplied"]) else np.inf
    if k in ("marginal", "marginal_leaves"):
        a, b = wrong["post"], right["post"]
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            return np.inf
        fin = np.isfinite(b)
        return float(np.max(np.abs(a[fin] - b[fin]) / (mc.RTOL * np.maximum(b[fin], mc.FLOOR)))) if fin.any() else 0.0
    if k in ("derivatives", "derivatives_built"):
        return max(dc.miss(a["r1"], a["r2"], a["d1"], a["d2"], b) for a, b in zip(wrong, right))
    if k == "sensitivities":
        return max(gc.miss_w(a["W"], b) for a, b in zip(wrong, right))
    if k == "joint":
        return 0.0 if np.array_equal(wrong, right) else np.inf
    if k == "hmm_logl":
        return abs(wrong["logl"] - right["logl"]) / right["allow"] if np.isfinite(right["logl"]) and right["allow"] > 0 else 0.0
    if k == "download":
        return 0.0 if np.allclose(wrong["cond"], right["cond"], rtol=1e-9, atol=1e-12) else np.inf
    return 0.0


# ---- playing a step on the device and holding what it returns -----------------------------------------------------------------------

def play(part, step):
    """The call of the step on ``part`` (a hip.HipPartition); what it returns.  Passes are called twice: identical bytes."""
    k = step["kind"]
    if k == "evaluate":
        e, M = step["entry"], step["M"]
        if e == "categories":
            return part.evaluate_categories(step["update"], step["q_nodes"], M, step["weights"], step["pi"], q_is_probability=True, per_site=True)
        if e == "async":                                 # (behind templates: the dense rate matrices of the rows)
            return part.evaluate_async(step["update"], step["q_nodes"], step["Q"] if "Q" in step else M, step["pi"], cat=step.get("cat", -1),
                                       q_is_probability="Q" not in step)
        if e == "built":
            part.build_q(step["rows"])
            return part.evaluate_built(step["update"], step["q_nodes"], step["pi"], per_site=True)
        if e == "mixture":
            return part.evaluate_mixture(step["update"], step["q_nodes"], step["components"], step["mix_weights"], step["pi"], per_site=True)
        if e == "catmix":
            return part.evaluate_categories_mixture(step["update"], step["q_nodes"], step["components"], step["mix_weights"], step["weights"],
                                                    step["pi"], per_site=True)
        return part.evaluate(step["update"], step["q_nodes"], M, step["pi"], cat=e[1] if isinstance(e, tuple) else -1,
                             q_is_probability=True, per_site=True)
    if k == "collect":
        return part.collect(per_site=True)
    if k == "download":
        return part.download_partials(step["cat"])
    if k == "set_repeats":
        return part.set_repeats(step["on"])
    if k == "pin":
        return part.set_pinned_states(step["node"], step["states"])
    if k == "unpin":
        return part.set_pinned_states(None)
    if k == "bc_build":
        return part.branch_cache_build(step["node"], step["cat"])
    if k == "bc_eval":
        return part.branch_cache_evaluate(step["node"], step["Q"] if "Q" in step else step["M"], step["cat"], q_is_probability="Q" not in step,
                                          per_site=True)
    if k == "hmm_sites":
        return part.hmm_set_sites(step["sites"])
    if k == "set_templates":
        return part.set_q_templates(step["T"])
    if k == "update_templates":
        return part.update_q_templates(step["T"])
    w = step.get("weights")
    call = {
        "marginal": lambda: part.marginal_ancestral("internal", weights=w, map=True),
        "marginal_leaves": lambda: part.marginal_ancestral("leaves", weights=w, map=True),
        "nni": lambda: part.nni_scores(step["moves"], weights=w, per_site=True),
        "trials": lambda: part.branch_trials(step["nodes"], step["M"] if part.C > 1 else step["M"][:, 0], weights=w, q_is_probability=True, per_site=True),
        "derivatives": lambda: part.branch_derivatives(step["nodes"], step["G"] if part.C > 1 else step["G"][:, 0], weights=w, per_site=True),
        "sensitivities": lambda: part.branch_sensitivities(step["nodes"], weights=w),
        "joint": lambda: (part.joint_ancestral(do_leaves=True, class_of_pattern=step.get("cls")),),
        "sample": lambda: (part.sample_ancestral(step["n_rep"], step["pos"], step.get("cls"), uniforms=step["u"]),
                           part.sample_ancestral(step["n_rep"], step["pos"], step.get("cls"), seed=step["seed"])),
        "hmm_logl": lambda: (np.array([part.hmm_logl(step["T"], step["f"])]),),
        "hmm_viterbi": lambda: (part.hmm_viterbi(step["T"], step["f"]),),
        "trials_built": lambda: part.branch_trials_built(step["nodes"], step["coeffs"] if part.C > 1 else step["coeffs"][:, 0], weights=w, per_site=True),
        "derivatives_built": lambda: part.branch_derivatives_built(step["nodes"], step["coeffs"] if part.C > 1 else step["coeffs"][:, 0], weights=w,
                                                                   per_site=True),
        "gradient": lambda: part.branch_gradient(step["nodes"], step["Q"] if part.C > 1 else step["Q"][:, 0], weights=w),
        # (with the device's own d1 of the same rows: test_gpu_gradient.py holds sum_k x_k grad_k to it)
        "gradient_built": lambda: part.branch_gradient_built(step["nodes"], step["coeffs"] if part.C > 1 else step["coeffs"][:, 0], weights=w)
        + (part.branch_derivatives_built(step["nodes"], step["coeffs"] if part.C > 1 else step["coeffs"][:, 0], weights=w)[0],),
        "simulate": lambda: (part.simulate(step["n_rep"], step["n_sites"], step.get("cls"), None, uniforms=step["u"], with_internal=True),
                             part.simulate(step["n_rep"], step["n_sites"], step.get("cls"), None, seed=step["seed"], with_internal=True),
                             part.simulate(step["n_rep"], step["n_sites"], step.get("cls"), None, seed=step["seed"])),
    }[k]
    got, again = call(), call()
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again)), f"{k}: two calls in a row differ"
    if k == "sample":                                    # the reference runs on the device's own conditionals: fetched AFTER the pass
        used = sorted(set(int(c) for c in step["cls"])) if step.get("cls") is not None else [0]
        return got + ({c: part.download_partials(c) for c in used},)
    return got


def hold_step(what, m, step, got, ref):
    """Compare what ``play`` returned with ``reference``; returns the largest deviation / allowance where the comparison has one
    (0 for exact comparisons).  ``m``: the model after the step."""
    k = step["kind"]
    if k in ("evaluate", "collect", "bc_eval"):
        if "lo" in ref:                                  # a matrix of the device's exponential is resident: the enclosure
            from tests import mixture_cases
            return mixture_cases.hold_enclosure(what, got, ref)
        hold._hold(what, got, ref["site"], ref["total"])
        return hold.miss(hold._site(got[1], got[2]), ref["site"])
    if k in RATE_PASSES:
        S_or_g, sk = got[0], got[1]
        worst = 0.0
        for t, r in enumerate(ref):
            assert int(sk[t]) == r["n_skipped"], (what, t, int(sk[t]), r["n_skipped"])
            if k == "gradient":
                x = float(np.max(np.abs(np.asarray(S_or_g[t]).reshape(r["S"].shape) - r["S"]) / r["allow_S"]))
            else:
                g, co = np.asarray(S_or_g[t]).reshape(r["grad"].shape), np.asarray(step["coeffs"][t]).reshape(r["grad"].shape)
                x = float(np.max(np.abs(g - r["grad"]) / r["allow_grad"]))
                both = r["allow_d1"] + float(np.sum(np.abs(co) * r["allow_grad"]))
                assert abs(float(got[2][t]) - float(np.sum(co * g))) <= both, (what, t, float(got[2][t]), float(np.sum(co * g)), both)
            print(f"{what} [{t}]: {x:.3g} of the allowance")
            assert x <= 1.0, (what, t, x)
            worst = max(worst, x)
        return worst
    if k == "simulate":
        for name, x, want in (("supplied", got[0], ref["supplied"]), ("philox", got[1], ref["philox"]), ("leaves", got[2], ref["philox"][:, :m.L])):
            bad = np.argwhere(x != want)
            assert x.dtype == np.int8 and x.shape == want.shape and len(bad) == 0, (what, name, len(bad), bad[:5].tolist())
        return 0.0
    if k == "download":
        hold.hold_download(what, got[0], got[1], ref["cond"], ref["log_mag"])
        return 0.0
    if k in ("marginal", "marginal_leaves"):
        sup, ms, mv = got
        gone = np.isneginf(ref["site"])
        assert np.isnan(ref["post"][:, gone]).all() and np.isnan(sup[:, gone]).all(), what
        mc.hold_support(what, sup, ref["post"], sums_to_one=k == "marginal")
        mc.hold_map(what, ms, mv, sup, ref["post"])
        return distance(step, dict(post=sup), ref)
    if k in ("nni", "trials", "trials_built"):
        ll, lik, sc = got
        worst = 0.0
        for t, r in enumerate(ref):
            hold._hold(f"{what} [{t}]", (float(ll[t]), lik[t], sc[t]), r["site"], r["total"])
            assert np.array_equal(lik[t] == 0.0, np.isneginf(r["site"])), (what, t)
            worst = max(worst, hold.miss(hold._site(lik[t], sc[t]), r["site"]))
        return worst
    if k in ("derivatives", "derivatives_built"):
        d1, d2, sk, s1, s2 = got
        worst = 0.0
        for t, r in enumerate(ref):
            x = dc.miss(s1[t], s2[t], d1[t], d2[t], r)
            assert x <= 1.0, (what, t, x)
            assert int(sk[t]) == r["n_skipped"], (what, t, int(sk[t]), r["n_skipped"])
            assert np.array_equal(np.isnan(s1[t]), np.isnan(r["r1"])) and np.array_equal(np.isnan(s2[t]), np.isnan(r["r1"])), (what, t)
            worst = max(worst, x)
        return worst
    if k == "sensitivities":
        W, sk = got
        worst = 0.0
        for t, r in enumerate(ref):
            x = gc.miss_w(W[t], r)
            assert x <= 1.0, (what, t, x)
            assert int(sk[t]) == r["n_skipped"], (what, t, int(sk[t]), r["n_skipped"])
            worst = max(worst, x)
        return worst
    if k == "joint":
        bad = np.argwhere(got[0] != ref)
        assert got[0].shape == ref.shape and len(bad) == 0, (what, len(bad), bad[:5].tolist())
        return 0.0
    if k == "sample":
        from tests import sample_ref as sr
        supplied, philox, down = got
        for c, (cache, counts) in down.items():
            hold.hold_download(f"{what}: the conditionals of class {c}", cache, counts, ref["download"][c]["cond"], ref["download"][c]["log_mag"])
        cond = np.stack([down[c][0] if c in down else np.zeros_like(next(iter(down.values()))[0]) for c in range(m.C)])
        n_sites = m.S if step["pos"] is None else len(step["pos"])
        P = m.P if m.C > 1 else m.P[0]
        for name, x, u in (("supplied", supplied, step["u"]), ("philox", philox, sr.uniforms(step["seed"], step["n_rep"], len(m.fp) - m.L, n_sites))):
            want = sr.sample_ref(m.fp, m.L, cond if m.C > 1 else cond[0], P, m.pi, u, step["pos"], step.get("cls"))
            bad = np.argwhere(x != want)
            assert x.dtype == np.int8 and x.shape == want.shape and len(bad) == 0, (what, name, len(bad), bad[:5].tolist())
        return 0.0
    if k == "hmm_logl":
        x = float(got[0][0])
        if not np.isfinite(ref["logl"]):
            assert (np.isnan(x) if np.isnan(ref["logl"]) else x == ref["logl"]), (what, x, ref["logl"])
            return 0.0
        print(f"{what}: log L {x!r} against {ref['logl']!r}, allowance {ref['allow']:.3e}")
        assert abs(x - ref["logl"]) <= ref["allow"], (what, x, ref["logl"], ref["allow"])
        return abs(x - ref["logl"]) / ref["allow"]
    if k == "hmm_viterbi":
        from tests import hmm_ref
        path = got[0]
        assert path.dtype == np.int8 and path.shape == ref["path"].shape, what
        if not np.isfinite(ref["score"]):
            assert np.all(path == -1), what
            return 0.0
        assert path.min() >= 0 and path.max() < m.C, (what, path)
        score = float(hmm_ref.path_score(ref["l"], ref["c"], step["T"], step["f"], m.sites, path))
        print(f"{what}: the path's score {score!r} against the best {ref['score']!r}, allowance {ref['allow']:.3e}")
        assert score >= ref["score"] - ref["allow"], (what, score, ref["score"], ref["allow"])
        return max(0.0, ref["score"] - score) / ref["allow"]
    raise AssertionError(f"{k} returns nothing to hold")


# ---- building sequences -----------------------------------------------------------------------------------------------------------

class Builder:
    """Appends steps while keeping a model of its own, so that every step is drawn against the state it will meet."""

    def __init__(self, profile, tag):
        self.profile = profile
        self.base = case(profile)
        self.m = Model(self.base, classes(profile))
        self.rng = np.random.default_rng([int(self.base["seed"]), *[ord(ch) for ch in str(tag)]])
        self.steps = []
        self.chain = None
        self.weights = WEIGHTS if self.m.C > 1 else None
        self.position = 0                                # (class-compressed profiles: whose turn among the positions a - f)

    # -- plumbing
    def add(self, step, why=None):
        got = refusal(self.m, step)
        assert got == why, (self.profile, label(step), "refusal", got, "expected", why)
        if why is not None:
            step = dict(kind="refused", inner=step, why=why)
        apply(self.m, step)
        self.steps.append(step)
        return step

    def pi(self, new=False):
        if new or self.m.pi is None:
            if self.m.pi is None:
                return np.asarray(self.base["root_freqs"], dtype=np.float64)
            p = self.rng.random(self.m.D) + 0.05
            return p / p.sum()
        return self.m.pi

    def matrix(self, kind):
        D = self.m.D
        if kind == 1:
            return sf.near_identity(self.rng, 1, D, float(self.rng.choice(TINY_EPS)))[0]
        return sf.ordinary(self.rng, 1, D)[0]

    def all_matrices(self, first=False):
        """Every (class, branch): the case's own at the start; later ordinary on two branches in three and near-identity on the rest."""
        m = self.m
        if first:
            P = np.asarray(self.base["P"], dtype=np.float64).reshape(m.C, m.B, m.D, m.D).copy()
            off = P[:, :, 0, 1]
            return P, (off < 1e-8).astype(np.int64)
        kinds = (self.rng.random((m.C, m.B)) < 1.0 / 3).astype(np.int64)
        P = np.stack([np.stack([self.matrix(kinds[c, b]) for b in range(m.B)]) for c in range(m.C)])
        return P, kinds

    def branches(self, n):
        """``n`` branches; on a class-compressed profile one of each position a - f of compressed_cases.kinds_at in turn."""
        if expectations(self.profile).get("in_use"):
            kinds = cc.kinds_at(self.base, cc.THETA_PLAN)
            out = set()
            while len(out) < n:
                cand = kinds["abcdef"[self.position % 6]]
                self.position += 1
                if cand:
                    out.add(int(cand[int(self.rng.integers(len(cand)))]))
            return np.array(sorted(out), dtype=np.int64)
        return np.sort(self.rng.choice(self.m.B, size=n, replace=False)).astype(np.int64)

    def entry(self, cat=None):
        if self.m.C == 1:
            return "evaluate"
        return "categories" if cat is None else ("class", int(cat))

    # -- templates: every matrix of the profile is exp of the rate matrix build_q forms from a coefficient row
    def templates(self, update=False):
        m = self.m
        if update:
            T = m.T * self.rng.uniform(0.5, 1.5, size=m.T.shape)          # new VALUES, the same sparsity
        elif m.templated:
            T = np.asarray(self.base["T"], dtype=np.float64)
        else:
            T = (self.rng.random((2, m.D, m.D)) + 0.05) * (self.rng.random((2, m.D, m.D)) < 0.5)
            T[:, np.arange(m.D), np.arange(m.D)] = 0.0
        self.add(dict(kind="update_templates" if update else "set_templates", T=T))

    def row(self, kind):
        """A coefficient row: 0.01 .. 0.05, a thousand times less for the other kind (what a change step swaps between)."""
        return self.rng.uniform(0.01, 0.05, size=len(self.m.T)) * (1e-3 if kind == 1 else 1.0)

    def built(self, rows):
        """(rows, the rate matrices build_q forms from them, their exponentials) as template_cases.replay keeps them."""
        from tests import expm_ref as er, template_cases as tc
        Q = np.stack([tc.rate_matrix(self.m.T, r) for r in rows])
        return dict(rows=np.asarray(rows, dtype=np.float64), Q=Q, M=np.stack([er.reference(q) for q in Q]))

    def built_step(self, lab, codes, rows, kinds, entry="built", update=None):
        step = dict(kind="evaluate", label=("" if entry == "async" else "built_") + lab, entry=entry, update=codes if update is None else update,
                    q_nodes=codes, kinds=kinds,
                    pi=self.pi(), weights=None, **self.built(rows))
        if entry == "async":
            step["cat"] = -1
        return self.add(step)

    # -- evaluation-like steps
    def full(self, lab="full", cat=None, first=False):
        m = self.m
        n = np.arange(m.B, dtype=np.int64)
        if m.templated:
            kinds = np.zeros(m.B, dtype=np.int64) if first else (self.rng.random(m.B) < 1.0 / 3).astype(np.int64)
            rows = np.asarray(self.base["x"], dtype=np.float64) if first else np.stack([self.row(k) for k in kinds])
            return self.built_step(lab, n, rows, kinds)
        P, kinds = self.all_matrices(first)
        e = self.entry(cat)
        M, kd = (P, kinds) if e == "categories" else (P[cat or 0], kinds[cat or 0])
        return self.add(dict(kind="evaluate", label=lab, entry=e, update=n, q_nodes=n, M=M, kinds=kd, pi=self.pi(), weights=self.weights))

    def mixture(self):
        """Two branches become branch-site mixtures of two and three named rate matrices of tests/expm_ref.py (every class its own, under
        the same counts): the device exponentiates them, so the branches carry mixture_cases' allowance until they are replaced."""
        from tests import mixture_cases as mx
        m = self.m
        like = dict(D=m.D, deep=False, K=0)
        codes, counts = self.branches(2), (2, 3)
        kern = mx.kernel_for(like, m.C * sum(counts))
        M, allow, comps, mixw = [], [], [], []
        for _ in range(m.C):
            brs = [mx.draw_branch(like, self.rng, n).under(kern) for n in counts]
            P, a = mx.matrices(brs)
            q, w = mx.dense_input(like, brs)
            M.append(P), allow.append(a), comps.append(q), mixw.append(w)
        one = m.C == 1
        return self.add(dict(kind="evaluate", label="mixture" if one else "catmix", entry="mixture" if one else "catmix", update=codes, q_nodes=codes,
                             M=M[0] if one else np.stack(M), allow=allow, kinds=np.zeros(2, dtype=np.int64) if one else np.zeros((m.C, 2), dtype=np.int64),
                             components=comps[0] if one else comps, mix_weights=mixw[0] if one else mixw, pi=self.pi(), weights=self.weights))

    def partial(self, codes=None, lab="partial", cat=None, entry=None):
        """The listed branches (default: one to three drawn ones) swap between ordinary and near-identity."""
        m = self.m
        codes = self.branches(int(self.rng.integers(1, 4))) if codes is None else np.asarray(sorted(codes), dtype=np.int64)
        if m.templated:
            kinds = 1 - m.kind[0][codes]
            return self.built_step(lab, codes, np.stack([self.row(k) for k in kinds]), kinds, entry or "built")
        e = entry or self.entry(cat)
        cls = list(range(m.C)) if e == "categories" else [e[1] if isinstance(e, tuple) else (cat or 0)]
        kinds = np.stack([1 - m.kind[c][codes] for c in cls])
        M = np.stack([np.stack([self.matrix(k) for k in kinds[j]]) for j in range(len(cls))])
        if e != "categories":
            M, kinds = M[0], kinds[0]
        step = dict(kind="evaluate", label=lab, entry=e, update=codes, q_nodes=codes, M=M, kinds=kinds, pi=self.pi(), weights=self.weights)
        if e == "async":
            step["cat"] = cls[0] if m.C > 1 else -1
        return self.add(step)

    def again(self, lab="again", new_pi=False, update=NONE, cat=None):
        return self.add(dict(kind="evaluate", label=lab, entry=self.entry(cat), update=np.asarray(update, dtype=np.int64), q_nodes=NONE, M=None,
                             kinds=None, pi=self.pi(new_pi), weights=self.weights))

    def pin(self, node=None):
        m = self.m
        node = int(self.rng.integers(m.L, m.L + len(m.fp) - m.L - 1)) if node is None else int(node)
        states = ((np.arange(m.S) * 5 + 1 + node) % m.D).astype(np.int64)
        self.add(dict(kind="pin", node=node, states=states))
        return node

    def path(self, node):
        return mc.pin_update_list(self.m.fp, self.m.L, node)

    # -- passes
    def a_pass(self, kind, why=None, weights="default"):
        m, rng = self.m, self.rng
        w = self.weights if isinstance(weights, str) else weights
        if m.C > 1 and w is not None and kind in ("marginal", "nni", "trials") and rng.random() < 0.3:
            w = WEIGHTS_ZERO
        step = dict(kind=kind, weights=w)
        cls = rng.integers(0, m.C, size=m.S).astype(np.int64) if m.C > 1 else None
        if kind == "nni":
            mv = nc.enumerate_moves(m.fp, m.L)
            step["moves"] = np.array([mv[i] for i in rng.choice(len(mv), size=min(4, len(mv)), replace=False)], dtype=np.int64)
        elif kind in ("trials", "derivatives", "sensitivities"):
            nodes = rng.choice(m.B, size=3, replace=False).astype(np.int64)
            step["nodes"] = nodes
            if kind == "trials":
                picks = rng.integers(1, len(bc.TRIAL_KINDS), size=3)
                cs = m.cs()
                step["M"] = np.stack([np.stack([bc.trials(dict(cs, P=m.P[c]), int(b), None)[k][1] for c in range(m.C)]) for b, k in zip(nodes, picks)])
            if kind == "derivatives":
                picks = rng.integers(0, len(dc.KINDS), size=3)
                step["G"] = np.stack([np.stack([dc.generators(self.base, int(b), c)[k][1] for c in range(m.C)]) for b, k in zip(nodes, picks)])
        elif kind in ("trials_built", "derivatives_built", "gradient", "gradient_built"):
            # (the rate passes: branches whose matrix is exp of a known rate matrix — and was built from a known row under these templates)
            ok = [b for b in range(m.B) if not np.isnan(m.Q[:, b]).any() and (kind != "gradient_built" or not np.isnan(m.rows[:, b]).any())]
            nodes = rng.choice(ok if kind in RATE_PASSES else m.B, size=3, replace=False).astype(np.int64)
            step["nodes"] = nodes
            if kind == "trials_built":
                step["coeffs"] = rng.uniform(0.002, 0.02, size=(3, m.C, len(m.T)))
            elif kind == "derivatives_built":
                step["coeffs"] = rng.uniform(0.002, 0.3, size=(3, m.C, len(m.T))) / m.D
            elif kind == "gradient":
                step["Q"] = np.stack([m.Q[:, int(b)] for b in nodes])
            else:
                step["coeffs"] = np.stack([m.rows[:, int(b)] for b in nodes])
        elif kind == "simulate":
            n_sites = 37
            step.update(n_rep=2, n_sites=n_sites, seed=int(rng.integers(1, 2 ** 31)), u=rng.random((2, len(m.fp), n_sites)),
                        cls=rng.integers(0, m.C, size=(2, n_sites)).astype(np.int64) if m.C > 1 else None)
        elif kind == "joint":
            step["cls"] = cls
        elif kind == "sample":
            pos = None if rng.random() < 0.5 else rng.integers(0, m.S, size=m.S + 5).astype(np.int64)
            n_sites = m.S if pos is None else len(pos)
            step.update(n_rep=2, pos=pos, cls=cls, seed=int(rng.integers(1, 2 ** 31)), u=rng.random((2, len(m.fp) - m.L, n_sites)))
        elif kind in HMM_PASSES:
            if self.chain is None:
                from tests import hmm_ref
                self.chain = hmm_ref.random_chain(np.random.default_rng(int(self.base["seed"])), m.C)
            step["T"], step["f"] = self.chain
        return self.add(step, why)

    def pass_kinds(self):
        return self.m.pass_kinds()

    def ready(self, kind):
        """What a pass needs beside what ``refusal`` looks at: templates for the built forms (set here when there are none)."""
        if kind in BUILT_PASSES and self.m.T is None:
            self.templates()

    def hmm_sites(self):
        m = self.m
        sites = self.rng.integers(0, m.S, size=40).astype(np.int64)
        self.add(dict(kind="hmm_sites", sites=sites))

    # -- the predecessors of a pass (PREDECESSORS)
    def predecessor(self, which):
        """Steps after which a pass follows directly; False when the profile has no such predecessor."""
        m = self.m
        if which == "lazy_full":
            if m.templated:                              # (new template values between passes: every branch is rebuilt under them)
                self.templates(update=True)
                self.full()
            elif not (self.steps and label(self.steps[-1]).endswith("full")):
                self.full()
            self.full("lazy_full")
        elif which == "partial":
            self.partial()
        elif which == "pass":
            kind = str(self.rng.choice(self.pass_kinds()))
            self.ready(kind)
            self.a_pass(kind)
        elif which == "unpin_reeval":
            node = self.pin()
            self.again("pinned", update=self.path(node))
            self.add(dict(kind="unpin"))
            self.again("unpinned", update=self.path(node))
        elif which == "repeats_toggle":
            self.add(dict(kind="set_repeats", on=not m.repeats))
        elif which == "pi_only":
            self.again("pi_only", new_pi=True)
        elif which == "async":
            self.partial(self.branches(2), lab="async", entry="async")
        elif which == "bc_build":
            if m.D < 5:
                return False
            self.add(dict(kind="bc_build", node=int(self.rng.integers(0, m.B)), cat=int(self.rng.integers(0, m.C))))
        return True

    def refused(self, why, kind=None):
        """One refused step of the kind ``why``, set up and taken down around it where the state has to be made."""
        m = self.m
        # (a hidden-Markov pass without a site list is refused for that, before anything else is looked at)
        # (simulate reads no conditionals: a pin does not stop it; the built forms without templates are refused for that)
        kind = kind or str(self.rng.choice([k for k in self.pass_kinds() if (k not in HMM_PASSES or m.sites is not None) and k != "simulate"
                                            and (k not in BUILT_PASSES + RATE_PASSES or (m.T is not None and all(m.evaluated)))]))
        if why == "nothing_pending":
            self.add(dict(kind="collect"), why)
        elif why == "no_weights":
            self.a_pass(str(self.rng.choice(["nni", "trials", "derivatives", "sensitivities"])), why, weights=None)
        elif why == "pin_active":
            self.pin()
            self.a_pass(kind, why)
            self.add(dict(kind="unpin"))                   # (no evaluation ran under it: nothing is left behind)
        elif why == "unevaluated":
            self.a_pass(kind, why)


def close_cache(b):
    """A cache evaluation on a cache that is still built, and the partial update that lists the branch afterwards."""
    m = b.m
    if not m.bc:
        return
    cat, node = sorted(m.bc.items())[0]
    k = 1 - m.kind[cat][node]
    if m.templated:                                       # the trial as a rate matrix, then the branch rebuilt from the same row
        f = b.built([b.row(k)])
        b.add(dict(kind="bc_eval", node=node, cat=cat, M=f["M"][0], Q=f["Q"][0], kinds=k))
        b.built_step("partial", np.array([node], dtype=np.int64), f["rows"], np.array([k]), update=b.path(node))
        return
    b.add(dict(kind="bc_eval", node=node, cat=cat, M=b.matrix(k), kinds=k))
    P = m.P[cat][node]
    e = "evaluate" if m.C == 1 else ("class", cat)
    b.add(dict(kind="evaluate", label="partial", entry=e, update=b.path(node) if node >= m.L else np.array([node]), q_nodes=np.array([node]),
               M=P[None].copy(), kinds=np.array([k]), pi=b.pi(), weights=b.weights))


def _applies(pair, m):
    pred, kind = pair
    return not (pred == "bc_build" and m.D < 5) and kind in m.pass_kinds()


def _deck():
    """Every (predecessor, pass kind) pair in one fixed order."""
    pairs = [(p, k) for p in PREDECESSORS for k in PASSES]
    return [pairs[i] for i in np.random.default_rng(7577).permutation(len(pairs))]


@functools.lru_cache(maxsize=None)
def _plan():
    """The committed sequences, drawn one after the other: each takes from the deck the first pairs its profile can run that no
    sequence before it has taken (the rate-class profiles first: only they can run the hidden-Markov passes), and deals from the
    whole deck once nothing is left.  Together the committed seeds therefore reach every pair."""
    left = _deck()
    out = {}
    few = HMM_PASSES + RATE_PASSES                       # the kinds only some profiles can run: those profiles go first and take them first
    order = sorted(PROFILES, key=lambda p: classes(p) == 1 and not expectations(p).get("templates"))
    for profile in order:
        for seed in SEEDS:
            turn = [0]

            def deal(m, short=False):
                mine = [q for q in left if _applies(q, m) and (not short or q[0] in SHORT)]
                if short and not mine:
                    return None
                if any(q[1] in few for q in mine):
                    mine = [q for q in mine if q[1] in few]
                if turn[0] == 0 and expectations(profile).get("in_use") and any(q[0] == "unpin_reeval" for q in mine):
                    mine = [q for q in mine if q[0] == "unpin_reeval"]       # (every class-compressed sequence evaluates under a pin
                if turn[0] == 1 and expectations(profile).get("in_use") and any(q[0] == "repeats_toggle" for q in mine):
                    mine = [q for q in mine if q[0] == "repeats_toggle"]     #  and turns the compressed form off and on again)
                if mine:
                    turn[0] += 1
                    left.remove(mine[0])
                    return mine[0]
                deck = [q for q in _deck() if _applies(q, m)]
                turn[0] += 1
                return deck[(7 * SEEDS.index(seed) + turn[0]) % len(deck)]
            out[(profile, seed)] = tuple(_draw(seed, profile, deal))
    # (three sequences behind templates cannot hold all sixteen pairs of the two rate passes: the fixed sequence
    #  ``templates_every_predecessor`` holds every one of them)
    assert all(q[1] in RATE_PASSES for q in left), (len(left), left)
    return out


def draw(seed, profile):
    """14 - 20 steps: two full passes (the second lazy), then (predecessor, pass) blocks dealt from the deck with refused steps and
    downloads in between, an open branch cache closed, a last partial update and a last full pass.  A committed seed deals what
    ``_plan`` gives it, any other seed deals from the deck at a place of its own."""
    if seed in SEEDS:
        return list(_plan()[(profile, seed)])
    at = [int(seed) * 5]

    def deal(m, short=False):
        deck = [q for q in _deck() if _applies(q, m) and (not short or q[0] in SHORT)]
        at[0] += 1
        return deck[at[0] % len(deck)]
    return _draw(seed, profile, deal)


def _draw(seed, profile, deal):
    b = Builder(profile, seed)
    m, rng = b.m, b.rng
    if rng.random() < 0.5:
        b.refused("unevaluated")
    if m.templated:
        b.templates()
    b.full(first=True)
    b.full("lazy_full")
    if 2 <= m.C <= 8:
        b.hmm_sites()
    refusals = sum(s["kind"] == "refused" for s in b.steps)

    def may_refuse():
        return 5 * (refusals + 1) <= len(b.steps) + 1

    while len(b.steps) < 13:
        pair = deal(m, short=len(b.steps) == 12)          # (at twelve steps only a predecessor of one step still fits)
        if pair is None:
            break
        pred, kind = pair
        b.ready(kind)
        b.predecessor(pred)
        b.a_pass(kind)
        if pred == "async" and may_refuse() and rng.random() < 0.7:
            b.refused("nothing_pending")                  # (the pass finished the pending evaluation)
            refusals += 1
        if pred == "bc_build":
            close_cache(b)
            if m.C > 1:
                b.again()                                 # (all classes behind the one-class update: a matrix in another class's slot shows)
        elif pred == "pass" and m.C > 1:
            b.partial(cat=int(rng.integers(0, m.C)), lab="class_partial")    # one class after the batch: the r06 slot-table path
            b.partial()
        elif pred == "pass" and rng.random() < 0.5:
            b.add(dict(kind="download", cat=0))
        if m.C > 1 and len(b.steps) <= 13 and may_refuse() and not any(x["kind"] == "refused" and x["why"] == "no_weights" for x in b.steps):
            b.refused("no_weights")
            refusals += 1
        elif len(b.steps) <= 11 and may_refuse() and rng.random() < 0.5:
            why = str(rng.choice(["pin_active", "nothing_pending"]))
            b.refused(why)
            refusals += 1
    if not m.repeats:
        b.add(dict(kind="set_repeats", on=True))
    if len(b.steps) <= 13 and rng.random() < 0.5:
        b.partial(b.branches(2), lab="async", entry="async")
        b.add(dict(kind="collect"))
    if m.D in MIXTURE_D and not m.templated and len(b.steps) <= 16:
        b.mixture()                                       # (no pass behind it: the last full pass replaces the mixture branches first)
        b.again()                                         # (nothing dirty: the mixture branches' matrices are what the device kept)
    while (sum(held(s) for s in b.steps) < 8 or len(b.steps) < 12) and len(b.steps) < 18:
        b.again()                                         # (an evaluation with nothing dirty: ten held steps with the two below)
    b.partial()
    b.full()
    assert 14 <= len(b.steps) <= 20, (profile, seed, len(b.steps))
    return b.steps


# ---- the fixed sequences ----------------------------------------------------------------------------------------------------------

def _start(profile, tag, lazy=True):
    b = Builder(profile, tag)
    b.templates()                                         # (for the built forms of the passes; behind templates: for everything)
    b.full(first=True)
    if lazy:
        b.full("lazy_full")
    if expectations(profile).get("in_use"):
        b.full("lazy_full")                               # (the third evaluation is a compressed pass over resident tables)
    if 2 <= b.m.C <= 8:
        b.hmm_sites()
    return b


def pin_then_pass(profile):
    """A pinned evaluation, the pin removed, then every pass at once: refused (the stored values still hold the pin) until the path
    is evaluated again, then held."""
    b = _start(profile, "pin_then_pass")
    node = b.pin(b.m.L + (len(b.m.fp) - b.m.L) // 2)
    b.again("pinned", update=b.path(node))
    b.add(dict(kind="unpin"))
    for k in b.pass_kinds():
        if k != "simulate":                               # (simulate reads the matrices alone and is served: not drawn before the path is back)
            b.a_pass(k, "pin_left")
    b.again("unpinned", update=b.path(node))
    for k in b.pass_kinds():
        b.a_pass(k)
    leaf = 1
    b.pin(leaf)
    b.again("pinned", update=b.path(leaf))
    b.add(dict(kind="unpin"))
    b.a_pass("marginal", "pin_left")
    b.full()                                              # (a full pass puts everything back as well)
    b.a_pass("marginal")
    b.full()              # (class-compressed: the first evaluation behind a pass rebuilds the class tables and is not the trunk walk yet)
    b.full("lazy_full")
    return b.steps


def compressed_pass_then_partial(profile):
    """Every pass kind on a partition that runs class-compressed, each followed by a partial update inside a class table (a or b of
    compressed_cases.kinds_at), one on the trunk (d) and a full pass."""
    b = _start(profile, "compressed_pass_then_partial")
    kinds = cc.kinds_at(b.base, cc.THETA_PLAN)
    inside, trunk = (kinds["a"] + kinds["b"]) or kinds["e"], kinds["d"] or kinds["e"] or kinds["c"]
    for j, k in enumerate(b.pass_kinds()):
        b.a_pass(k)
        b.partial([inside[j % len(inside)]])
        b.partial([trunk[j % len(trunk)]])
        if j % 3 == 2:
            b.full()
    b.full()
    b.full("lazy_full")                                   # (the kind of pass the partition was left in before the first pass)
    return b.steps


def lazy_batch_then_one_class(profile):
    """Found by the drawn sequences: a lazy batched full pass leaves no class's conditionals persisted, a one-class partial update
    restores that class's alone, and the batched partial update that follows has to restore the others before it walks them."""
    b = _start(profile, "lazy_batch_then_one_class")
    for c in (1, 0):
        b.full()
        b.full("lazy_full")
        b.partial(cat=c, lab="class_partial")
        b.partial()
        b.a_pass("marginal")
        b.a_pass("hmm_logl")
    b.full()
    return b.steps


def async_then_pass(profile):
    """evaluate_async with two changed branches, a pass without collect (it equals the reference of the NEW matrices), collect refused."""
    b = _start(profile, "async_then_pass")
    for k in b.pass_kinds():
        b.partial(b.branches(2), lab="async", entry="async")
        b.a_pass(k)
        b.refused("nothing_pending")
        b.partial()
    b.partial(b.branches(2), lab="async", entry="async")
    b.add(dict(kind="collect"))
    b.full()
    return b.steps


def cache_across_passes(profile):
    """A branch cache built behind a lazy full pass, every pass kind once, then the cache evaluated and the branch's path updated."""
    b = _start(profile, "cache_across_passes")
    node = b.m.L + 1
    b.add(dict(kind="bc_build", node=node, cat=0))
    for k in b.pass_kinds():
        b.a_pass(k)
    close_cache(b)
    b.full()
    return b.steps


def pi_only(profile):
    """New root frequencies and nothing to update, then every pass kind; with classes, one class alone under new frequencies again."""
    b = _start(profile, "pi_only")
    b.again("pi_only", new_pi=True)
    for k in b.pass_kinds():
        b.a_pass(k)
    if b.m.C > 1:
        # one class alone under new frequencies: the conditionals of the others do not depend on them, their per-pattern values do —
        # the passes over the conditionals are held, the hidden-Markov ones refused until every class has been combined again
        b.again("class_pi_only", new_pi=True, cat=1)
        for k in b.pass_kinds():
            b.a_pass(k, "pi_stale" if k in HMM_PASSES else None)
        b.again()
        for k in HMM_PASSES:
            b.a_pass(k)
    b.full()
    return b.steps


def templates_every_predecessor(profile):
    """Behind templates: branch_gradient and branch_gradient_built directly after every predecessor of sequence_cases.PREDECESSORS (three
    drawn sequences cannot hold all sixteen pairs), new template values and a rebuilt tree in between."""
    b = _start(profile, "templates_every_predecessor")
    for pred in PREDECESSORS:
        for k in RATE_PASSES:
            b.predecessor(pred)
            b.a_pass(k)
            if pred == "async":
                b.refused("nothing_pending")
            if pred == "bc_build":
                close_cache(b)
    # the built forms of trials and derivatives directly behind new template values, before and after the tree is rebuilt under them
    # (before: the trial rows are built from the NEW values while every resident matrix is still one of the OLD ones)
    b.templates(update=True)
    b.a_pass("trials_built")
    b.full()
    b.a_pass("trials_built")
    b.a_pass("gradient_built")                            # (holds the device's derivatives_built of the same rows beside the gradient)
    b.add(dict(kind="set_repeats", on=True))
    b.partial()
    b.full()
    return b.steps


FIXED = {"templates_every_predecessor": templates_every_predecessor, "pin_then_pass": pin_then_pass, "compressed_pass_then_partial": compressed_pass_then_partial, "async_then_pass": async_then_pass,
         "cache_across_passes": cache_across_passes, "pi_only": pi_only, "lazy_batch_then_one_class": lazy_batch_then_one_class}
FIXED_PROFILES = {"templates_every_predecessor": ("templates",), "pin_then_pass": ("wave_lazy", "compressed", "nuc", "classes20"), "compressed_pass_then_partial": ("compressed",),
                  "async_then_pass": ("wave_lazy", "compressed", "nuc"), "cache_across_passes": ("wave_lazy", "compressed"),
                  "pi_only": ("wave_lazy", "compressed", "nuc", "classes20"), "lazy_batch_then_one_class": ("classes", "classes20")}


@functools.lru_cache(maxsize=None)
def sequence(profile, which):
    """The steps of a committed seed (an int) or a fixed sequence (its name); not to be written to."""
    return tuple(FIXED[which](profile) if which in FIXED else draw(which, profile))


def all_sequences():
    return [(p, s) for p in PROFILES for s in SEEDS] + [(p, f) for f in FIXED for p in FIXED_PROFILES[f]]


# The step list every committed seed expands to (tests/test_sequence_cases_cpu.py holds ``draw`` to it).
EXPANDS = {
    ('wave_lazy', 1): ('refused[unevaluated:sample]', 'full', 'lazy_full', 'nni', 'joint', 'set_templates', 'async',
        'derivatives_built', 'simulate', 'marginal', 'download', 'derivatives_built', 'sample', 'async', 'collect', 'mixture', 'again',
        'partial', 'full'),
    ('wave_lazy', 2): ('refused[unevaluated:joint]', 'full', 'lazy_full', 'partial', 'simulate', 'bc_build', 'marginal', 'bc_eval',
        'partial', 'pi_only', 'derivatives', 'joint', 'simulate', 'async', 'collect', 'mixture', 'again', 'partial', 'full'),
    ('wave_lazy', 3): ('refused[unevaluated:marginal_leaves]', 'full', 'lazy_full', 'async', 'marginal_leaves', 'joint', 'derivatives',
        'download', 'partial', 'marginal_leaves', 'set_templates', 'pi_only', 'trials_built', 'mixture', 'again', 'partial', 'full'),
    ('workgroup', 1): ('full', 'lazy_full', 'set_repeats', 'marginal', 'partial', 'sample', 'refused[nothing_pending:collect]',
        'set_templates', 'set_repeats', 'derivatives_built', 'bc_build', 'derivatives', 'bc_eval', 'partial', 'partial', 'full'),
    ('workgroup', 2): ('refused[unevaluated:nni]', 'full', 'lazy_full', 'set_repeats', 'marginal_leaves', 'set_templates', 'full',
        'lazy_full', 'trials_built', 'full', 'lazy_full', 'nni', 'marginal_leaves', 'trials', 'set_repeats', 'partial', 'full'),
    ('workgroup', 3): ('full', 'lazy_full', 'bc_build', 'joint', 'bc_eval', 'partial', 'partial', 'derivatives', 'set_repeats',
        'sample', 'pin', 'refused[pin_active:trials]', 'unpin', 'set_repeats', 'partial', 'full'),
    ('rerooted', 1): ('full', 'lazy_full', 'pin', 'pinned', 'unpin', 'unpinned', 'marginal_leaves', 'set_templates', 'sample',
        'derivatives_built', 'download', 'refused[nothing_pending:collect]', 'partial', 'derivatives_built', 'mixture', 'again',
        'partial', 'full'),
    ('rerooted', 2): ('full', 'lazy_full', 'lazy_full', 'marginal', 'refused[nothing_pending:collect]', 'set_templates', 'pi_only',
        'derivatives_built', 'async', 'sample', 'pin', 'pinned', 'unpin', 'unpinned', 'sample', 'mixture', 'again', 'partial', 'full'),
    ('rerooted', 3): ('refused[unevaluated:nni]', 'full', 'lazy_full', 'pi_only', 'nni', 'sample', 'marginal_leaves', 'pin', 'pinned',
        'unpin', 'unpinned', 'derivatives', 'set_templates', 'async', 'trials_built', 'refused[nothing_pending:collect]', 'mixture',
        'again', 'partial', 'full'),
    ('compressed', 1): ('refused[unevaluated:marginal]', 'full', 'lazy_full', 'pin', 'pinned', 'unpin', 'unpinned', 'joint',
        'set_repeats', 'joint', 'full', 'lazy_full', 'sensitivities', 'set_repeats', 'mixture', 'again', 'partial', 'full'),
    ('compressed', 2): ('refused[unevaluated:nni]', 'full', 'lazy_full', 'set_templates', 'pin', 'pinned', 'unpin', 'unpinned',
        'trials_built', 'set_repeats', 'simulate', 'refused[nothing_pending:collect]', 'async', 'nni',
        'refused[nothing_pending:collect]', 'set_repeats', 'mixture', 'again', 'partial', 'full'),
    ('compressed', 3): ('full', 'lazy_full', 'pin', 'pinned', 'unpin', 'unpinned', 'sensitivities', 'pin', 'refused[pin_active:trials]',
        'unpin', 'set_repeats', 'trials', 'pi_only', 'sample', 'set_repeats', 'mixture', 'again', 'partial', 'full'),
    ('compressed_nuc', 1): ('refused[unevaluated:marginal_leaves]', 'full', 'lazy_full', 'lazy_full', 'sample', 'set_templates', 'full',
        'lazy_full', 'derivatives_built', 'async', 'trials', 'refused[nothing_pending:collect]', 'pi_only', 'simulate', 'mixture',
        'again', 'partial', 'full'),
    ('compressed_nuc', 2): ('full', 'lazy_full', 'lazy_full', 'trials', 'pin', 'refused[pin_active:joint]', 'unpin', 'full',
        'lazy_full', 'simulate', 'full', 'lazy_full', 'derivatives', 'mixture', 'again', 'partial', 'full'),
    ('compressed_nuc', 3): ('refused[unevaluated:derivatives]', 'full', 'lazy_full', 'pi_only', 'trials', 'pi_only', 'marginal',
        'partial', 'trials', 'refused[nothing_pending:collect]', 'set_templates', 'derivatives_built', 'sensitivities', 'async',
        'collect', 'mixture', 'again', 'partial', 'full'),
    ('classes', 1): ('refused[unevaluated:sensitivities]', 'full', 'lazy_full', 'hmm_sites', 'derivatives', 'hmm_logl', 'class_partial',
        'partial', 'pin', 'pinned', 'unpin', 'unpinned', 'hmm_viterbi', 'refused[no_weights:derivatives]', 'catmix', 'again', 'partial',
        'full'),
    ('classes', 2): ('refused[unevaluated:trials]', 'full', 'lazy_full', 'hmm_sites', 'bc_build', 'hmm_logl', 'bc_eval', 'partial',
        'again', 'refused[no_weights:sensitivities]', 'async', 'hmm_viterbi', 'partial', 'hmm_viterbi', 'catmix', 'again', 'partial',
        'full'),
    ('classes', 3): ('refused[unevaluated:joint]', 'full', 'lazy_full', 'hmm_sites', 'async', 'hmm_logl', 'set_repeats', 'hmm_viterbi',
        'set_repeats', 'hmm_logl', 'refused[no_weights:trials]', 'pi_only', 'hmm_logl', 'catmix', 'again', 'partial', 'full'),
    ('classes20', 1): ('full', 'lazy_full', 'hmm_sites', 'full', 'lazy_full', 'hmm_logl', 'refused[no_weights:trials]', 'pin', 'pinned',
        'unpin', 'unpinned', 'hmm_logl', 'pi_only', 'hmm_viterbi', 'catmix', 'again', 'partial', 'full'),
    ('classes20', 2): ('refused[unevaluated:marginal]', 'full', 'lazy_full', 'hmm_sites', 'bc_build', 'hmm_viterbi', 'bc_eval',
        'partial', 'again', 'refused[no_weights:nni]', 'full', 'lazy_full', 'hmm_viterbi', 'catmix', 'again', 'partial', 'full'),
    ('classes20', 3): ('full', 'lazy_full', 'hmm_sites', 'partial', 'hmm_logl', 'refused[no_weights:trials]', 'joint', 'hmm_viterbi',
        'class_partial', 'partial', 'pin', 'refused[pin_active:nni]', 'unpin', 'catmix', 'again', 'partial', 'full'),
    ('shards', 1): ('refused[unevaluated:joint]', 'full', 'lazy_full', 'bc_build', 'sample', 'bc_eval', 'partial', 'bc_build',
        'sensitivities', 'bc_eval', 'partial', 'set_templates', 'bc_build', 'trials_built', 'bc_eval', 'partial', 'mixture', 'again',
        'partial', 'full'),
    ('shards', 2): ('refused[unevaluated:marginal]', 'full', 'lazy_full', 'bc_build', 'nni', 'bc_eval', 'partial', 'bc_build',
        'marginal_leaves', 'bc_eval', 'partial', 'refused[nothing_pending:collect]', 'pi_only', 'marginal_leaves', 'mixture', 'again',
        'partial', 'full'),
    ('shards', 3): ('full', 'lazy_full', 'set_templates', 'bc_build', 'derivatives_built', 'bc_eval', 'partial', 'async', 'joint',
        'refused[nothing_pending:collect]', 'pin', 'refused[pin_active:marginal]', 'unpin', 'async', 'collect', 'mixture', 'again',
        'partial', 'full'),
    ('nuc', 1): ('refused[unevaluated:joint]', 'full', 'lazy_full', 'set_templates', 'set_repeats', 'trials_built', 'set_repeats',
        'derivatives', 'pin', 'pinned', 'unpin', 'unpinned', 'nni', 'async', 'collect', 'mixture', 'again', 'partial', 'full'),
    ('nuc', 2): ('full', 'lazy_full', 'partial', 'nni', 'pin', 'refused[pin_active:marginal]', 'unpin', 'pi_only', 'sensitivities',
        'set_repeats', 'nni', 'async', 'simulate', 'refused[nothing_pending:collect]', 'set_repeats', 'mixture', 'again', 'partial',
        'full'),
    ('nuc', 3): ('full', 'lazy_full', 'async', 'sensitivities', 'pin', 'refused[pin_active:marginal]', 'unpin', 'full', 'lazy_full',
        'joint', 'set_templates', 'derivatives_built', 'trials_built', 'download', 'mixture', 'again', 'partial', 'full'),
    ('nucgen', 1): ('refused[unevaluated:joint]', 'full', 'lazy_full', 'lazy_full', 'marginal_leaves', 'async', 'marginal', 'trials',
        'nni', 'pin', 'refused[pin_active:joint]', 'unpin', 'set_templates', 'partial', 'trials_built', 'mixture', 'again', 'partial',
        'full'),
    ('nucgen', 2): ('full', 'lazy_full', 'pin', 'pinned', 'unpin', 'unpinned', 'trials', 'partial', 'joint', 'pi_only', 'joint', 'pin',
        'pinned', 'unpin', 'unpinned', 'simulate', 'mixture', 'again', 'partial', 'full'),
    ('nucgen', 3): ('full', 'lazy_full', 'set_repeats', 'sensitivities', 'partial', 'sensitivities', 'refused[nothing_pending:collect]',
        'async', 'derivatives', 'refused[nothing_pending:collect]', 'pin', 'pinned', 'unpin', 'unpinned', 'marginal', 'set_repeats',
        'mixture', 'again', 'partial', 'full'),
    ('chunks', 1): ('refused[unevaluated:sample]', 'full', 'lazy_full', 'bc_build', 'simulate', 'bc_eval', 'partial', 'set_templates',
        'pin', 'pinned', 'unpin', 'unpinned', 'derivatives_built', 'async', 'collect', 'mixture', 'again', 'partial', 'full'),
    ('chunks', 2): ('refused[unevaluated:joint]', 'full', 'lazy_full', 'partial', 'marginal', 'bc_build', 'trials', 'bc_eval',
        'partial', 'partial', 'marginal_leaves', 'set_templates', 'pi_only', 'trials_built', 'mixture', 'again', 'partial', 'full'),
    ('chunks', 3): ('refused[unevaluated:marginal_leaves]', 'full', 'lazy_full', 'bc_build', 'derivatives', 'bc_eval', 'partial',
        'set_repeats', 'marginal_leaves', 'set_templates', 'full', 'lazy_full', 'trials_built', 'set_repeats', 'mixture', 'again',
        'partial', 'full'),
    ('templates', 1): ('set_templates', 'built_full', 'built_lazy_full', 'update_templates', 'built_full', 'built_lazy_full',
        'gradient_built', 'pi_only', 'gradient', 'built_partial', 'gradient_built', 'refused[nothing_pending:collect]', 'pi_only',
        'gradient_built', 'built_partial', 'built_full'),
    ('templates', 2): ('refused[unevaluated:trials]', 'set_templates', 'built_full', 'built_lazy_full', 'bc_build', 'gradient_built',
        'bc_eval', 'built_partial', 'bc_build', 'gradient', 'bc_eval', 'built_partial', 'set_repeats', 'gradient_built', 'set_repeats',
        'built_partial', 'built_full'),
    ('templates', 3): ('set_templates', 'built_full', 'built_lazy_full', 'pin', 'pinned', 'unpin', 'unpinned', 'gradient_built', 'pin',
        'pinned', 'unpin', 'unpinned', 'gradient', 'async', 'collect', 'built_partial', 'built_full'),
}


if __name__ == "__main__":
    prof, which = sys.argv[1], sys.argv[2]
    which = which if which in FIXED else int(which)
    for i, st in enumerate(sequence(prof, which)):
        print(f"{i:2d}  {describe(st)}")
