"""Cases, call sequences and replayed references that hold the class-compressed form (repeats.hip) to tests/scalefree.py while the
2^64 rescale is active: partial updates, re-evaluations, downloads and rate classes on partitions whose per-class exponents
(``rep_cnt``) and hand-over exponents (``hand_cnt``) are non-zero and move from step to step.  (A download switches the partition
to its own tree by a persisting full pass there, and the compressed pass after it is promoted to a full one: the library has no
re-expansion of the class tables, so the download step holds those two passes and the downloaded values.)

Case: ``common.compressible_case(D, seed)`` without its ``Q``; every branch carries a row-stochastic matrix (``q_is_probability``),
at the start ``scalefree.near_identity`` with an eps drawn per branch from EPS_LIST.  One mismatch below a node at eps 1e-30 is
-69 in the logarithm: more than one step of 64 ln 2 = 44.4.

Sequence: a list of steps ``(what, update_nodes, q_nodes, matrices or None, pi, entry)``; ``replay`` keeps the current matrix of every
branch (and class) on the host and gives ``scalefree.prune`` of the current matrices as the reference of each step.  ``entry`` is
"evaluate", "download" (``download_partials``; nothing changes), "categories" (``evaluate_categories``) or ("class", c)
(``evaluate(cat=c)``).

Branch positions, by ``hip.plan_repeats`` at theta = 0.05 (at 0.9 every node but the root is compressed, since every pattern of
the case occurs twice: the same branches are then leaf and inner branches of tables, and (d), (e) hang below the lone trunk node):
  a  a leaf branch whose parent is compressed
  b  an internal branch whose node and parent are both compressed
  c  the branch above a topmost compressed node
  d  an internal trunk branch
  e  a leaf hanging off the trunk
  f  a leaf with ambiguity codes inside a compressed subtree
Among the branches of a kind the one is taken whose change between an ordinary matrix and a near-identity one at 1e-30 moves the
scale-free log-magnitude of its parent by more than 64 ln 2 on the most patterns (a conserved leaf moves none).

tests/test_compressed_cases_cpu.py checks, without a GPU, what makes the device tests meaningful.  The oracle
(oracle/hyphy_oracle.c) played over every step of every sequence stays within

    COMPRESSED_ORACLE_MAX_REL = 8.6e-16

of the replayed reference (8.561e-16 measured, the D = 61 rate classes at '3 classes partial (a, d)'; at most 6.3e-16 on every other
sequence; the constant is that rounded up), with -inf in the same places.  That is below scalefree.ORACLE_MAX_REL = 3.1e-15, so
scalefree.GPU_RTOL holds on these cases as it stands.
"""
import functools

import numpy as np

from tests import common, scalefree as sf

STATE_COUNTS = (4, 5, 17, 20, 33, 49, 61, 64)     # 1 - 4 row blocks, padded and exact, and the 4-state table kernel
WIDE = tuple(D for D in STATE_COUNTS if D != 4)
CLASS_D = (20, 61)
CLOSED_D = (20, 61)
EPS_LIST = (1e-30, 1e-30, 1e-20, 1e-10)
CLASS_EPS = (1e-2, 1e-12, 1e-30)
CLASS_WEIGHTS = np.array([0.5, 0.3, 0.2])
TINY = 1e-30
THETA_PLAN = 0.05
POSITIONS = "abcdef"
NONE = np.zeros(0, dtype=np.int64)
COMPRESSED_ORACLE_MAX_REL = 8.6e-16

# seed of compressible_case per state count: the first of 7400 + D + 100 k at which every position exists and the main sequence
# meets the conditions of tests/test_compressed_cases_cpu.py.  About one seed in a hundred does (one in a thousand at D = 20 and 64):
# what compresses at theta = 0.05 is nearly conserved, a conserved subtree carries no exponent, and a mismatch below a node moves
# its exponent by a whole step only while none of the node's other children can explain it more cheaply.
SEEDS = {4: 11004, 5: 19405, 17: 17017, 20: 119720, 33: 26533, 49: 16149, 61: 10361, 64: 165864}


def kinds_at(fx, theta):
    """Branch codes of each kind (a) - (f) under the compressed set of ``theta``."""
    from hyphy_amd import hip
    L, fp = int(fx["L"]), fx["flat_parents"]
    I = len(fp) - L
    _, comp, _ = hip.plan_repeats(fp, L, fx["leaf_codes"], theta)
    amb = (fx["leaf_codes"] < 0).any(axis=1)
    a = [l for l in range(L) if comp[fp[l]]]
    return {"a": a,
            "b": [L + i for i in range(I - 1) if comp[i] and comp[fp[L + i]]],
            "c": [L + i for i in range(I - 1) if comp[i] and not comp[fp[L + i]]],
            "d": [L + i for i in range(I - 1) if not comp[i]],
            "e": [l for l in range(L) if not comp[fp[l]]],
            "f": [l for l in a if amb[l]]}


def _prune(fx, P, pi=None, **kw):
    return sf.prune(fx["D"], fx["flat_parents"], fx["L"], fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], P,
                    fx["root_freqs"] if pi is None else pi, **kw)


def parent_log_mag(fx, ref, code, cls=None):
    """Log-magnitude [S] at the parent of branch ``code`` ([C, S] of a rate-class reference when no class is named)."""
    lm = ref["log_mag"] if cls is None else ref["log_mag"][cls]
    return lm[..., int(fx["flat_parents"][code]), :]


def moved(x, y):
    """(patterns whose value falls by more than 64 ln 2 from x to y, patterns whose value rises by more), over the patterns finite
    in both."""
    ok = np.isfinite(x) & np.isfinite(y)
    d = y[ok] - x[ok]
    return int(np.sum(d < -sf.LOG_SCALER)), int(np.sum(d > sf.LOG_SCALER))


def _trial_pair(fx, code):
    rng = np.random.default_rng([int(fx["seed"]), int(code), 1])
    D = int(fx["D"])
    return sf.ordinary(rng, 1, D)[0], sf.near_identity(rng, 1, D, TINY)[0]


def siblings(fx, code):
    fp = fx["flat_parents"]
    return [c for c in range(len(fp) - 1) if fp[c] == fp[code] and c != code]


def _score(fx, eps, code):
    """Patterns at which the parent's log-magnitude moves by more than one step when the branch goes from ordinary to 1e-30 while
    its siblings sit at 1e-30 (with a sibling at 1e-10 the other explanation of a mismatch costs 23: less than a step)."""
    e = eps.copy()
    e[siblings(fx, code)] = TINY
    P = sf.near_identity(np.random.default_rng([int(fx["seed"]), int(code), 2]), len(e), int(fx["D"]), e)
    lm = []
    for M in _trial_pair(fx, code):
        P[code] = M
        lm.append(parent_log_mag(fx, _prune(fx, P, conditionals=True), code))
    return sum(moved(lm[0], lm[1]))


def _positions(fx, eps):
    """Branch per position and its score; the siblings of a chosen branch get eps 1e-30 for good (``eps`` is changed in place)."""
    pos, score = {}, {}
    for k, cand in kinds_at(fx, THETA_PLAN).items():
        cand = [c for c in cand if c not in pos.values()]
        assert cand, (int(fx["D"]), int(fx["seed"]), f"no branch of kind ({k}): pick another seed")
        taken = set(pos.values())
        sc = [_score(fx, eps, c) * (1.0 if not taken & set(siblings(fx, c)) else 0.5) for c in cand]    # (rather not two of one family)
        best = int(np.argmax(sc))
        assert sc[best] > 0, (int(fx["D"]), int(fx["seed"]), f"no branch of kind ({k}) moves an exponent: pick another seed")
        pos[k], score[k] = int(cand[best]), int(_score(fx, eps, cand[best]))
        eps[[c for c in siblings(fx, cand[best]) if c not in taken]] = TINY
    return pos, score


def draw(rng, fx):
    """New matrices for every branch at the case's eps per branch."""
    return sf.near_identity(rng, len(fx["eps"]), int(fx["D"]), fx["eps"])


@functools.lru_cache(maxsize=None)
def case(D, seed=None):
    """The case at ``D`` states: compressible_case's keys without "Q", plus "seed", "eps" (per branch, drawn from EPS_LIST; 1e-30 on
    the siblings of the positions), "P" (the starting matrices), "pos" (branch code per position) and "pos_score"."""
    seed = SEEDS[D] if seed is None else seed
    fx = common.compressible_case(D, seed)
    del fx["Q"]
    fx["seed"] = seed
    fx["name"] = f"compressed_D{D}"
    B = len(fx["flat_parents"]) - 1
    rng = np.random.default_rng([seed, 2])
    fx["eps"] = rng.choice(EPS_LIST, size=B)
    fx["pos"], fx["pos_score"] = _positions(fx, fx["eps"])
    fx["P"] = draw(rng, fx)
    return fx


def _nodes(fx):
    return np.arange(len(fx["flat_parents"]) - 1, dtype=np.int64)


class _Builder:
    """Builds a sequence while keeping the current matrices, so that a kind may refer to the branch's current matrix."""

    def __init__(self, fx, seed_tag, C=None):
        self.fx, self.D, self.C = fx, int(fx["D"]), C
        self.rng = np.random.default_rng([int(fx["seed"]), seed_tag])
        self.cur = None
        self.pi = fx["root_freqs"]
        self.steps = []

    def matrix(self, kind, code, cls=None):
        D, rng = self.D, self.rng
        cur = self.cur[code] if cls is None else self.cur[cls][code]
        if kind == "tiny":
            return sf.near_identity(rng, 1, D, TINY)[0]
        if kind == "ord":
            return sf.ordinary(rng, 1, D)[0]
        if kind == "eye":
            return np.eye(D)
        if kind == "bz":
            return sf._block_zero(cur[None], D)[0]
        if kind == "bz_tiny":
            return sf._block_zero(sf.near_identity(rng, 1, D, TINY), D)[0]
        if kind == "bz_ord":
            return sf._block_zero(sf.ordinary(rng, 1, D), D)[0]
        return sf.near_identity(rng, 1, D, float(kind), spread=D * float(kind) < 0.3)[0]     # an eps

    def full(self, what, P, entry="evaluate"):
        self.cur = P.copy()
        n = _nodes(self.fx)
        self.steps.append((what, n, n, P.copy(), self.pi, entry))

    def partial(self, what, change, entry="evaluate"):
        """``change``: {branch code: kind} — or {branch code: (kind per class)} in a rate-class sequence."""
        codes = np.array(sorted(change), dtype=np.int64)
        if self.C is None or isinstance(entry, tuple):
            cls = entry[1] if isinstance(entry, tuple) else None
            M = np.stack([self.matrix(change[int(c)], int(c), cls) for c in codes])
            (self.cur if cls is None else self.cur[cls])[codes] = M
        else:
            M = np.stack([np.stack([self.matrix(change[int(c)][k], int(c), k) for c in codes]) for k in range(self.C)])
            self.cur[:, codes] = M
        label = ", ".join(f"{int(c)}:{change[int(c)]}" for c in codes)
        self.steps.append((f"{what} [{label}]", codes, codes, M, self.pi, entry))

    def again(self, what, pi=None, entry="evaluate"):
        if pi is not None:
            self.pi = pi
        self.steps.append((what, NONE, NONE, None, self.pi, entry))


@functools.lru_cache(maxsize=None)
def main_sequence(D):
    """The eleven kinds of step of the main sequence, in order (the numbers in the labels)."""
    fx = case(D)
    p = fx["pos"]
    a, b, c, d, e, f = (p[k] for k in POSITIONS)
    B = len(fx["flat_parents"]) - 1
    sb = _Builder(fx, 3)
    rng = sb.rng
    sb.full("1 full (persists)", fx["P"])
    P = draw(rng, fx)
    for code, kind in ((a, "tiny"), (c, "tiny"), (e, "tiny"), (b, "ord"), (d, "ord"), (f, "ord")):
        sb.cur = P
        P[code] = sb.matrix(kind, code)
    sb.full("2 full (lazy)", P)
    # 3: one position at a time; a, c, e fall back to ordinary (exponents above them drop), b, d, f go to 1e-30 (they rise)
    for k, kind in zip(POSITIONS, ("ord", "tiny", "ord", "tiny", "ord", "tiny")):
        sb.partial(f"3 partial ({k})", {p[k]: kind})
    # 4: two and three positions at once, each the other way round
    sb.partial("4 partial (a, d)", {a: "tiny", d: "ord"})
    sb.partial("4 partial (b, c, f)", {b: "ord", c: "tiny", f: "ord"})
    # 5: the same dirty set twice in a row (a ring-slot hit)
    sb.partial("5 partial (e)", {e: "tiny"})
    sb.partial("5 partial (e) again", {e: "ord"})
    # 6: seven dirty sets, then the first again (four ring slots: evicted and rebuilt)
    sb.partial("6 partial (a)", {a: "ord"})
    sb.partial("6 partial (b)", {b: "tiny"})
    sb.partial("6 partial (c)", {c: "ord"})
    sb.partial("6 partial (f)", {f: "bz"})
    sb.partial("6 partial (d)", {d: "tiny"})
    sb.partial("6 partial (e)", {e: "eye"})
    sb.partial("6 partial (a, b)", {a: "tiny", b: "ord"})
    sb.partial("6 partial (a) after eviction", {a: "ord"})
    sb.again("7 again")
    pi2 = rng.random(D) + 0.05
    sb.again("8 root frequencies", pi2 / pi2.sum())
    sb.again("9 download", entry="download")
    sb.partial("9 partial (c, e) after the download", {c: "tiny", e: "ord"})
    sb.full("10 full", draw(rng, fx))
    sb.full("11 full (lazy)", draw(rng, fx))
    return tuple(sb.steps)


def _revived(fx, P, code):
    """Patterns impossible under ``P`` that an ordinary matrix on ``code`` makes possible."""
    Q = P.copy()
    Q[code] = _trial_pair(fx, code)[0]
    return int(np.sum(np.isneginf(_prune(fx, P)["site_logl"]) & np.isfinite(_prune(fx, Q)["site_logl"])))


@functools.lru_cache(maxsize=None)
def closed_branches(D):
    """(x, z, y) of the closed sequence and the eps per branch it draws its matrices at: the three branches, no two of one family,
    whose opening revives the most patterns among those that also move the exponent of their parent (``_score``); they and their
    siblings sit at 1e-30, so that opening and closing them moves exponents by whole steps at the patterns that stay possible.
    (Variable leaves: at theta = 0.05 they hang off the trunk or sit in small tables, at 0.9 all are inside tables.)"""
    fx = case(D)
    P = sf._block_zero(fx["P"], D)
    B = len(fx["flat_parents"]) - 1
    rank = sorted(((_revived(fx, P, c), c) for c in range(B)), key=lambda t: (-t[0], t[1]))
    chosen = []
    for alive, c in rank:
        if alive > 0 and _score(fx, fx["eps"], c) > 0 and not set(siblings(fx, c)) & set(chosen):
            chosen.append(c)
        if len(chosen) == 3:
            break
    assert len(chosen) == 3, (D, chosen, "fewer than three branches whose opening revives a pattern and moves an exponent")
    eps = fx["eps"].copy()
    for c in chosen:
        eps[[c] + siblings(fx, c)] = TINY
    x, z, y = chosen
    return x, z, y, eps


@functools.lru_cache(maxsize=None)
def closed_sequence(D):
    """Every matrix ``_block_zero``'d: the last state (in the case's palette) cannot be left or reached, so patterns that hold it at
    some leaves only are impossible.  One branch is opened (some become possible), closed again, opened together with others, and one
    of those closed again.  Every step also takes its branch between 1e-30 and ordinary: the exponents of the patterns that stay
    possible move as well."""
    fx = case(D)
    x, z, y, eps = closed_branches(D)
    D_ = int(fx["D"])
    sb = _Builder(fx, 4)
    rng = sb.rng

    def closed():
        return sf._block_zero(sf.near_identity(rng, len(eps), D_, eps), D_)

    sb.full("1 full (persists), closed", closed())
    sb.full("2 full (lazy), closed", closed())
    sb.partial("3 open x", {x: "ord"})
    sb.partial("4 y stays closed", {y: "bz_ord"})
    sb.partial("5 close x", {x: "bz_tiny"})
    sb.again("6 again")
    sb.partial("7 open x, y, z", {x: "ord", y: "tiny", z: "ord"})
    sb.partial("8 close z", {z: "bz_tiny"})
    sb.full("9 full, closed", closed())
    sb.full("10 full (lazy), closed", closed())
    return tuple(sb.steps)


def _class_matrices(rng, B, D):
    return np.stack([sf.near_identity(rng, B, D, e, spread=D * e < 0.3) for e in CLASS_EPS])


@functools.lru_cache(maxsize=None)
def class_sequence(D):
    """Three rate classes with off-diagonals 1e-2 / 1e-12 / 1e-30 (scalefree's ``classes_*``): all classes in one call — full, lazy,
    three partial batches that give every class a matrix — then one partial ``evaluate(cat=c)`` per class and two last full passes."""
    fx = case(D)
    p = fx["pos"]
    a, b, c, d, e, f = (p[k] for k in POSITIONS)
    B = len(fx["flat_parents"]) - 1
    sb = _Builder(fx, 5, C=3)
    rng = sb.rng
    lo, mid, hi = (str(x) for x in CLASS_EPS)
    sb.full("1 classes full (persists)", _class_matrices(rng, B, D), "categories")
    sb.full("2 classes full (lazy)", _class_matrices(rng, B, D), "categories")
    sb.partial("3 classes partial (a, d)", {a: (hi, lo, "ord"), d: (hi, "ord", "ord")}, "categories")
    sb.partial("4 classes partial (b, c, f)", {b: (mid, hi, "ord"), c: (hi, lo, "ord"), f: ("tiny", lo, "ord")}, "categories")
    sb.partial("5 classes partial (a, e)", {a: (lo, hi, "tiny"), e: (hi, mid, "ord")}, "categories")
    # (a class at 1e-2 or 1e-12 moves by a step only where the siblings cannot explain the mismatch instead: they change too)
    sb.partial("6 class 0 alone (a and its siblings)", dict.fromkeys([a] + siblings(fx, a), "tiny"), ("class", 0))
    sb.partial("7 class 1 alone (c and its siblings)", dict.fromkeys([c] + siblings(fx, c), "tiny"), ("class", 1))
    sb.partial("8 class 2 alone (d, f)", {d: "tiny", f: "tiny"}, ("class", 2))
    sb.full("9 classes full", _class_matrices(rng, B, D), "categories")
    sb.full("10 classes full (lazy)", _class_matrices(rng, B, D), "categories")
    return tuple(sb.steps)


SEQUENCES = {"main": main_sequence, "closed": closed_sequence, "classes": class_sequence}


def sequence(D, which):
    return SEQUENCES[which](D)


@functools.lru_cache(maxsize=None)
def replay(D, which):
    """Per step of the sequence a dict: "ref" (scalefree.prune of the current matrices, conditionals included), "P" (the current
    matrices), "prev" (the matrices before the step), "changed" (branch codes), "cls" (the class of an ("class", c) step)."""
    fx = case(D)
    out, cur = [], None
    for what, un, qn, M, pi, entry in sequence(D, which):
        prev = None if cur is None else cur.copy()
        cls = entry[1] if isinstance(entry, tuple) else None
        if M is not None:
            if len(qn) == len(fx["flat_parents"]) - 1 and cls is None:
                cur = M.copy()
            elif cls is not None:
                cur[cls][qn] = M
            elif cur.ndim == 4:
                cur[:, qn] = M
            else:
                cur[qn] = M
        ref = _prune(fx, cur, pi, weights=CLASS_WEIGHTS if cur.ndim == 4 else None, conditionals=True)
        out.append(dict(what=what, ref=ref, P=cur.copy(), prev=prev, changed=[int(c) for c in qn] if M is not None else [], cls=cls,
                        pi=pi, entry=entry, partial=M is not None and len(qn) < len(fx["flat_parents"]) - 1))
    return tuple(out)


def step_reference(fx, rec):
    """(per-pattern log-likelihood, total) a step is held to: the mixture's, or the one class's of a ("class", c) step."""
    ref = rec["ref"]
    if rec["cls"] is None:
        return ref["site_logl"], ref["logl"]
    want = ref["class_site_logl"][rec["cls"]]
    return want, float(np.sum(want * fx["pattern_freq"]))
