"""Cases and references for the template path (hyphy_hip_set_q_templates / _update_q_templates / _build_q and every evaluation that
consumes what they stage): tests/test_template_cases_cpu.py admits the cases, tests/test_gpu_templates.py runs them on the device.

A case is a tree, patterns, pi and a SEQUENCE of steps.  A step is a dict:

  t        index into the case's template values T[0], T[1], ... sent before the step's build_q (None: no template call)
  rows     {branch (node code): coefficient row [K]} — [C, K] per branch in a "cat" case (one row per rate class), [M, K] in a "mix"
           case (one row per mixture component); only these branches are rebuilt
  update   the update list (node codes)
  entry    the entry point the device test uses ("built", "device", "mixture", "categories", "none": an evaluation without matrices)
  cls      the rate class the step evaluates ("percls" cases: one template set per class, the adapter's use); pi: index into case["pis"]

``replay`` plays the sequence on the host.  Per branch (and class) it keeps the matrix LAST BUILT for it: expm_ref.reference(Q) with
Q = sum_k c_k offdiag(T_k), the sum formed in extended precision, the diagonal minus math.fsum of the row; a zero row is the exact
identity, a mixture is sum_m w_m reference(Q_m).  A branch that a step does not rebuild keeps its matrix whatever happened to the
templates since.  Per-pattern log-likelihoods and totals are scalefree.prune's ([C, B, D, D] with weights for the rate classes).
The templates arrive WITH diagonals (minus the row sum, as the host adapter's solved M_k do); the reference ignores them, as
include/hyphy_hip.h says the library does.

``replay(..., mistake=(kind, i))`` gives step i under one of the mistakes the sequence is there to catch (MISTAKES): the previous
template values for the rebuilt branches, the new values also for the branches NOT rebuilt, the previous coefficient rows, the
caller's diagonal added into Q, a template missing.  tests/test_template_cases_cpu.py requires each to move the total by 1000 times
the allowance of tests/hold.py.

Largest deviation of the project's oracle (oracle.expm + OraclePartition on the same sequences) from these references, as a fraction
of that allowance (scalefree.GPU_RTOL |ref| + 1e-9 per pattern), over every step of every case, measured by
test_template_cases_cpu.py::test_oracle_within_half_the_allowance:

    ORACLE_MAX_RATIO = 4e-4

(3.2e-4 measured, step 0 of mixture_D61_K4; the constant is that rounded up.)  It has to stay below one half: the allowance is
reachable by correct double-precision arithmetic with room to spare.
"""
import functools
import math

import numpy as np

from tests import expm_ref as er
from tests import scalefree as sf
from tests.expm_child import path_above

ORACLE_MAX_RATIO = 4e-4
MISTAKES = ("old_templates", "new_everywhere", "old_rows", "diagonal", "missing_template")
STATE_COUNTS = (4, 20, 48, 49, 61, 64)
S_DEFAULT = 40
N_VALUES = 9                     # T[0] .. T[8]: the host-ahead sequences take nine


# ---- ingredients --------------------------------------------------------------------------------------------------------------------

def set_diagonal(T, kind):
    """The same off-diagonals with diagonal 0 ("zero"), minus the row sum ("rowsum") or +7 ("seven")."""
    T = np.array(T, dtype=np.float64)
    idx = np.arange(T.shape[-1])
    T[..., idx, idx] = 0.0
    if kind == "rowsum":
        T[..., idx, idx] = -T.sum(axis=-1)
    elif kind == "seven":
        T[..., idx, idx] = 7.0
    else:
        assert kind == "zero"
    return np.ascontiguousarray(T)


def template_values(D, K, seed, n=N_VALUES):
    """T[0] .. T[n-1], each [K, D, D]: not reversible, off-diagonals >= 0; entry (i, j) belongs to template (i + 2 j) mod (K + 1),
    and to every template where that is K (disjoint and overlapping supports).  T[v + 1] is T[v] with a third of the entries of
    template v mod K multiplied by factors in [1.25, 3]."""
    rng = np.random.default_rng(seed)
    i, j = np.indices((D, D))
    cls = (i + 2 * j) % (K + 1)
    T = np.stack([np.where((cls == k) | (cls == K), rng.uniform(0.2, 1.0, size=(D, D)), 0.0) for k in range(K)]) * (2.0 / D)
    out = [set_diagonal(T, "rowsum")]
    for v in range(n - 1):
        T = out[-1].copy()
        k = v % K
        f = np.where(rng.random((D, D)) < 1.0 / 3.0, rng.uniform(1.25, 3.0, size=(D, D)), 1.0)
        r, c = np.nonzero(T[k] * (i != j))
        f[r[0], c[0]] = f[r[-1], c[-1]] = 2.125           # (never an empty change)
        T[k] *= f
        out.append(set_diagonal(T, "rowsum"))
    for T in out:
        T.setflags(write=False)
    return out


def tree(kind):
    if kind == "bal8":
        return sf.balanced_tree(2, 3)
    return sf.ladder_tree({"lad3": 3, "lad5": 5, "lad40": 40, "lad70": 70}[kind])


def live_branches(kind, fp, L):
    """The branches that carry non-zero rows: all, or on the long ladders six (both ends and the middle, leaves and internals)."""
    B = len(fp) - 1
    if kind in ("lad40", "lad70"):
        return [0, L // 2, L - 1, L + 0, L + L // 2, 2 * L - 3]
    return list(range(B))


def _patterns(rng, fp, L, D, S, live):
    """Leaf codes [L, S]: leaves joined by branches that stay the identity show one state (else the pattern is impossible); leaf 0
    (its branch is live) shows the case's ambiguity row at every fifth pattern."""
    B = len(fp) - 1
    comp = list(range(B + 1))

    def find(x):
        while comp[x] != x:
            comp[x] = comp[comp[x]]
            x = comp[x]
        return x
    for b in range(B):
        if b not in live:
            comp[find(b)] = find(L + int(fp[b]))
    roots = sorted({find(x) for x in range(B + 1)})
    state = rng.integers(0, D, size=(len(roots), S))
    state[:, ::7] = rng.integers(0, D, size=S)[None, ::7]       # conserved columns
    codes = np.stack([state[roots.index(find(leaf))] for leaf in range(L)]).astype(np.int64)
    codes[0, 2::5] = -1
    return codes


def coefficient_rows(rng, branches, shape):
    """Rows in (0.03, 0.5), no powers of two."""
    return {int(b): rng.uniform(0.03, 0.5, size=shape) for b in branches}


def _base(name, kind, D, K, tree_kind, seed, S=S_DEFAULT, C=1, M=1):
    rng = np.random.default_rng(seed)
    fp, L = tree(tree_kind)
    live = live_branches(tree_kind, fp, L)
    ambig = (rng.random((1, D)) < 0.5).astype(np.float64)
    ambig[0, :2] = 1.0
    pis = []
    for _ in range(2):
        pi = rng.random(D) + 0.1
        pis.append(pi / pi.sum())
    cs = dict(name=name, kind=kind, D=D, K=K, C=C, M=M, tree=tree_kind, flat_parents=fp, L=int(L), B=len(fp) - 1, live=live,
              leaf_codes=_patterns(rng, fp, L, D, S, live), ambig=ambig, pattern_freq=rng.integers(1, 4, size=S).astype(np.int64),
              pis=pis, T=template_values(D, K, seed + 1), steps=[], rng=rng)
    if kind == "cat":
        cs["weights"] = np.array([0.5, 0.3, 0.2])[:C] / np.array([0.5, 0.3, 0.2])[:C].sum()
        cs["rates"] = np.array([0.37, 1.0, 2.3])[:C]
    if kind == "mix":
        w = rng.random((cs["B"], M)) + 0.2
        cs["mixw"] = w / w.sum(axis=1, keepdims=True)
    return cs


def _row_shape(cs):
    return {"plain": (cs["K"],), "percls": (cs["K"],), "cat": (cs["K"],), "mix": (cs["M"], cs["K"])}[cs["kind"]]


def _rows(cs, branches):
    rows = coefficient_rows(cs["rng"], [b for b in branches if b in cs["live"]], _row_shape(cs))
    if cs["kind"] == "cat":            # one row per class: the class rate times the branch's row
        rows = {b: cs["rates"][:, None] * r[None, :] for b, r in rows.items()}
    for b in branches:
        if b not in cs["live"]:
            rows[int(b)] = np.zeros(_row_shape(cs) if cs["kind"] != "cat" else (cs["C"], cs["K"]))
    return rows


def _step(cs, t, branches, update=None, entry=None, cls=0, pi=0):
    all_nodes = np.arange(cs["B"], dtype=np.int64)
    if update is None:
        update = all_nodes
    entry = entry or {"plain": "built", "percls": "built", "cat": "categories", "mix": "mixture"}[cs["kind"]]
    cs["steps"].append(dict(t=t, rows=_rows(cs, branches), update=np.asarray(update, dtype=np.int64), entry=entry, cls=cls, pi=pi))


def _paths(cs, branches):
    out = set()
    for b in branches:
        out |= set(int(x) for x in path_above(cs["flat_parents"], cs["L"], b))
    return np.array(sorted(out), dtype=np.int64)


# ---- the case list ------------------------------------------------------------------------------------------------------------------

# (D, K) of the consumer cases: every D, and every K at 20 and 61 states
# (49, 2): the site fits take at most four templates, and 49 is the smallest state count on the padded image
CONSUMER_GRID = ((4, 2), (20, 1), (20, 2), (20, 4), (20, 5), (48, 4), (49, 5), (61, 1), (61, 2), (61, 4), (61, 5), (64, 2), (49, 2))
MIXTURE_GRID = ((4, 4), (20, 2), (48, 1), (49, 2), (61, 4), (64, 5))      # mixtures (M = 3)
CLASS_GRID = MIXTURE_GRID[1:]                                            # rate classes (C = 3): evaluate_categories_built starts at 5 states
PARTIAL_STATES = (4, 20, 61, 64)
RESIDENT_STATES = (4, 20, 61)
AHEAD = (("ahead_inline_D61_K2", "plain", 61, 2, "bal8", "device"), ("ahead_ring_D20_K3", "plain", 20, 3, "lad70", "device"),
         ("ahead_ring_D49_K3", "plain", 49, 3, "lad70", "device"), ("ahead_fold_D4_K2", "plain", 4, 2, "lad5", "device"),
         ("ahead_mix_D20_K2", "mix", 20, 2, "bal8", "mixture"))


def _enumerate():
    seed = 5000

    def nxt():
        nonlocal seed
        seed += 10
        return seed
    # 1. set(T0), full pass, update(T1), build_q, consumer
    for D, K in CONSUMER_GRID:
        cs = _base(f"consumer_D{D}_K{K}", "plain", D, K, "bal8", 4900 if (D, K) == (49, 2) else nxt())   # (a seed of its own: the others stay)
        _step(cs, 0, range(cs["B"]))
        _step(cs, 1, range(cs["B"]))
        yield cs
    for D, K in MIXTURE_GRID:
        seed_cat = nxt()
        if (D, K) in CLASS_GRID:
            cs = _base(f"classes_D{D}_K{K}", "cat", D, K, "bal8", seed_cat, C=3)
            _step(cs, 0, range(cs["B"]))
            _step(cs, 1, range(cs["B"]))
            yield cs
        cs = _base(f"mixture_D{D}_K{K}", "mix", D, K, "lad5", nxt(), M=3)
        _step(cs, 0, range(cs["B"]))
        _step(cs, 1, range(cs["B"]))
        yield cs
    # 2. partial rebuilds: T0 full; T1, a leaf branch and an internal one; T2, one other branch; a full rebuild under T2
    for D in PARTIAL_STATES:
        cs = _base(f"partial_D{D}_K2", "plain", D, 2, "bal8", nxt())
        L = cs["L"]
        _step(cs, 0, range(cs["B"]))
        _step(cs, 1, (3, L + 1), _paths(cs, (3, L + 1)))
        _step(cs, 2, (L + 4,), _paths(cs, (L + 4,)))
        _step(cs, None, range(cs["B"]))
        yield cs
    # ... on a 40-leaf ladder with pi changed in the middle (the device test runs it re-rooted: branches L + 20 and 2 L - 3 lie
    # between the given root and the ladder's middle, leaf 0 does not; the 70-leaf ladder's path exceeds what a re-rooted schedule takes)
    cs = _base("partial_reroot_D61_K2", "plain", 61, 2, "lad40", nxt())
    L = cs["L"]
    _step(cs, 0, range(cs["B"]))
    _step(cs, None, (), entry="none")                               # (a full pass behind a full pass: the re-rooted form is a steady-state one)
    _step(cs, 1, (0, 2 * L - 3), _paths(cs, (0, 2 * L - 3)))
    _step(cs, None, (), entry="none")
    _step(cs, None, (), entry="none")                               # (re-rooted again: the twin of 2 L - 3 had to follow)
    _step(cs, 2, (L + L // 2,), _paths(cs, (L + L // 2,)), pi=1)
    _step(cs, None, (), entry="none", pi=1)
    _step(cs, None, (), entry="none", pi=1)
    _step(cs, None, range(cs["B"]), pi=1)
    _step(cs, None, (), entry="none", pi=1)
    yield cs
    # ... with 70 patterns (the device test forces three shards)
    cs = _base("partial_shards_D20_K4", "plain", 20, 4, "bal8", nxt(), S=70)
    L = cs["L"]
    _step(cs, 0, range(cs["B"]))
    _step(cs, 1, (5, L + 2), _paths(cs, (5, L + 2)))
    _step(cs, 2, (L + 5,), _paths(cs, (L + 5,)))
    _step(cs, None, range(cs["B"]))
    yield cs
    # ... one template set per class: class 0 under T0, class 1 under T1, then one branch of class 0 under T0 again
    for D in (20, 61):
        cs = _base(f"perclass_D{D}_K2", "percls", D, 2, "bal8", nxt(), C=2)
        _step(cs, 0, range(cs["B"]), cls=0)
        _step(cs, 1, range(cs["B"]), cls=1)
        _step(cs, 0, (2,), _paths(cs, (2,)), cls=0)
        yield cs
    # 3. resident matrices: two full passes (the second without matrices); the device test then updates WITHOUT build_q
    for D in RESIDENT_STATES:
        cs = _base(f"resident_D{D}_K2", "plain", D, 2, "bal8", nxt())
        _step(cs, 0, range(cs["B"]))
        _step(cs, None, (), entry="none")
        yield cs
    # the hand-sized case of the mpmath check (not run on the device)
    cs = _base("hand_D2_K2", "plain", 2, 2, "lad3", nxt(), S=8)
    _step(cs, 0, range(cs["B"]))
    _step(cs, 1, (1, cs["L"]), _paths(cs, (1, cs["L"])))
    yield cs
    # 6. nine steps of update + build_q + evaluation, queued without a wait
    for name, kind, D, K, tk, entry in AHEAD:
        cs = _base(name, kind, D, K, tk, nxt(), M=3 if kind == "mix" else 1)
        for v in range(N_VALUES):
            _step(cs, v, range(cs["B"]), entry=entry)
        yield cs


@functools.lru_cache(maxsize=None)
def _cases():
    cs = list(_enumerate())
    for c in cs:
        del c["rng"]
    assert len({c["name"] for c in cs}) == len(cs)
    return tuple(cs)


def cases():
    return list(_cases())


def cases_by_name():
    return {c["name"]: c for c in _cases()}


# ---- references ---------------------------------------------------------------------------------------------------------------------

def rate_matrix(T, row, add_diagonal=False):
    """sum_k c_k offdiag(T_k) in extended precision, diagonal minus math.fsum of the row (``add_diagonal``: the mistake of adding the
    caller's diagonal sum_k c_k T_k[i, i] on top)."""
    T = np.asarray(T, dtype=np.float64)
    D = T.shape[1]
    Q = np.asarray(np.tensordot(np.asarray(row, dtype=np.longdouble), T.astype(np.longdouble), axes=(0, 0)), dtype=np.float64)
    extra = Q[np.arange(D), np.arange(D)].copy()
    for i in range(D):
        Q[i, i] = 0.0
        Q[i, i] = -math.fsum(Q[i])
        if add_diagonal:
            Q[i, i] += extra[i]
    return Q


def _plain_expm(Q):
    """exp(Q) by scaling, a 30-term Taylor series and squaring in float64: for the mistake whose Q is no rate matrix (accurate to
    ~1e-13, against a required gap of 1000 allowances)."""
    nm = float(np.abs(Q).sum(axis=1).max())
    s = max(0, int(math.ceil(math.log2(nm))) + 2) if nm > 0 else 0
    A = Q / 2.0 ** s
    E = term = np.eye(Q.shape[0])
    for j in range(1, 31):
        term = term @ A / j
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


class Reference:
    """expm_ref.reference and scalefree.prune."""
    name = "reference"

    @staticmethod
    def matrix(Q):
        return er.reference(Q)

    @staticmethod
    def sites(cs, P, pi, weights=None):
        r = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, pi, weights=weights)
        return r["site_logl"]


@functools.lru_cache(maxsize=None)
def _matrix(backend, name, t, row_bytes, shape, add_diagonal, w_bytes):
    cs = cases_by_name()[name]
    rows = np.frombuffer(row_bytes, dtype=np.float64).reshape(shape)
    if not rows.any():
        return np.eye(cs["D"])
    if rows.ndim == 1:
        rows, w = rows[None], np.ones(1)
    else:
        w = np.frombuffer(w_bytes, dtype=np.float64)
    P = 0.0
    for wm, row in zip(w, rows):
        Q = rate_matrix(cs["T"][t], row, add_diagonal)
        P = P + wm * (_plain_expm(Q) if add_diagonal else backend.matrix(Q))
    return P


def replay(name, backend=Reference, mistake=None):
    """[{"site_logl", "logl", "P"}] per step (``mistake`` = (kind, i): steps 0 .. i, step i under that mistake; None where the mistake
    does not apply to step i)."""
    cs = cases_by_name()[name]
    D, B, K = cs["D"], cs["B"], cs["K"]
    ncls = cs["C"] if cs["kind"] in ("cat", "percls") else 1
    P = np.tile(np.eye(D), (ncls, B, 1, 1))
    last = {}                                  # (class, branch) -> rows as last built
    built_t = {}                               # (class, branch) -> the template values they were built from
    t_cur = None
    out = []
    for i, st in enumerate(cs["steps"]):
        bad = mistake[0] if mistake is not None and mistake[1] == i else None
        t_before = t_cur
        if st["t"] is not None:
            t_cur = st["t"]
        changed = t_before is not None and t_cur != t_before
        live_rows = {b: r for b, r in st["rows"].items() if r.any()}
        if bad == "old_templates" and not (changed and live_rows):
            return None
        if bad in ("diagonal", "old_rows") and not live_rows:
            return None
        if bad == "missing_template" and not (K >= 2 and live_rows):
            return None
        for b, rows in st["rows"].items():
            per_class = rows if cs["kind"] == "cat" else [rows]
            for c, r in enumerate(per_class):
                c = st["cls"] if cs["kind"] == "percls" else c
                use = np.ascontiguousarray(r, dtype=np.float64)
                if bad == "old_rows":
                    use = np.ascontiguousarray(last.get((c, b), np.zeros_like(use)))
                if bad == "missing_template":
                    use = use.copy()
                    use[..., K - 1] = 0.0
                w = cs["mixw"][b] if cs["kind"] == "mix" else np.ones(1)
                P[c, b] = _matrix(backend, name, t_before if bad == "old_templates" else t_cur, use.tobytes(), use.shape,
                                  bad == "diagonal", np.ascontiguousarray(w).tobytes())
                last[(c, b)] = np.ascontiguousarray(r, dtype=np.float64)
                built_t[(c, b)] = t_cur
        if bad == "new_everywhere":
            others = [(c, b) for (c, b), r in last.items() if b not in st["rows"] and r.any() and built_t[(c, b)] != t_cur
                      and (cs["kind"] != "percls" or c == st["cls"])]
            if not (changed and others):
                return None
            for c, b in others:
                w = cs["mixw"][b] if cs["kind"] == "mix" else np.ones(1)
                P[c, b] = _matrix(backend, name, t_cur, last[(c, b)].tobytes(), last[(c, b)].shape, False, np.ascontiguousarray(w).tobytes())
        pi = cs["pis"][st["pi"]]
        if mistake is not None and i < mistake[1]:
            out.append(None)
            continue
        if cs["kind"] == "cat":
            site = backend.sites(cs, P, pi, cs["weights"])
        else:
            site = backend.sites(cs, P[st["cls"] if cs["kind"] == "percls" else 0], pi)
        out.append(dict(site_logl=site, logl=float(np.sum(site * cs["pattern_freq"])), P=P.copy()))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The references of every step of a case, computed once per process and shared (read-only)."""
    out = replay(name)
    for r in out:
        r["site_logl"].setflags(write=False)
        r["P"].setflags(write=False)
    return tuple(out)


def coefficients(cs, step):
    """(q_nodes, coefficient rows as build_q takes them) of a step: one row per branch; class-major [C * n_q, K] for rate classes;
    [n_q, M, K] for a mixture."""
    qn = np.array(sorted(step["rows"]), dtype=np.int64)
    if not len(qn):
        return qn, None
    rows = np.stack([step["rows"][int(b)] for b in qn])
    if cs["kind"] == "cat":
        rows = np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(cs["C"] * len(qn), cs["K"])
    return qn, np.ascontiguousarray(rows)
