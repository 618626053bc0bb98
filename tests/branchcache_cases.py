"""Cases for the branch cache (hyphy_hip_branch_cache_build / _evaluate): a fixed, named, seeded list built from tests/scalefree.py's
builders, the trial matrices of every branch under test, and the references.

The reference for "branch cache at ``node`` with trial matrix M" is ``scalefree.prune`` with ``P[node] = M`` (``reference``).
``rerooted_site_logl`` restates what the library computes instead (include/hyphy_hip.h, "branch cache"; prune.hip above
transpose_frag_kernel): the tree re-rooted at the branch's parent, L_s = sum_i A_s[i] sum_j M[i][j] B_s[j], with the edges between the
old root and the parent walked through the transposed matrices and pi on the edge that leaves the old root.  It exists so that the
CPU tests can show that these cases tell a missing transposition or a misplaced pi from the right answer (its two switches).

Every matrix is row-stochastic and none is reversible (``scalefree.ordinary`` / ``near_identity`` draw every entry on its own);
``root_freqs`` is random: not the stationary distribution of anything and not uniform.

Patterns follow scalefree's ``mixed_*`` recipe, so that every 16 patterns hold conserved, conflicting, ambiguous and impossible ones
side by side; S is never a multiple of 16 and the frequencies are 1 .. 3.  Within every 16 patterns:
  * 2, 6, 10, 14 carry ambiguity codes: leaf l of the case's ambiguous leaves has one at pattern 2 + 4 (l mod 4) — the tile of a cached
    leaf branch then mixes coded and ambiguous lanes, and the leaf's siblings carry codes too; the other leaves have none anywhere;
  * 5 is impossible at build time in the cases of odd seed (in the others it is one more conflicting pattern: with an impossible
    pattern the total is -inf whatever the rest does, and half of the cases must hold the finite total), 9 is the isolated state everywhere, 13 is possible at build time and impossible under a
    ``_block_zero`` trial matrix at some branches (below).
Exact zeros: the build-time matrices of the "closed" leaf branches are ``_block_zero`` ones (the last state is cut off), every other
matrix is dense.  Closed are all leaf children of internal node 0 and of its parent, and every leaf child but the first of any other
node with two or more leaf children (the first is "open").  Pattern 5 puts the last state at leaf 0 and others at its siblings:
impossible, and possible again once a dense trial matrix sits on one of those branches.  Pattern 13 puts the last state at the
leaves below internal node 0 and at the open leaves, others elsewhere: a ``_block_zero`` trial on an open leaf's branch (its closed
sibling forbids the last state at the parent), or on internal node 0's branch when its parent has a leaf child, makes it impossible.
"""
import numpy as np

from tests import scalefree as sf

STATE_COUNTS = (2, 5, 16, 17, 33, 48, 61, 64)
FULL_D = (5, 33, 61)              # the full-coverage shapes run at these
SMALL_D = (5, 17, 33, 61)         # the small shapes: one state count per row-block count (1d needs leaf pairs at each)
TRIAL_KINDS = ("build", "near_1em7", "near_eps", "ordinary", "identity", "block_zero")


def star_tree(n):
    """A root with ``n`` leaf children and a cherry."""
    return np.array([1] * n + [0, 0] + [1, -1], dtype=np.int64), n + 2


def star_below_tree(n):
    """scalefree's star_* shape: a node above ``n`` leaves next to a cherry, below a two-child root."""
    return np.array([0] * n + [1, 1] + [2, 2, -1], dtype=np.int64), n + 2


SHAPES = {
    # name: (flat_parents, L), S, which leaves carry ambiguity codes
    "bal2x4": (lambda: sf.balanced_tree(2, 4), 17, lambda l: l % 4 != 3),
    "bal4x3": (lambda: sf.balanced_tree(4, 3), 24, lambda l: l % 4 < 2),
    "ladder40": (lambda: sf.ladder_tree(40), 20, lambda l: l % 3 != 2),
    "star5": (lambda: star_tree(5), 21, lambda l: l in (0, 2)),
    "starbelow5": (lambda: star_below_tree(5), 21, lambda l: l in (1, 5)),
    "root_leaf_internal": (lambda: (np.array([0, 0, 1, 1, -1], dtype=np.int64), 3), 19, lambda l: l == 0),
    "root_internal_internal": (lambda: (np.array([0, 0, 1, 1, 2, 2, -1], dtype=np.int64), 4), 19, lambda l: l == 3),
    "three_leaves": (lambda: (np.array([0, 0, 0, -1], dtype=np.int64), 3), 1, lambda l: l == 1),
}
FULL_SHAPES = ("bal2x4", "bal4x3", "ladder40")


def closed_and_open_leaves(fp, L):
    ch = sf.children_of(fp, L)
    closed, opened = set(), set()
    special = [0] + ([int(fp[L])] if fp[L] >= 0 else [])
    for n, kids in enumerate(ch):
        leaves = [c for c in kids if c < L]
        if n in special:
            closed.update(leaves)
        elif len(leaves) >= 2:
            opened.add(leaves[0])
            closed.update(leaves[1:])
    return closed, opened


def leaves_below(fp, L, code):
    if code < L:
        return [code]
    ch = sf.children_of(fp, L)
    out, todo = [], [code]
    while todo:
        c = todo.pop()
        if c < L:
            out.append(c)
        else:
            todo += ch[c - L]
    return sorted(out)


def _mixed_patterns(rng, fp, L, D, S, k, is_ambig, impossible):
    codes = sf._patterns(rng, L, D, S, k)
    closed, opened = closed_and_open_leaves(fp, L)
    low = max(D - 1, 1)
    for l in range(L):                                  # ambiguity codes only where the case wants them, and there for certain
        neg = codes[l] < 0
        if not is_ambig(l):
            codes[l, neg] = (np.flatnonzero(neg) + 3 * l) % D
        elif 2 + 4 * (l % 4) < S:
            codes[l, 2 + 4 * (l % 4)] = -(1 + l % 2)
    shut = sorted(closed)                               # no zero likelihood by accident: the cut-off state stays away from closed leaves
    codes[shut] = np.where(codes[shut] == D - 1, max(D - 2, 0), codes[shut])
    first = leaves_below(fp, L, L)                      # the leaves below internal node 0
    for s in range(5, S, 16) if impossible else ():     # impossible at build time
        codes[:, s] = (np.arange(L) + s) % low
        codes[0, s] = D - 1
    for s in range(9, S, 16):                           # the isolated state everywhere
        codes[:, s] = D - 1
    for s in range(13, S, 16):                          # impossible under a _block_zero trial at an open leaf / at internal node 0
        codes[:, s] = (np.arange(L) * 3 + s) % low
        codes[first, s] = D - 1
        codes[sorted(opened), s] = D - 1
    return codes


def _matrices(rng, fp, L, D, eps):
    B = len(fp) - 1
    P = sf.ordinary(rng, B, D) if eps is None else sf.near_identity(rng, B, D, eps)
    closed, _ = closed_and_open_leaves(fp, L)
    idx = sorted(closed)
    P[idx] = sf._block_zero(P[idx], D)
    return P


def _make(name, shape, D, seed, branches=None, eps=None, tree=None, S=None, k=4):
    rng = np.random.default_rng(seed)
    if tree is None:
        mk, S, is_ambig = SHAPES[shape]
        fp, L = mk()
    else:
        (fp, L), is_ambig = tree, (lambda l: l % 5 == 0)
    if shape == "three_leaves":
        codes = np.array([[0], [-1], [1 % D]], dtype=np.int64)
    else:
        codes = _mixed_patterns(rng, fp, L, D, S, k, is_ambig, seed % 2 == 1)
    P = _matrices(rng, fp, L, D, eps)
    pi = rng.random(D) + 0.1
    cs = sf._case(name, D, fp, L, codes, P, rng, root_freqs=pi / pi.sum())
    B = len(fp) - 1
    cs["shape"] = shape
    cs["seed"] = seed
    cs["impossible_at_build"] = seed % 2 == 1 and shape != "three_leaves"
    cs["eps"] = 1e-3 if eps is None else eps
    cs["branches"] = list(range(B)) if branches is None else [int(b) for b in branches]
    return cs


def spread_ladder_branches(n_taxa):
    """Six branches of the n-taxon ladder from the bottom to just below the root, leaf and internal alike (leaf l >= 2 hangs off
    internal node l - 1; the root is internal node n - 2)."""
    L = n_taxa
    return [0, L + 0, n_taxa // 3, L + (2 * n_taxa) // 3, n_taxa - 1, L + n_taxa - 3]


# A case on which the reference's own scheme (oracle/hyphy_oracle.c) is not accurate to 1e-12 per pattern against ``prune``
# (tests/test_branchcache_cpu.py, check 1a) is named here with the reason and is then not built; no shape, state count or trial kind
# may lose all its cases this way.  (None so far.)
REFERENCE_FAILS = frozenset()


def _enumerate():
    seed = 7100
    for shape in FULL_SHAPES:
        for D in FULL_D:
            seed += 1
            yield dict(name=f"{shape}_D{D}", shape=shape, D=D, seed=seed)
    for D in STATE_COUNTS:
        if D not in FULL_D:
            seed += 1
            yield dict(name=f"bal2x4_D{D}", shape="bal2x4", D=D, seed=seed)
    for shape in SHAPES:
        if shape in FULL_SHAPES:
            continue
        for D in SMALL_D:
            seed += 1
            yield dict(name=f"{shape}_D{D}", shape=shape, D=D, seed=seed)
    for (D, n) in ((61, 300), (20, 600)):
        seed += 1
        yield dict(name=f"bigladder_D{D}_{n}", shape="bigladder", D=D, seed=seed, tree=sf.ladder_tree(n), S=20,
                   branches=spread_ladder_branches(n))
    for D in (20, 61):
        for eps in (1e-15, 1e-30):
            seed += 1
            fp, L = sf.balanced_tree(2, 6)
            path = [0]                                   # leaf 0 and its ancestors, the last leaf, a leaf and a node in the middle
            while fp[path[-1]] >= 0 and L + int(fp[path[-1]]) < len(fp) - 1:
                path.append(L + int(fp[path[-1]]))
            yield dict(name=f"conflict_D{D}_{sf._name_eps(eps)}", shape="conflict", D=D, seed=seed, tree=(fp, L), S=24, k=2, eps=eps,
                       branches=path + [L - 1, 20, L + 13])


def cases():
    return [_make(**kw) for kw in _enumerate() if kw["name"] not in REFERENCE_FAILS]


_by_name = {}


def cases_by_name():
    if not _by_name:
        _by_name.update({c["name"]: c for c in cases()})
    return _by_name


def full_coverage_names():
    return [f"{shape}_D{D}" for shape in FULL_SHAPES for D in FULL_D]


def class_cases():
    """scalefree's ``classes_*`` recipe (three rate classes with off-diagonals 1e-2, 1e-12, 1e-30) at D = 20 and 61 on the 64-taxon
    binary tree, with this module's patterns and a random pi.  ``branches``: a leaf branch, a deep internal branch, a root child."""
    out = []
    for j, D in enumerate((20, 61)):
        rng = np.random.default_rng(7300 + j)
        fp, L = sf.balanced_tree(2, 6)
        codes = _mixed_patterns(rng, fp, L, D, 24, 2, lambda l: l % 5 == 0, j == 1)
        B = len(fp) - 1
        P = np.stack([sf.near_identity(rng, B, D, e, spread=D * e < 0.3) for e in (1e-2, 1e-12, 1e-30)])
        pi = rng.random(D) + 0.1
        cs = sf._case(f"bc_classes_D{D}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum(), weights=np.array([0.5, 0.3, 0.2]))
        cs["seed"] = 7300 + j
        cs["eps"] = 1e-12
        cs["branches"] = [5, L + 3, B - 1]
        out.append(cs)
    return out


def chunked_class_case(D, S):
    """``class_cases``' recipe (three rate classes with off-diagonals 1e-2, 1e-12, 1e-30, weights 0.5, 0.3, 0.2) on the shape the
    chunking tests walk in chunks: the 32-taxon binary tree (62 branches), ``S`` patterns, twelve sampled branches."""
    rng = np.random.default_rng(7360 + D)
    fp, L = sf.balanced_tree(2, 5)
    codes = _mixed_patterns(rng, fp, L, D, S, 4, lambda l: l % 5 == 0, False)
    B = len(fp) - 1
    P = np.stack([sf.near_identity(rng, B, D, e, spread=D * e < 0.3) for e in (1e-2, 1e-12, 1e-30)])
    pi = rng.random(D) + 0.1
    cs = sf._case(f"wide_bal2x5_classes_D{D}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum(), weights=np.array([0.5, 0.3, 0.2]))
    cs["seed"] = 7360 + D
    cs["eps"] = 1e-12
    cs["branches"] = [int(b) for b in rng.choice(B, size=12, replace=False)]
    return cs


# ---- trial matrices and references ------------------------------------------------------------------------------------------------

def trials(cs, node, cls=None):
    """[(kind, M)] for branch ``node`` of the case, in TRIAL_KINDS' order; seeded by the case and the branch."""
    D = int(cs["D"])
    rng = np.random.default_rng([int(cs["seed"]), int(node)])
    P = cs["P"] if cls is None else cs["P"][cls]
    return [("build", P[node].copy()),
            ("near_1em7", sf.near_identity(rng, 1, D, 1e-7)[0]),
            ("near_eps", sf.near_identity(rng, 1, D, float(cs["eps"]))[0]),
            ("ordinary", sf.ordinary(rng, 1, D)[0]),
            ("identity", np.eye(D)),
            ("block_zero", sf._block_zero(sf.ordinary(rng, 1, D), D)[0])]


_refs = {}


def reference(cs, node=None, M=None, key=None, cls=None):
    """scalefree.prune of the case with ``P[node] = M`` (class ``cls`` of a rate-class case), cached under (case, node, key, cls)."""
    k = (cs["name"], node, key, cls)
    if key is None or k not in _refs:
        P = cs["P"] if cls is None else cs["P"][cls]
        if node is not None:
            P = P.copy()
            P[node] = M
        ref = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P, cs["root_freqs"])
        if key is None:
            return ref
        _refs[k] = ref
    return _refs[k]


def ancestors(cs, node):
    """Internal indices from the root down to the parent of ``node``: a[0] = root ... a[m] = parent; m is the path depth."""
    L = int(cs["L"])
    fp = cs["flat_parents"]
    a = []
    x = int(fp[node])
    while x >= 0:
        a.append(x)
        x = int(fp[L + x])
    return a[::-1]


def rerooted_site_logl(cs, node, M, transposed=True, pi_on_edge=True):
    """Per-pattern log-likelihood by the re-rooted recurrence, in plain float64 without any rescaling (small trees only).
    A_0 = product over the root's other children of their edge products; for k >= 1
    A_k[j] = (sum_i M_k[j][i] A_{k-1}[i]) x (edge products of a[k]'s other children), M_k[j][i] = P_{a[k]}[i][j], times pi_i when
    k = 1; L_s = sum_i A_m[i] (pi_i when m = 0) sum_j M[i][j] B[j], B the conditionals of ``node``.
    ``transposed=False`` uses P_{a[k]} as it stands, ``pi_on_edge=False`` leaves pi off the edge below the old root: the two
    mistakes that a reversible model at its stationary pi cannot show."""
    D, L = int(cs["D"]), int(cs["L"])
    fp = np.asarray(cs["flat_parents"], dtype=np.int64)
    codes = np.asarray(cs["leaf_codes"], dtype=np.int64)
    amb = np.asarray(cs["ambig"], dtype=np.float64)
    P, pi = cs["P"], np.asarray(cs["root_freqs"], dtype=np.float64)
    S = codes.shape[1]
    sel = np.arange(S)
    ch = sf.children_of(fp, L)
    cond = [None] * len(ch)
    for n in range(len(ch)):                             # inside vectors, unnormalised
        v = np.ones((S, D))
        for c in ch[n]:
            v = v * sf._edge(P[c], c, L, codes, amb, cond, None, sel)
        cond[n] = v
    a = ancestors(cs, node)
    m = len(a) - 1
    A = None
    for k in range(m + 1):
        exclude = L + a[k + 1] if k < m else node
        if k == 0:
            A = np.ones((S, D))
        else:
            Pk = P[L + a[k]]
            Mk = Pk.T if transposed else Pk
            if k == 1 and pi_on_edge:
                Mk = Mk * pi[None, :]
            A = A @ Mk.T
        for c in ch[a[k]]:
            if c != exclude:
                A = A * sf._edge(P[c], c, L, codes, amb, cond, None, sel)
    t = A * sf._edge(np.asarray(M, dtype=np.float64), node, L, codes, amb, cond, None, sel)
    if m == 0:
        t = t * pi
    lik = t.sum(axis=1)
    with np.errstate(divide="ignore"):
        return np.where(lik > 0, np.log(lik), -np.inf)


def arm_features(cs, node, order=None):
    """What the build and the evaluation of branch ``node`` run through, as the library decides it (api.hip: the leaf pairing of
    hyphy_hip_branch_cache_build; prune.hip: bc_eval_kernel's arms per tile of 16 patterns in the device's pattern order)."""
    L = int(cs["L"])
    codes = np.asarray(cs["leaf_codes"])
    S = codes.shape[1]
    order = np.arange(S) if order is None else np.asarray(order)
    has_amb = (codes < 0).any(axis=1)
    ch = sf.children_of(cs["flat_parents"], L)
    a = ancestors(cs, node)
    m = len(a) - 1
    f = dict(blocks=(int(cs["D"]) + 15) // 16, depth=m, internal_child=node >= L, leaf_plain_tile=False, leaf_mixed_tile=False,
             leaf_pair=False, ambig_sibling=False)
    if node < L:
        row = codes[node][order]
        for t in range(0, S, 16):
            neg = row[t: t + 16] < 0
            if not neg.any():
                f["leaf_plain_tile"] = True
            elif not neg.all():
                f["leaf_mixed_tile"] = True
    for k in range(m + 1):
        exclude = L + a[k + 1] if k < m else node
        leaves = [c for c in ch[a[k]] if c < L and c != exclude]
        i = 0
        while i < len(leaves):
            if has_amb[leaves[i]]:
                f["ambig_sibling"] = True
                i += 1
            elif i + 1 < len(leaves) and not has_amb[leaves[i + 1]]:
                f["leaf_pair"] = True
                i += 2
            else:
                i += 1
    return f
