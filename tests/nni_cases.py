"""Cases and references for the nearest-neighbour interchanges (hyphy_hip_plan_nni / hyphy_hip_nni_scores, hyphy_amd/nni.py).

A move (x, y): c = parent(x) is an internal node other than the root, y a sibling of c; x and y exchange parents and every branch
keeps its matrix.  The reference for a move is ``scalefree.prune`` on ``nni.apply_nni``'s tree with the matrices permuted along
(``reference``).  ``model`` restates what the library computes instead (include/hyphy_hip.h, "nearest-neighbour interchange"): the
outside vectors of a pre-order pass and the contraction at the branch, every vector under the 2^64 rule, in numpy.

``enumerate_moves`` / ``is_move`` are the rule in plain Python, ``check_numbering`` what a valid tree is, ``PLAN_TREES`` the trees the
planner is compared on, ``shape_cases`` the shapes tests/branchcache_cases.py lacks, ``search_case`` the data of the hill-climb test.
"""
import numpy as np

from tests import branchcache_cases as bc
from tests import scalefree as sf

# ---- the rule ---------------------------------------------------------------------------------------------------------------------


def is_move(fp, L, x, y):
    fp = np.asarray(fp, dtype=np.int64)
    root = len(fp) - 1
    if not (0 <= x < root and 0 <= y < root):
        return False
    c = L + int(fp[x])
    return c != root and y != c and fp[y] == fp[c]


def why_not_a_move(fp, L, x, y):
    """None for a move, else the part of the rule the pair breaks, in the library's words (include/hyphy_hip.h: the first that applies
    of: x no branch, y no branch, c the root, y == c, y no sibling of c)."""
    fp = np.asarray(fp, dtype=np.int64)
    root = len(fp) - 1
    if not 0 <= x < root:
        return "x is not the code of a branch (the root has none)"
    if not 0 <= y < root:
        return "y is not the code of a branch (the root has none)"
    c = L + int(fp[x])
    if c == root:
        return "the parent of x is the root"
    if y == c:
        return "y is the parent of x"
    siblings = [k for k in range(root) if fp[k] == fp[c] and k != c]
    return None if y in siblings else "y is not a sibling of the parent of x"


def enumerate_moves(fp, L):
    """Every move as (x, y), in ascending (c, y, x)."""
    fp = np.asarray(fp, dtype=np.int64)
    ch = sf.children_of(fp, L)
    out = []
    for ci in range(len(ch) - 1):
        c = L + ci
        for y in ch[int(fp[c])]:
            if y != c:
                out += [(x, y) for x in ch[ci]]
    return out


def check_numbering(fp, L):
    """Children before parents, the root last and alone without a parent, every internal node with at least one child."""
    fp = np.asarray(fp, dtype=np.int64)
    I = len(fp) - L
    assert I >= 1 and fp[-1] == -1, fp
    assert np.all(fp[:-1] >= 0) and np.all(fp[:-1] < I), fp
    for i in range(I - 1):
        assert fp[L + i] > i, (i, fp)
    assert all(len(k) >= 1 for k in sf.children_of(fp, L)), fp


def splits(fp, L):
    """The leaf sets below the internal non-root nodes (a rooted tree's clades)."""
    fp = np.asarray(fp, dtype=np.int64)
    return {frozenset(bc.leaves_below(fp, L, L + i)) for i in range(len(fp) - L - 1)}


def from_nested(t):
    """(flat_parents, L) of a tree written as nested lists of leaf numbers: internal nodes are numbered in post-order, the children
    of a node in the order written."""
    leaves = []

    def count(n):
        if isinstance(n, int):
            leaves.append(n)
        else:
            for k in n:
                count(k)
    count(t)
    L = len(leaves)
    assert sorted(leaves) == list(range(L))
    par = {}
    nxt = [L]

    def walk(n):
        if isinstance(n, int):
            return n
        kids = [walk(k) for k in n]
        code = nxt[0]
        nxt[0] += 1
        for k in kids:
            par[k] = code - L
        return code
    root = walk(t)
    par[root] = -1
    return np.array([par[c] for c in range(root + 1)], dtype=np.int64), L


def wide_node_tree(n=41):
    """A node with ``n`` children (leaves and two cherries) below a three-child root."""
    return from_nested([[[0, 1], [2, 3]] + list(range(4, 4 + n - 2)), [n + 2, n + 3], n + 4])


PLAN_TREES = {
    "balanced": lambda: sf.balanced_tree(2, 4),
    "balanced4": lambda: sf.balanced_tree(4, 2),
    "ladder": lambda: sf.ladder_tree(9),
    "star": lambda: (np.array([0] * 6 + [-1], dtype=np.int64), 6),
    "three_leaves": lambda: (np.array([0, 0, 0, -1], dtype=np.int64), 3),
    "two_child_root": lambda: (np.array([0, 0, 1, 1, 2, 2, -1], dtype=np.int64), 4),
    "three_child_root": lambda: from_nested([[0, 1], [[2, 3], 4], 5]),
    "wide41": wide_node_tree,
    "shapes": lambda: from_nested(SHAPE_TREE),
}

# ---- references -------------------------------------------------------------------------------------------------------------------


def neighbour(cs, x, y):
    """(flat_parents, P) of the neighbour tree: ``apply_nni``'s numbering, the matrices permuted along."""
    from hyphy_amd import nni
    fp2, perm = nni.apply_nni(cs["flat_parents"], int(cs["L"]), x, y)
    P = np.asarray(cs["P"])
    return fp2, (P[perm[:-1]] if P.ndim == 3 else P[:, perm[:-1]])


_refs = {}


def reference(cs, x, y):
    """scalefree.prune on the neighbour tree, cached under (case, move)."""
    k = (cs["name"], int(x), int(y))
    if k not in _refs:
        fp2, P2 = neighbour(cs, x, y)
        _refs[k] = sf.prune(cs["D"], fp2, cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], P2, cs["root_freqs"],
                            weights=cs.get("weights"))
    return _refs[k]


def _rescale(v, cnt):
    """rescale_vec's rule on the rows of v ([S, D]) with their exponents cnt ([S]), in place."""
    T, U = 2.0 ** -64, 2.0 ** 64
    tot = v.sum(axis=1)
    for _ in range(15):
        low = (tot < T) & (tot > 0)
        if not low.any():
            break
        v[low] *= U
        tot[low] *= U
        cnt[low] += 1
    for _ in range(15):
        high = (tot > U) & np.isfinite(tot)
        if not high.any():
            break
        v[high] *= T
        tot[high] *= T
        cnt[high] -= 1


def model(cs, moves, cls=None):
    """[(likelihood [S], exponent [S])] of ``moves`` by the formula the library documents, every vector under the 2^64 rule:
    R = U_p prod E_k (children of p other than c and y), inner = E_y prod E_k (children of c other than x),
    l = sum_i R[i] E_x[i] (P_c inner)[i], exponent(R) + exponent(E_x) + exponent(inner)."""
    D, L = int(cs["D"]), int(cs["L"])
    fp = np.asarray(cs["flat_parents"], dtype=np.int64)
    I = len(fp) - L
    codes = np.asarray(cs["leaf_codes"], dtype=np.int64)
    S = codes.shape[1]
    amb = np.asarray(cs["ambig"], dtype=np.float64) if cs["ambig"] is not None and len(cs["ambig"]) else np.zeros((1, D))
    P = cs["P"] if cls is None else cs["P"][cls]
    pi = np.asarray(cs["root_freqs"], dtype=np.float64)
    ch = sf.children_of(fp, L)
    sel = np.arange(S)
    cond, ccnt = [None] * I, np.zeros((I, S), dtype=np.int64)
    E, ecnt = {}, {}
    for n in range(I):                                     # inside pass
        v = np.ones((S, D))
        for k in ch[n]:
            E[k] = sf._edge(P[k], k, L, codes, amb, cond, None, sel)
            ecnt[k] = ccnt[k - L].copy() if k >= L else np.zeros(S, dtype=np.int64)
            v = v * E[k]
            ccnt[n] += ecnt[k]
            _rescale(v, ccnt[n])
        cond[n] = v
    U, ucnt = [None] * I, np.zeros((I, S), dtype=np.int64)
    U[I - 1] = np.broadcast_to(pi, (S, D)).copy()
    for n in range(I - 1, -1, -1):                         # outside pass
        for k in ch[n]:
            if k < L:
                continue
            v, cnt = U[n].copy(), ucnt[n].copy()
            for s2 in ch[n]:
                if s2 != k:
                    v = v * E[s2]
                    cnt += ecnt[s2]
                    _rescale(v, cnt)
            u = v @ P[k]
            _rescale(u, cnt)
            U[k - L], ucnt[k - L] = u, cnt
    out = []
    for x, y in moves:
        ci = int(fp[x])
        pidx = int(fp[L + ci])
        R, rcnt = U[pidx].copy(), ucnt[pidx].copy()
        for k in ch[pidx]:
            if k not in (L + ci, y):
                R = R * E[k]
                rcnt += ecnt[k]
                _rescale(R, rcnt)
        inner, icnt = E[y].copy(), ecnt[y].copy()
        for k in ch[ci]:
            if k != x:
                inner = inner * E[k]
                icnt += ecnt[k]
                _rescale(inner, icnt)
        F = inner @ P[L + ci].T
        out.append(((R * E[x] * F).sum(axis=1), rcnt + ecnt[x] + icnt))
    return out


# ---- moves of the branch-cache cases ----------------------------------------------------------------------------------------------


def case_moves(cs):
    """The moves a case is scored on: all of them, except on the 300- and 600-taxon ladders, where only those at the lowest, a middle
    and the highest branch are (their exponents are the furthest from zero, and the reference stays short)."""
    fp, L = cs["flat_parents"], int(cs["L"])
    mv = enumerate_moves(fp, L)
    if cs["name"].startswith("bigladder"):
        cs_ = sorted({L + int(fp[x]) for x, _ in mv})
        keep = {cs_[0], cs_[len(cs_) // 2], cs_[-1]}
        mv = [m for m in mv if L + int(fp[m[0]]) in keep]
    return mv


def shuffled(moves, fp, L, seed):
    """``moves`` in a seeded order in which the moves of one branch are not adjacent, wherever no branch holds more than half of them
    (``can_keep_apart``): the next move comes from the branch with the most moves left other than the one just served, ties at random."""
    rng = np.random.default_rng(seed)
    per = {}
    for m in moves:
        per.setdefault(L + int(fp[m[0]]), []).append(m)
    for c in per:
        per[c] = [per[c][k] for k in rng.permutation(len(per[c]))]
    out, last = [], None
    while any(per.values()):
        cand = [c for c in sorted(per) if per[c] and c != last] or [last]
        most = max(len(per[c]) for c in cand)
        c = int(rng.choice([c for c in cand if len(per[c]) == most]))
        out.append(per[c].pop())
        last = c
    return out


def can_keep_apart(moves, fp):
    n = {}
    for x, _ in moves:
        n[int(fp[x])] = n.get(int(fp[x]), 0) + 1
    return max(n.values()) <= (len(moves) + 1) // 2


# ---- the shapes the branch-cache cases lack ---------------------------------------------------------------------------------------

# G1 = [[0, 1], 2, [3, 4, 5]] has three children, so has its last child; the root has three children with a leaf the third.
#   c = G1:          x a leaf (2) or internal; y = G2 (internal, numbered above c) or leaf 10 (the root's third child: R = pi E_G2)
#   c = [3, 4, 5]:   three leaf children (inner carries two more factors); p = G1 is not the root (R = U_p E_k); y = [0, 1] or leaf 2
#   c = G2:          y = G1 (internal, numbered below c) or leaf 10
SHAPE_TREE = [[[0, 1], 2, [3, 4, 5]], [[6, 7], [8, 9]], 10]
AMBIG_ROWS = (0, 2, 5, 10)        # leaves that are x or y of some move; their ambiguity codes sit in patterns 16 .. 31 only
SHAPE_S = 40
IMPOSSIBLE_MOVES = ((0, 2), (1, 2))   # ... make pattern 7 impossible (shape_case)


def shape_case(D):
    """The shape tree at ``D`` states, 40 patterns: ambiguity codes in the rows of AMBIG_ROWS at patterns 16 .. 31 and nowhere else,
    pattern 3 of frequency 0, and block-zero matrices (the last state cut off) on the branches of leaves 0, 1 and 2.  Pattern 7 has
    the cut-off state at leaves 0 and 1 and other states elsewhere: possible on the tree as it stands ([0, 1] is in the cut-off
    state, and its own branch is dense), impossible once 2 has taken the place of 0 or 1 (IMPOSSIBLE_MOVES): the two children of
    [0, 1] then ask for the cut-off state and for another one.  Nowhere else does a closed leaf carry the cut-off state, except in
    pattern 9, which has it everywhere."""
    rng = np.random.default_rng(7500 + D)
    fp, L = from_nested(SHAPE_TREE)
    S = SHAPE_S
    low = max(D - 1, 1)
    codes = rng.integers(0, D, size=(L, S))
    codes[:3] = np.minimum(codes[:3], low - 1)
    codes[:, 0] = 1                                       # conserved
    codes[:, 1] = np.arange(L) % low
    codes[:, 20] = 2 % D
    for j, l in enumerate(AMBIG_ROWS):
        codes[l, 17 + 3 * j] = -1 - (j % 2)
        codes[l, 18 + 3 * j] = -2 + (j % 2)
    codes[:, 7] = (np.arange(L) * 3) % low
    codes[[0, 1], 7] = D - 1
    codes[:, 9] = D - 1                                   # the isolated state everywhere
    B = len(fp) - 1
    P = sf.ordinary(rng, B, D)
    P[:3] = sf._block_zero(P[:3], D)
    pi = rng.random(D) + 0.1
    cs = sf._case(f"nni_shapes_D{D}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum())
    cs["pattern_freq"][3] = 0
    cs["seed"] = 7500 + D
    return cs


_shape = {}


def shape_cases():
    for D in (5, 61):
        if D not in _shape:
            _shape[D] = shape_case(D)
    return [_shape[5], _shape[61]]


# ---- the hill-climb ---------------------------------------------------------------------------------------------------------------

SEARCH_TREE = [[[0, 1], [2, 3]], [4, [5, 6]], 7]          # 8 taxa, a three-child root
SEARCH_SEED, SEARCH_SITES = 11, 600
SEARCH_START_MOVES = 2


def hky_unit(kappa, pi):
    """HKY85 rate matrix of unit expected rate (states A, C, G, T)."""
    Q = np.array([[0, 1, kappa, 1], [1, 0, 1, kappa], [kappa, 1, 0, 1], [1, kappa, 1, 0]], dtype=np.float64) * pi[None, :]
    Q[np.arange(4), np.arange(4)] = -Q.sum(axis=1)
    return Q / -(pi * np.diag(Q)).sum()


def expm_np(Q):
    """exp(Q) by scaling and squaring with a Taylor series (host-side check only)."""
    Q = np.asarray(Q, dtype=np.float64)
    s = max(0, int(np.ceil(np.log2(max(np.abs(Q).sum(axis=-1).max(), 1e-300)))) + 4)
    X = Q / 2.0 ** s
    out = term = np.broadcast_to(np.eye(Q.shape[-1]), Q.shape).copy()
    for k in range(1, 16):
        term = term @ X / k
        out = out + term
    for _ in range(s):
        out = out @ out
    return out


def search_case():
    """Patterns sampled down SEARCH_TREE under HKY85 (kappa 3) from a fixed seed, and a starting tree SEARCH_START_MOVES moves away."""
    from hyphy_amd import nni
    rng = np.random.default_rng(SEARCH_SEED)
    fp, L = from_nested(SEARCH_TREE)
    B = len(fp) - 1
    pi = np.array([0.3, 0.2, 0.2, 0.3])
    Q = hky_unit(3.0, pi)
    t = rng.uniform(0.08, 0.25, size=B)
    P = expm_np(t[:, None, None] * Q[None])
    n = SEARCH_SITES
    state = np.zeros((B + 1, n), dtype=np.int64)
    state[B] = rng.choice(4, size=n, p=pi)
    for code in range(B - 1, -1, -1):
        par = L + int(fp[code])
        cum = np.cumsum(P[code][state[par]], axis=1)
        state[code] = np.minimum((rng.random(n)[:, None] > cum).sum(axis=1), 3)
    cols, freq = np.unique(state[:L], axis=1, return_counts=True)
    start, moves = fp, []
    for k in range(SEARCH_START_MOVES):                    # away from the generating tree: each move breaks one more of its clades
        for x, y in enumerate_moves(start, L):
            cand, _ = nni.apply_nni(start, L, x, y)
            if len(splits(cand, L) - splits(fp, L)) == k + 1:
                start = cand
                moves.append((x, y))
                break
    assert len(splits(start, L) - splits(fp, L)) == SEARCH_START_MOVES
    return dict(name="nni_search", D=4, L=L, flat_parents=fp, start=start, leaf_codes=np.ascontiguousarray(cols), ambig=None,
                pattern_freq=freq.astype(np.int64), root_freqs=pi, Q=Q, t=t)
