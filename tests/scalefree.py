"""A scale-free reference for the pruning, and the cases that stress the 2^64 rescaling.

``prune`` is Felsenstein's recurrence in numpy with NO power-of-2^64 scheme: at every internal node the children's ``P @ v`` are
multiplied, the vector is divided by its largest element and the logarithm of that element goes to a per-pattern accumulator.  It
shares nothing with the kernels or with ``oracle/hyphy_oracle.c`` beyond the recurrence, so a mistake common to both (threshold
direction, multi-step rescale, the cap on the steps) shows against it.  tests/test_scalefree_cpu.py pins it to mpmath at 50 digits, to
the reference's own per-site values in the goldens, and to the oracle on every case of ``rescale_edge_cases``.

Largest deviation of the oracle's per-pattern log-likelihood from this reference over the whole case list, measured by
test_scalefree_cpu.py::test_oracle_agrees_on_every_generated_case (relative, patterns of finite likelihood):

    ORACLE_MAX_REL = 3.1e-15

(3.0e-15 measured, ladder_D20_600; the constant is that rounded up.)  It is below 1e-13, so the GPU tests hold the kernels to
GPU_RTOL = 100 x that plus the absolute 1e-9 of tests/test_gpu_parity.py (tests/test_gpu_rescale.py).  With per-pattern values of
1e2 .. 1e4 in size the relative term is 3e-11 .. 3e-9: for most patterns the absolute 1e-9 is the larger part of the allowance.

``prune(..., posteriors=True)`` adds the marginal posteriors of a pre-order pass over the same normalised vectors: ``post`` for the
internal nodes and ``leaf_post``, the reference's DOLEAVES ratio L_s(leaf = x) / L_s (not normalised over x), for the leaves;
test_scalefree_cpu.py pins both to pinned-state evaluations (exp of the difference of two ``site_logl``) and to brute force.

Node numbering as everywhere in the project: leaf l has node code l, internal node i has code L + i, children before parents, the
root last; ``flat_parents[code]`` is the internal index of the parent; ``P[code]`` is the matrix of the branch above ``code``.
"""
import numpy as np

LOG_SCALER = 64.0 * np.log(2.0)
ORACLE_MAX_REL = 3.1e-15
GPU_RTOL = 100 * ORACLE_MAX_REL


def children_of(flat_parents, L):
    fp = np.asarray(flat_parents, dtype=np.int64)
    I = len(fp) - int(L)
    ch = [[] for _ in range(I)]
    for code in range(len(fp) - 1):
        ch[int(fp[code])].append(code)
    return ch


def _edge(P, code, L, leaf_codes, ambig, cond, pin, sel):
    """[S, D] values of (P @ v) of the child with node code ``code`` at every selected pattern."""
    if code >= L:
        return cond[code - L] @ P.T
    k = leaf_codes[code, sel]
    if pin is not None and pin[0] == code:
        k = pin[1][sel]
    out = P.T[np.maximum(k, 0)]                       # resolved state: a column of P
    amb = np.flatnonzero(k < 0)
    if len(amb):
        out = out.copy()
        out[amb] = ambig[-k[amb] - 1] @ P.T
    return out


def _prune_one(D, fp, L, leaf_codes, ambig, P, pi, pin, sel, want_cond, want_post, ft=np.float64):
    I = len(fp) - L
    S = len(sel)
    ch = children_of(fp, L)
    cond = [None] * I          # normalised conditionals (largest element 1; zeros where the likelihood is zero)
    lg = np.zeros((I, S), dtype=ft)   # log of everything divided out at and below the node (``ft``: the type it is summed in)
    edges = {}
    for n in range(I):
        v = np.ones((S, D))
        acc = np.zeros(S, dtype=ft)
        if pin is not None and pin[0] == L + n:
            v = np.zeros((S, D))
            v[np.arange(S), pin[1][sel]] = 1.0
        for c in ch[n]:
            e = _edge(P[c], c, L, leaf_codes, ambig, cond, pin, sel)
            if want_post:
                edges[c] = e
            v = v * e
            if c >= L:
                acc = acc + lg[c - L]
            m = v.max(axis=1)                         # normalise after every factor: nothing piles up
            ok = m > 0
            v = np.where(ok[:, None], v / np.where(ok, m, 1.0)[:, None], 0.0)
            with np.errstate(divide="ignore"):
                acc = acc + np.log(m.astype(ft))
        cond[n] = v
        lg[n] = acc
    root = cond[I - 1] @ pi
    with np.errstate(divide="ignore"):
        site = np.log(root.astype(ft)) + lg[I - 1]
    site = np.where(root > 0, site, -np.inf)
    out = {"site_logl": site}
    if want_cond:
        out["cond"] = np.stack(cond)
        out["log_mag"] = lg
    if want_post:
        # pre-order: up[n] = everything outside the subtree of n, as a function of n's state (normalised)
        up = [None] * I
        up[I - 1] = np.broadcast_to(pi, (S, D)).copy()
        post = np.zeros((I, S, D))
        leaf_post = np.zeros((L, S, D))
        for n in range(I - 1, -1, -1):
            w = cond[n] * up[n]
            t = w.sum(axis=1)
            post[n] = np.where((t > 0)[:, None], w / np.where(t > 0, t, 1.0)[:, None], np.nan)
            kids = ch[n]
            for c in kids:
                o = up[n].copy()
                if pin is not None and pin[0] == L + n:
                    z = np.zeros((S, D))
                    z[np.arange(S), pin[1][sel]] = 1.0
                    o = o * z
                for s2 in kids:
                    if s2 != c:
                        o = o * edges[s2]
                        m = o.max(axis=1)
                        o = np.where((m > 0)[:, None], o / np.where(m > 0, m, 1.0)[:, None], 0.0)
                u = o @ P[c]
                if c < L:                             # a leaf: U_l(x) / sum_y U_l(y) leafvec_l(y), unnormalised over x
                    k = leaf_codes[c, sel]
                    lv = np.where((k >= 0)[:, None], np.eye(D)[np.maximum(k, 0)], ambig[np.maximum(-k - 1, 0)])
                    t = (u * lv).sum(axis=1)
                    leaf_post[c] = np.where((t > 0)[:, None], u / np.where(t > 0, t, 1.0)[:, None], np.nan)
                    continue
                m = u.max(axis=1)
                up[c - L] = np.where((m > 0)[:, None], u / np.where(m > 0, m, 1.0)[:, None], 0.0)
        out["post"] = post
        out["leaf_post"] = leaf_post
    return out


def prune(D, flat_parents, L, leaf_codes, ambig, pattern_freq, P, root_freqs, weights=None, pinned=None, patterns=None,
          conditionals=False, posteriors=False, log_dtype=np.float64):
    """Scale-free pruning.  ``P``: [B, D, D] transition matrices by node code, or [C, B, D, D] with class ``weights`` [C];
    ``pinned`` = (node code, states [S]); ``patterns``: the subset of pattern indices to evaluate (default: all).
    Returns a dict: ``site_logl`` [S'] (-inf where the likelihood is exactly zero), ``logl`` (sum over patterns with their
    frequencies), and on request ``cond`` [C?, I, S', D] (conditionals divided by their largest element), ``log_mag`` [C?, I, S']
    (log of that divisor, accumulated over the subtree), ``post`` [I, S', D] (marginal posteriors of the internal nodes) and
    ``leaf_post`` [L, S', D] (the reference's DOLEAVES quantity L_s(leaf = x) / L_s, not normalised over x: U_l(x) / sum_y U_l(y)
    leafvec_l(y) with U_l the outside vector pushed through P[l]); both NaN where the likelihood is zero.  Classes are mixed by
    their share of the pattern's likelihood; a class of share 0 is passed over.  ``log_dtype``: the type the logarithms are summed in
    (np.longdouble where two ``site_logl`` of size 1e3 are to be subtracted to 1e-12 of their difference's exponential)."""
    D, L = int(D), int(L)
    fp = np.asarray(flat_parents, dtype=np.int64)
    codes = np.asarray(leaf_codes, dtype=np.int64)
    amb = np.asarray(ambig, dtype=np.float64) if ambig is not None and len(ambig) else np.zeros((1, D))
    freq = np.asarray(pattern_freq, dtype=np.float64)
    pi = np.asarray(root_freqs, dtype=np.float64)
    sel = np.arange(codes.shape[1]) if patterns is None else np.asarray(patterns, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    pin = None if pinned is None else (int(pinned[0]), np.asarray(pinned[1], dtype=np.int64))
    if P.ndim == 3:
        out = _prune_one(D, fp, L, codes, amb, P, pi, pin, sel, conditionals, posteriors, log_dtype)
    else:
        w = np.asarray(weights, dtype=np.float64)
        per = [_prune_one(D, fp, L, codes, amb, P[c], pi, pin, sel, conditionals, posteriors, log_dtype) for c in range(P.shape[0])]
        sl = np.stack([p["site_logl"] for p in per])
        with np.errstate(divide="ignore"):
            z = sl + np.log(w)[:, None]
        top = z.max(axis=0)
        safe = np.where(np.isfinite(top), top, 0.0)
        with np.errstate(divide="ignore"):
            site = np.where(np.isfinite(top), safe + np.log(np.exp(z - safe).sum(axis=0)), -np.inf)
        out = {"site_logl": site, "class_site_logl": sl}
        if conditionals:
            out["cond"] = np.stack([p["cond"] for p in per])
            out["log_mag"] = np.stack([p["log_mag"] for p in per])
        if posteriors:   # classes mixed by their share of the pattern's likelihood
            share = np.exp(z - safe)           # (a class under which the pattern is impossible has share 0 and a NaN posterior
            tot = share.sum(axis=0)            #  of its own: it is passed over; impossible under every class: NaN)
            share = share / np.where(tot > 0, tot, 1.0)
            for key in ("post", "leaf_post"):
                mix = sum(np.where(share[c][None, :, None] > 0, share[c][None, :, None] * per[c][key], 0.0) for c in range(len(per)))
                out[key] = np.where((tot > 0)[None, :, None], mix, np.nan)
    out["logl"] = float(np.sum(out["site_logl"] * freq[sel]))
    return out


def case_reference(cs, **kw):
    return prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], cs["P"], cs["root_freqs"],
                 weights=cs.get("weights"), **kw)


# ---- a model of "which nodes are tested" (the 2^64 rule in numpy), for the CPU test of the thinning rule ----------------------

def model_logl(cs, tested=None):
    """Per-pattern log-likelihood under the 2^64 rule applied to the NODE sums of the internal nodes in ``tested`` (a boolean array
    over the internal nodes; None: every node) — what a kernel that finalises a node and then tests it computes, in plain float64,
    denormals and underflow included."""
    D, L = int(cs["D"]), int(cs["L"])
    fp = np.asarray(cs["flat_parents"], dtype=np.int64)
    I = len(fp) - L
    codes = np.asarray(cs["leaf_codes"], dtype=np.int64)
    S = codes.shape[1]
    amb = np.asarray(cs["ambig"], dtype=np.float64) if cs["ambig"] is not None and len(cs["ambig"]) else np.zeros((1, D))
    ch = children_of(fp, L)
    cond = [None] * I
    cnt = np.zeros((I, S), dtype=np.int64)
    sel = np.arange(S)
    T, U = 2.0 ** -64, 2.0 ** 64
    for n in range(I):
        v = np.ones((S, D))
        for c in ch[n]:
            v = v * _edge(cs["P"][c], c, L, codes, amb, cond, None, sel)
            if c >= L:
                cnt[n] += cnt[c - L]
        if tested is None or tested[n]:
            tot = v.sum(axis=1)
            for _ in range(15):
                low = (tot < T) & (tot > 0)
                if not low.any():
                    break
                v[low] *= U
                tot[low] *= U
                cnt[n][low] += 1
        cond[n] = v
    lik = cond[I - 1] @ np.asarray(cs["root_freqs"], dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(lik > 0, np.log(lik) - LOG_SCALER * cnt[I - 1], -np.inf)


# ---- cases --------------------------------------------------------------------------------------------------------------------

def balanced_tree(k, depth):
    """flat_parents, L of the balanced tree with ``k`` children per node and ``depth`` levels of internal nodes."""
    L = k ** depth
    parents = []
    width = L                      # nodes of the level below (leaves first)
    level_start = 0
    for _ in range(depth):
        parents += [level_start + j // k for j in range(width)]
        level_start += width // k
        width //= k
    return np.array(parents + [-1], dtype=np.int64), L


def ladder_tree(n_taxa, hang=None):
    """A caterpillar of ``n_taxa`` leaves; ``hang`` = (k, depth): its lowest cherry is replaced by a balanced k-ary conflict tree."""
    if hang is None:
        L = n_taxa
        # internal i joins (i == 0: leaves 0, 1; else internal i-1 and leaf i+1)
        parents = [0, 0] + list(range(1, L - 1)) + list(range(1, L - 1)) + [-1]
        return np.array(parents, dtype=np.int64), L
    bp, bl = balanced_tree(*hang)
    bi = len(bp) - bl
    L = bl + n_taxa
    I = bi + n_taxa
    leaf_par = list(bp[:bl]) + [bi + j for j in range(n_taxa)]
    int_par = list(bp[bl:-1]) + [bi + j for j in range(n_taxa)] + [-1]
    assert len(int_par) == I
    return np.array(leaf_par + int_par, dtype=np.int64), L


def near_identity(rng, B, D, eps, spread=True):
    """[B, D, D] row-stochastic matrices with off-diagonal entries around ``eps`` (per branch x0.5 .. x2, per entry x0.5 .. x1.5)."""
    e = np.broadcast_to(np.asarray(eps, dtype=np.float64), (B,))
    off = e[:, None, None] * np.ones((B, D, D))
    if spread:
        off = off * rng.uniform(0.5, 2.0, size=(B, 1, 1)) * rng.uniform(0.5, 1.5, size=(B, D, D))
    idx = np.arange(D)
    off[:, idx, idx] = 0.0
    off[:, idx, idx] = 1.0 - off.sum(axis=2)
    assert off.min() >= 0.0
    return off


def ordinary(rng, B, D):
    """[B, D, D] row-stochastic matrices of branches of ordinary length (diagonal 0.6 .. 0.95)."""
    M = rng.random((B, D, D)) + 0.05
    idx = np.arange(D)
    M[:, idx, idx] = 0.0
    M = M / M.sum(axis=2, keepdims=True) * rng.uniform(0.05, 0.4, size=(B, 1, 1))
    M[:, idx, idx] = 1.0 - M.sum(axis=2)
    return M


def _patterns(rng, L, D, S, k, ambig_n=2):
    """Leaf codes [L, S]: in every group of 16 consecutive patterns a conserved one, a fully conflicting one (siblings differ), one
    with ambiguity codes and random ones; the rest of the group cycles through these kinds."""
    codes = np.zeros((L, S), dtype=np.int64)
    j = np.arange(L)
    for s in range(S):
        kind = s % 4
        if kind == 0:
            codes[:, s] = rng.integers(D)
        elif kind == 1:
            codes[:, s] = (j + j // k + s) % D
        elif kind == 2:
            codes[:, s] = (j * 7 + s) % D
            m = rng.random(L) < 0.2
            codes[m, s] = -rng.integers(1, ambig_n + 1, size=int(m.sum()))
        else:
            codes[:, s] = rng.integers(0, D, size=L)
    return codes


def _case(name, D, fp, L, codes, P, rng, ambig_n=2, **extra):
    ambig = (rng.random((ambig_n, D)) < 0.5).astype(np.float64)
    ambig[:, 0] = 1.0
    ambig[0, :] = 1.0        # a full gap
    S = codes.shape[1]
    pi = extra.pop("root_freqs", None)
    if pi is None:
        pi = np.full(D, 1.0 / D)
    return dict(name=name, D=np.int64(D), L=np.int64(L), flat_parents=np.asarray(fp, dtype=np.int64), leaf_codes=codes, ambig=ambig,
                pattern_freq=rng.integers(1, 4, size=S).astype(np.int64), root_freqs=np.asarray(pi, dtype=np.float64), P=P, **extra)


def _block_zero(P, D):
    """Make the last state unreachable from the others and the others unreachable from it (exact zeros, rows still sum to one)."""
    P = P.copy()
    P[:, : D - 1, D - 1] = 0.0
    P[:, D - 1, : D - 1] = 0.0
    idx = np.arange(D)
    P[:, idx, idx] = 0.0
    P[:, idx, idx] = 1.0 - P.sum(axis=2)
    return P


def threshold_node_sum(D, states, eps):
    """Sum over i of prod_c P[i, states[c]] for the uniform near-identity matrix with off-diagonal ``eps``: a node above leaves
    alone, in the oracle's left-to-right arithmetic."""
    P = np.full((D, D), eps)
    P[np.arange(D), np.arange(D)] = 1.0 - (D - 1) * eps
    v = np.ones(D)
    for s in states:
        v = v * P[:, s]
    tot = 0.0
    for x in v:
        tot += x
    return tot


THRESHOLD_STATES = (0, 1, 2, 3, 0, 1)


def _threshold_eps(D, side):
    """Bisect ``eps`` so that threshold_node_sum is the largest value below 2^-64 (side < 0) or the smallest at or above it."""
    lo, hi = 1e-8, 1e-2
    assert threshold_node_sum(D, THRESHOLD_STATES, lo) < 2.0 ** -64 <= threshold_node_sum(D, THRESHOLD_STATES, hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if threshold_node_sum(D, THRESHOLD_STATES, mid) < 2.0 ** -64:
            lo = mid
        else:
            hi = mid
    return lo if side < 0 else hi


EPS = (1e-3, 1e-6, 1e-10, 1e-15, 1e-20, 1e-30)
# (children per node, depth, D, eps) of the conflict trees on which a numpy model of the former thinning rule loses the likelihood
# (zero, or denormal digits) while a test at every node with up to 15 steps keeps it; candidates like any other
TABLE_ROWS = ((4, 3, 4, 1e-30), (4, 3, 61, 1e-20), (4, 3, 61, 1e-30), (4, 4, 61, 1e-15), (4, 4, 4, 1e-30))


def _name_eps(eps):
    return f"{eps:.0e}".replace("e-0", "e-").replace("e-", "em")


# Candidates on which the REFERENCE's own scheme is not accurate (oracle/hyphy_oracle.c against ``prune``: -inf or NaN where the
# likelihood is finite), found by test_scalefree_cpu.py and taken out here, not skipped at run time.  The reference does not test a
# node that has only resolved leaves below it and stops rescaling a (node, pattern) once its factor reaches sqrt(DBL_MAX * 1e-10)
# ~ 2^507, i.e. after seven steps: above three or more children whose conditionals sit near eps^(k-1) each it runs out of steps and
# the next product underflows.  All of TABLE_ROWS are among them: a model that tests every node with up to 15 steps keeps them,
# the reference does not test that way.  (The kernels use 15 steps at every node and may well be right on these; without an
# accurate reference-scheme value they cannot be part of this list.)  The enumeration below passes over these names (their seeds
# stay used up, so taking a case out does not change the others).
REFERENCE_FAILS = frozenset("""
conflict_k3_d4_D20_1em30 conflict_k3_d4_D61_1em30 conflict_k3_d4_D64_1em30 conflict_k4_d3_D4_1em30 conflict_k4_d3_D20_1em30
conflict_k4_d3_D61_1em30 conflict_k4_d3_D61_1em20 conflict_k4_d3_D64_1em30 conflict_k4_d4_D4_1em30 conflict_k4_d4_D4_1em20
conflict_k4_d4_D20_1em30 conflict_k4_d4_D20_1em15 conflict_k4_d4_D61_1em30 conflict_k4_d4_D61_1em20 conflict_k4_d4_D61_1em15
conflict_k4_d4_D64_1em30 conflict_k4_d4_D64_1em15 conflict_k5_d3_D4_1em30 conflict_k5_d3_D4_1em20 conflict_k5_d3_D4_1em15
conflict_k5_d3_D20_1em30 conflict_k5_d3_D20_1em15 conflict_k5_d3_D61_1em30 conflict_k5_d3_D61_1em20 conflict_k5_d3_D61_1em15
conflict_k5_d3_D61_1em10 conflict_k5_d3_D64_1em30 conflict_k5_d3_D64_1em15
""".split())


def rescale_edge_cases():
    return list(_enumerate_cases())


def _enumerate_cases():
    """The fixed list of named, seeded cases (dicts with the golden fixtures' keys plus "name" and "P" [B, D, D] — "P" [C, B, D, D]
    and "weights" for the rate-class case).  Every matrix is row-stochastic: pass with q_is_probability=True.
    The list is enumerated here and filtered nowhere else: a case on which the reference's own scheme is not accurate to 1e-12 per
    pattern (test_scalefree_cpu.py) is taken out by adding its name to REFERENCE_FAILS, with the reason, and is then not built."""
    seed = 0

    def rng_for():
        nonlocal seed
        seed += 1
        return np.random.default_rng(9000 + seed)

    # -- conflict trees
    shapes = {2: (6, 8), 3: (4,), 4: (3, 4), 5: (3,)}       # 64 / 256, 81, 64 / 256, 125 taxa
    wanted = set()
    for k, depths in shapes.items():
        for d in depths:
            for D in (4, 20, 61, 64):
                for e in EPS:
                    # the full product is kept at D = 4 and 61; D = 20 and 64 take the two ends and the middle
                    if D in (20, 64) and e not in (1e-3, 1e-15, 1e-30):
                        continue
                    if k in (2, 3) and d == shapes[k][-1] and D in (20, 64) and e == 1e-15:
                        continue
                    if k == 2 and d == 8 and e in (1e-6, 1e-10, 1e-20):
                        continue
                    wanted.add((k, d, D, e))
    for row in TABLE_ROWS:
        wanted.add(row)
    for (k, d, D, e) in sorted(wanted):
        rng = rng_for()
        name = f"conflict_k{k}_d{d}_D{D}_{_name_eps(e)}"
        if name in REFERENCE_FAILS:
            continue
        fp, L = balanced_tree(k, d)
        S = 24 if L <= 128 else 20
        codes = _patterns(rng, L, D, S, k)
        yield _case(name, D, fp, L, codes, near_identity(rng, len(fp) - 1, D, e), rng)

    # -- mixed tiles: conserved / conflicting / ambiguous / impossible in every 16 patterns; S not a multiple of 16, several tiles
    for (D, k, d, e, S) in ((4, 4, 3, 1e-20, 37), (61, 4, 3, 1e-15, 53), (20, 2, 6, 1e-30, 70), (64, 3, 4, 1e-10, 41), (4, 2, 6, 1e-6, 300)):
        rng = rng_for()
        fp, L = balanced_tree(k, d)
        codes = _patterns(rng, L, D, S, k)
        P = _block_zero(near_identity(rng, len(fp) - 1, D, e), D)
        for s in range(5, S, 16):          # impossible: the isolated state at one leaf, another state at its sibling
            codes[:, s] = (np.arange(L) + s) % (D - 1)
            codes[0, s] = D - 1
        for s in range(9, S, 16):          # possible: the isolated state everywhere (or ambiguous)
            codes[:, s] = D - 1
            codes[3, s] = -1
        pi = rng.random(D) + 0.1
        yield _case(f"mixed_D{D}_k{k}_{_name_eps(e)}_S{S}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum())

    # -- several steps at one node: a star of n leaf children below the root, next to a cherry
    for (D, n, e) in ((4, 6, 3e-9), (4, 8, 1e-9), (61, 9, 2e-8), (20, 12, 1e-6), (64, 12, 5e-6), (61, 10, 1e-7)):
        rng = rng_for()
        L = n + 2
        fp = np.array([0] * n + [1, 1] + [2, 2, -1], dtype=np.int64)
        S = 21
        codes = _patterns(rng, L, D, S, n)
        yield _case(f"star_D{D}_n{n}_{_name_eps(e)}", D, fp, L, codes, near_identity(rng, len(fp) - 1, D, e, spread=False), rng)

    # -- at the threshold: a node above six leaves whose sum is the float next to 2^-64, on either side
    for D in (4, 61):
        for side in (-1, 1):
            rng = rng_for()
            states = list(THRESHOLD_STATES)
            e = _threshold_eps(D, side)
            L = 8
            fp = np.array([0] * 6 + [1, 1] + [2, 2, -1], dtype=np.int64)
            S = 19
            codes = np.zeros((L, S), dtype=np.int64)
            for s in range(S):                                   # the same multiset of states, rotated: sums a few ulps apart
                codes[:6, s] = (np.array(states) + s) % 4
                codes[6:, s] = s % 4
            P = near_identity(rng, len(fp) - 1, D, e, spread=False)
            yield _case(f"threshold_D{D}_{'below' if side < 0 else 'above'}", D, fp, L, codes, P, rng)

    # -- ladders: many single steps; deeper than the walk's stack; hung off a 4-way conflict tree
    for (D, n, hang) in ((4, 300, None), (61, 300, None), (20, 600, None), (61, 600, None), (61, 120, (4, 3)), (4, 200, (4, 3))):   # (the D = 61 one at 1e-15: at 1e-20 the reference fails, as above)
        rng = rng_for()
        fp, L = ladder_tree(n, hang)
        S = 20
        codes = _patterns(rng, L, D, S, 4)
        P = ordinary(rng, len(fp) - 1, D)
        if hang:
            bp, bl = balanced_tree(*hang)
            nb = len(bp) - 1
            Pn = near_identity(rng, nb, D, 1e-15 if D == 61 else 1e-20)
            P[:bl] = Pn[:bl]
            P[L: L + nb - bl] = Pn[bl:]
        tag = f"ladder_D{D}_{n}" + (f"_on_k{hang[0]}d{hang[1]}" if hang else "")
        yield _case(tag, D, fp, L, codes, P, rng)

    # -- classes far apart: three rate classes with off-diagonals 1e-2, 1e-12, 1e-30
    for (D, k, d) in ((61, 2, 6), (4, 3, 4), (20, 2, 6)):   # (4 children per node at 1e-30: the reference fails, as above)
        rng = rng_for()
        fp, L = balanced_tree(k, d)
        S = 24
        codes = _patterns(rng, L, D, S, k)
        B = len(fp) - 1
        P = np.stack([near_identity(rng, B, D, e, spread=D * e < 0.3) for e in (1e-2, 1e-12, 1e-30)])
        yield _case(f"classes_D{D}_k{k}", D, fp, L, codes, P, rng, weights=np.array([0.5, 0.3, 0.2]))


def cases_by_name():
    return {c["name"]: c for c in rescale_edge_cases()}


# the named subset the secondary paths run (conflict trees next to the table's rows, one mixed-tile case, one ladder)
# — of the table's rows the reference only sustains the neighbours at the next larger eps, which stand in for them
SUBSET = ("conflict_k4_d3_D4_1em20", "conflict_k4_d3_D61_1em15", "conflict_k4_d4_D61_1em10", "conflict_k4_d4_D4_1em15",
          "conflict_k5_d3_D61_1em6", "conflict_k2_d8_D61_1em30", "mixed_D61_k4_1em15_S53", "ladder_D61_300")
