"""The references behind hyphy_hip_branch_sensitivities / _gradient / _gradient_built and hyphy_hip_expm_frechet_adjoint_batch.

``outside`` is tests/deriv_cases.py's longdouble recursion once more, keeping per branch the conditional below it as well:
(V_c, E_c = P_c in_c, log of what was divided out of V_c and in_c together, in_c).  ``sensitivities`` forms per class
    W_c[i][j] = sum_s f_s w_c V[s, i] in[s, j] exp(lm_c[s] - top[s]) / Lmix[s],     Lmix = sum_c w_c (V . E)_c exp(lm_c - top)
in longdouble (``top``: the largest lm among the classes that are not exactly zero at the pattern; a class that is, or has weight 0,
contributes nothing and does not move ``top``).  All terms are >= 0, so the allowance is componentwise:
    |dW_ij| <= (GPU_RTOL + S 2^-53) W_ij + 1e-280,   and an entry that is zero here must be exactly zero.

``frechet_ref`` is S = L(Q^T, W), L(A, E) = int_0^1 e^{sA} E e^{(1-s)A} ds, in 192-bit fixed point (57 digits) on Python integers: the
Taylor pair of exp and its derivative on A / 2^p until the terms vanish, then p squarings.  tests/test_grad_cases_cpu.py holds it to
mpmath's exponential of the block matrix [[Q^T, W], [0, Q^T]] at 50 digits (whose upper-right block is L(Q^T, W)) where that is
affordable (a 2D x 2D mpmath product takes 2.6 s at D = 64, an exponential a hundred of them; the integer form 0.02 s a product).
``frechet_model`` restates the device's algorithm in float64: A = Q^T, p the least integer with ||A||_inf / 2^p <= 1/4, degree 13,
A_j = A_{j-1} X / j, D_j = (D_{j-1} X + A_{j-1} E') / j, then p times L <- P L + L P, P <- P P.

Largest deviation of ``frechet_model`` from ``frechet_ref`` per entry, in units of max |W|, over ``adjoint_cases`` at D = 4, 5, 16,
17, 20 (test_grad_cases_cpu.py::test_frechet_model_against_extended_precision prints them):
    matrices that need no squaring     4.15e-16   (MODEL_DEV_PLAIN = 4.2e-16)
    matrices that need squarings       6.30e-14   (MODEL_DEV_SQUARED = 6.4e-14; at ||Q|| = 200, ten squarings)
The device's allowance per entry is four times these (the margin the project gave its exponentials over the oracle's own deviation),
never less than the exponentials' own bars: 2e-15 without squarings, 5e-14 with."""
import functools
import math

import numpy as np

from tests import branchcache_cases as bc
from tests import deriv_cases as dc
from tests import scalefree as sf

RTOL = sf.GPU_RTOL
MISTAKES = ("w_transposed", "q_not_transposed", "e_for_in", "no_one_over_l", "no_diagonal_chain", "unaligned", "u_for_v")
TAYLOR_DEGREE = 13
MODEL_DEV_PLAIN = 4.2e-16     # measured, see the docstring
MODEL_DEV_SQUARED = 6.4e-14
ALLOW_PLAIN = max(4 * MODEL_DEV_PLAIN, 2e-15)
ALLOW_SQUARED = max(4 * MODEL_DEV_SQUARED, 5e-14)
GOLDEN_D = (48, 49, 61, 64)      # frechet_ref of adjoint_cases(D) is stored (tools/make_frechet_golden.py)
ADJOINT_KINDS = ("zero", "tiny", "quarter", "three", "two_hundred", "sparse", "w_spread")


# ---- the outside pass with in_c ---------------------------------------------------------------------------------------------------

def outside(cs, P=None, ft=np.longdouble, mistake=None):
    """Per branch c of one class: (V_c [S, D], E_c [S, D], log divided out of V_c and in_c together [S], in_c [S, D])."""
    o = dc.outside(cs, P, ft, mistake="u_for_v" if mistake == "u_for_v" else None)
    D, L = int(cs["D"]), int(cs["L"])
    P = np.asarray(cs["P"] if P is None else P).astype(ft)
    S = np.asarray(cs["leaf_codes"]).shape[1]
    ch = sf.children_of(np.asarray(cs["flat_parents"], dtype=np.int64), L)
    cond, ins = [None] * len(ch), {}
    for n in range(len(ch)):                              # deriv_cases.outside's inside pass, keeping what enters each branch
        v, acc = np.ones((S, D), dtype=ft), np.zeros(S, dtype=ft)
        for c in ch[n]:
            ins[c] = cond[c - L] if c >= L else dc._leaf_vectors(cs, c, ft)
            v, acc = dc._norm(v * (ins[c] @ P[c].T), acc)
        cond[n] = v
    return {c: (o[c][0], o[c][1], o[c][2], ins[c]) for c in o}


_outs = {}


def outs_of(cs):
    """The longdouble ``outside`` of every class of the case, computed once per case name."""
    if cs["name"] not in _outs:
        P = np.asarray(cs["P"])
        _outs[cs["name"]] = [outside(cs)] if P.ndim == 3 else [outside(cs, P[c]) for c in range(P.shape[0])]
    return _outs[cs["name"]]


def sensitivities(cs, outs, node, weights=None, mistake=None):
    """dict(W [C, D, D] longdouble, allow [C, D, D], n_skipped) of branch ``node``."""
    f = np.asarray(cs["pattern_freq"], dtype=np.float64)
    w = np.ones(1) if weights is None else np.asarray(weights, dtype=np.float64)
    ft = outs[0][node][0].dtype
    l0 = [(o[node][0] * o[node][1]).sum(axis=1) for o in outs]
    lm = np.stack([o[node][2] for o in outs])
    live = np.stack([(w[c] != 0) & (l0[c] != 0) for c in range(len(outs))])
    with np.errstate(invalid="ignore"):
        top = np.where(live, lm, -np.inf).max(axis=0)
    top = np.where(np.isfinite(top), top, 0)
    sc = []
    for c in range(len(outs)):
        with np.errstate(invalid="ignore", over="ignore"):
            sc.append(np.where(live[c], 1.0 if mistake == "unaligned" else np.exp(np.where(live[c], lm[c] - top, 0)), 0).astype(ft))
    Lmix = sum(w[c] * sc[c] * l0[c] for c in range(len(outs)))
    ok = Lmix != 0
    use = ok & (f > 0)
    den = np.ones_like(Lmix) if mistake == "no_one_over_l" else np.where(ok, Lmix, 1)
    Ws = []
    for c, o in enumerate(outs):
        V, E, _, inn = o[node]
        g = np.where(use & live[c], f.astype(ft) * w[c] * sc[c] / den, 0)
        Wc = (V * g[:, None]).T @ (E if mistake == "e_for_in" else inn)
        Ws.append(Wc.T if mistake == "w_transposed" else Wc)
    W = np.stack(Ws)
    return dict(W=W, allow=(RTOL + len(f) * 2.0 ** -53) * W + 1e-280, n_skipped=int(np.sum((~ok) & (f > 0))))


def miss_w(got, ref):
    """Largest deviation / allowance of a [C, D, D] block (inf where an exact zero is missed or NaN appears)."""
    got = np.asarray(got).reshape(ref["W"].shape)
    if np.isnan(got).any():
        return np.inf
    zero = ref["W"] == 0
    if np.any(got[zero] != 0):
        return np.inf
    dev = np.abs(got - ref["W"]).astype(np.float64)
    return float(np.max(dev / ref["allow"].astype(np.float64)))


# ---- the adjoint of the exponential's Frechet derivative ---------------------------------------------------------------------------

def squarings(Q):
    """p of the device's scaling: the least p >= 0 with ||Q^T||_inf / 2^p <= 1/4, by its loop."""
    s, p = float(np.abs(np.asarray(Q, dtype=np.float64).T).sum(axis=1).max()), 0
    while s > 0.25:
        s, p = s * 0.5, p + 1
    return p


def frechet_model(Q, W, q_not_transposed=False):
    """The device's algorithm in float64 numpy."""
    Q, W = np.asarray(Q, dtype=np.float64), np.asarray(W, dtype=np.float64)
    A = Q if q_not_transposed else Q.T
    p = squarings(A.T)
    X, E = A * 2.0 ** -p, W * 2.0 ** -p
    Aj, Dj = X.copy(), E.copy()
    SA, SD = np.eye(len(Q)) + X, E.copy()
    for j in range(2, TAYLOR_DEGREE + 1):
        Dj, Aj = (Dj @ X + Aj @ E) / j, (Aj @ X) / j
        SA, SD = SA + Aj, SD + Dj
    for _ in range(p):
        SD, SA = SA @ SD + SD @ SA, SA @ SA
    return SD


_BITS = 192


def _fix(M):
    def one(x):
        if x == 0:
            return 0
        m, e = math.frexp(float(x))
        v, sh = int(m * 2 ** 53), _BITS + e - 53
        return v << sh if sh >= 0 else v >> -sh
    return np.array([one(x) for x in np.asarray(M, dtype=np.float64).ravel()], dtype=object).reshape(np.shape(M))


def _mul(a, b):
    return a.dot(b) // (1 << _BITS)


def _pair(A, E, p):
    """Fixed point: (exp(A), L(A, E)) with A / 2^p and E / 2^p entering the Taylor pair, then p squarings."""
    X, E = _fix(A * 2.0 ** -p), _fix(E) // (1 << p)
    n = len(A)
    eye = np.array([[(1 << _BITS) if i == j else 0 for j in range(n)] for i in range(n)], dtype=object)
    Aj, Dj = X.copy(), E.copy()
    SA, SD = eye + X, E.copy()
    lean = not E.any()                                    # (the exponential alone: a third of the products)
    for j in range(2, 80):
        if not lean:
            Dj = (_mul(Dj, X) + _mul(Aj, E)) // j
        Aj = _mul(Aj, X) // j
        SA, SD = SA + Aj, SD + Dj
        if not Aj.any() and not Dj.any():
            break
    for _ in range(p):
        if not lean:
            SD = _mul(SA, SD) + _mul(SD, SA)
        SA = _mul(SA, SA)
    return SA, SD


def frechet_ref(Q, W, q_not_transposed=False):
    """L(Q^T, W) in 192-bit fixed point, rounded to float64."""
    Q, W = np.asarray(Q, dtype=np.float64), np.asarray(W, dtype=np.float64)
    A = Q if q_not_transposed else Q.T
    SD = _pair(A, W, squarings(A.T) + 3)[1]                # ||X||_inf <= 1/32: the series is short
    return np.array([math.ldexp(float(v), -_BITS) for v in SD.ravel()], dtype=np.float64).reshape(Q.shape)


def expm_fixed(Q):
    """exp(Q) in 192-bit fixed point, rounded to longdouble (64 fraction bits: entries of a transition matrix)."""
    Q = np.asarray(Q, dtype=np.float64)
    SA = _pair(Q, np.zeros_like(Q), squarings(Q.T) + 3)[0]
    def one(v):
        hi = v >> (_BITS - 32)
        mid = (v - (hi << (_BITS - 32))) >> (_BITS - 64)
        return (np.longdouble(float(hi)) + np.longdouble(float(mid)) / np.longdouble(2.0 ** 32)) / np.longdouble(2.0 ** 32)
    return np.array([one(v) for v in SA.ravel()], dtype=np.longdouble).reshape(Q.shape)


def frechet_mpmath(Q, W, dps=50):
    """The upper-right block of exp([[Q^T, W], [0, Q^T]]) by mpmath at ``dps`` digits, rounded to float64 (small D only)."""
    import mpmath as mp
    D = len(Q)
    with mp.workdps(dps):
        M = mp.zeros(2 * D)
        for i in range(D):
            for j in range(D):
                M[i, j] = M[D + i, D + j] = mp.mpf(float(Q[j][i]))
                M[i, D + j] = mp.mpf(float(W[i][j]))
        X = mp.expm(M, method="taylor")
        return np.array([[float(X[i, D + j]) for j in range(D)] for i in range(D)])


def random_rates(rng, D, density=1.0):
    """A rate matrix: non-negative, not reversible, diagonal -(row sum)."""
    M = (rng.random((D, D)) + 0.05) * (rng.random((D, D)) < density)
    M[np.arange(D), np.arange(D)] = 0.0
    if not M.any():
        M[0, 1] = 1.0
    M[np.arange(D), np.arange(D)] = -M.sum(axis=1)
    return M


def _scaled(Q, norm):
    n = np.abs(Q.T).sum(axis=1).max()
    return Q * (norm / n)


@functools.lru_cache(maxsize=None)
def adjoint_cases(D, n=3):
    """[(kind, Q [n, D, D], W [n, D, D])] in ADJOINT_KINDS' order: Q = 0; ||Q^T||_inf = 1e-13; 0.2 (no squaring); 3; 200 (ten
    squarings); a 10 %-dense MG94-like matrix of norm 1; and at norm 3 a W with zeros and entries spread over 1e-13 .. 1."""
    rng = np.random.default_rng([7700, D])
    out = []
    for kind in ADJOINT_KINDS:
        Q = np.stack([random_rates(rng, D, 0.1 if kind == "sparse" else 1.0) for _ in range(n)])
        norm = dict(zero=0.0, tiny=1e-13, quarter=0.2, three=3.0, two_hundred=200.0, sparse=1.0, w_spread=3.0)[kind]
        Q = np.stack([_scaled(q, norm) for q in Q])
        W = rng.random((n, D, D)) + 0.1
        if kind == "w_spread":
            W = 10.0 ** (-13.0 * rng.random((n, D, D))) * (rng.random((n, D, D)) < 0.7)
            W[:, 0, 0] = 1.0
        out.append((kind, Q, W))
    return out


def adjoint_allowance(Q, W):
    """Per entry: ALLOW_PLAIN or ALLOW_SQUARED times max |W|."""
    return (ALLOW_SQUARED if squarings(Q) > 0 else ALLOW_PLAIN) * float(np.abs(W).max())


# ---- the chain to the coefficients -------------------------------------------------------------------------------------------------

def build_q(T, x):
    Q = np.einsum("k,kij->ij", np.asarray(x, dtype=np.float64), np.asarray(T, dtype=np.float64))
    D = len(Q)
    Q[np.arange(D), np.arange(D)] = 0.0
    Q[np.arange(D), np.arange(D)] = -Q.sum(axis=1)
    return Q


def chain(S, T, mistake=None):
    """grad_k = sum_{i != j} T_k[i][j] (S[i][j] - S[i][i])."""
    S = np.asarray(S)
    D = S.shape[-1]
    off = ~np.eye(D, dtype=bool)
    d = S - (0 if mistake == "no_diagonal_chain" else np.diagonal(S)[:, None])
    return np.array([np.sum((np.asarray(Tk) * d)[off]) for Tk in T])


def chain_allowance(aS, T):
    """sum_{i != j} |T_k[i][j]| (a_ij + a_ii)."""
    D = aS.shape[-1]
    off = ~np.eye(D, dtype=bool)
    return np.array([np.sum((np.abs(Tk) * (aS + np.diagonal(aS)[:, None]))[off]) for Tk in T])


def gradient(cs, outs, node, Qs, weights=None, T=None, mistake=None):
    """dict(S [C, D, D], allow_S, grad [C, K], allow_grad (with T), n_skipped): W by ``sensitivities``, S = L(Q_c^T, W_c) by
    ``frechet_ref``.  The allowance of S: W's share L(Q^T, allow_W) (the kernel of L(Q^T, .) is non-negative for a rate matrix) plus
    the adjoint's own, per entry."""
    ref = sensitivities(cs, outs, node, weights, mistake)
    S, aS = [], []
    for c, Q in enumerate(Qs):
        Wc = ref["W"][c].astype(np.float64)
        S.append(frechet_ref(Q, Wc, q_not_transposed=mistake == "q_not_transposed"))
        aS.append(frechet_model(Q, ref["allow"][c].astype(np.float64)) * (1 + 1e-9) + adjoint_allowance(Q, Wc))
    out = dict(S=np.stack(S), allow_S=np.stack(aS), n_skipped=ref["n_skipped"], W=ref["W"])
    if T is not None:
        out["grad"] = np.stack([chain(s, T, mistake) for s in S])
        out["allow_grad"] = np.stack([chain_allowance(a, T) for a in aS])
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

def _tree_case(name, D, tree, S, seed, ambig_leaves=(3, 9), zero_freq=7):
    rng = np.random.default_rng(seed)
    fp, L = tree
    codes = bc._mixed_patterns(rng, fp, L, D, S, 4, lambda l: l in ambig_leaves, seed % 2 == 1)
    P = bc._matrices(rng, fp, L, D, None)
    pi = rng.random(D) + 0.1
    cs = sf._case(name, D, fp, L, codes, P, rng, root_freqs=pi / pi.sum())
    cs["pattern_freq"][zero_freq] = 0
    cs["seed"] = seed
    cs["branches"] = list(range(len(fp) - 1))
    return cs


@functools.lru_cache(maxsize=None)
def bal_case(D, S=40):
    """The 16-taxon balanced tree at ``D`` states and ``S`` patterns (40: three tiles, the last one padded): leaves 3 and 9 carry
    ambiguity codes, pattern 7 has frequency 0, the isolated state and (odd D) patterns impossible at build time as in
    branchcache_cases, matrices with exact zeros at the closed leaves, a random pi."""
    return _tree_case(f"grad_bal2x4_D{D}_S{S}", D, sf.balanced_tree(2, 4), S, 7900 + D)


@functools.lru_cache(maxsize=None)
def star_case(D=20):
    """A 41-child star node."""
    return _tree_case(f"grad_star41_D{D}", D, bc.star_tree(40), 20, 7960 + D)


def forward_terms(cs, outs, node, Qs, T, weights=None):
    """[C, K, S] per-pattern terms of d log L / d x_k in the forward form: g_s V_s^T L(Q, dQ/dx_k) in_s, float64 (their f-weighted
    sums are the gradient once more; the sums of their magnitudes scale the bar of the central differences)."""
    f = np.asarray(cs["pattern_freq"], dtype=np.float64)
    w = np.ones(1) if weights is None else np.asarray(weights, dtype=np.float64)
    l0 = [(o[node][0] * o[node][1]).sum(axis=1) for o in outs]
    lm = np.stack([o[node][2] for o in outs])
    live = np.stack([(w[c] != 0) & (l0[c] != 0) for c in range(len(outs))])
    top = np.where(live, lm, -np.inf).max(axis=0)
    top = np.where(np.isfinite(top), top, 0)
    sc = [np.where(live[c], np.exp(np.where(live[c], lm[c] - top, 0)), 0) for c in range(len(outs))]
    Lmix = sum(w[c] * sc[c] * l0[c] for c in range(len(outs)))
    ok = (Lmix != 0) & (f > 0)
    out = np.zeros((len(outs), len(T), len(f)))
    for c, o in enumerate(outs):
        V, _, _, inn = o[node]
        g = np.where(ok & live[c], w[c] * sc[c] / np.where(Lmix != 0, Lmix, 1), 0)
        for k, Tk in enumerate(T):
            M = frechet_model(np.asarray(Qs[c]).T, build_q([Tk], [1.0]))      # L(Q, dQ / dx_k)
            out[c, k] = np.asarray(g * ((V @ M) * inn).sum(axis=1), dtype=np.float64)
    return out


def ladder_template_case(K=2):
    """deriv_cases.ladder_class_case's tree, patterns and weights with P_c = exp(Q_c): templates and coefficient rows per class, the
    classes' coefficients scaled by 1, 1e-2 and 1e-3 (off-diagonals down to 1e-5: the classes' exponents differ and live in in_c; a
    smaller class could not be held to central differences of a longdouble log L at a relative step of 1e-6).
    Returns (cs, T, x [C, B, K], Q [C, B, D, D])."""
    from tests import expm_ref
    cs = dict(dc.ladder_class_case())
    T, x0, _ = template_model(cs, K, 3, zero_rows=False, tiny=False)
    x = np.stack([x0 * s for s in (1.0, 1e-2, 1e-3)])
    Q = np.stack([np.stack([build_q(T, xb) for xb in xc]) for xc in x])
    cs["P"] = np.stack([np.stack([expm_ref.reference(q) for q in Qc]) for Qc in Q])
    cs["name"] = f"grad_ladder40_classes_D20_K{K}"
    return cs, T, x, Q


def built_case(D, K, seed=1, **kw):
    """``bal_case(D)`` with P_b = exp(Q_b) of ``template_model``: (cs, T, x [B, K], Q [B, D, D])."""
    from tests import expm_ref
    cs = dict(bal_case(D))
    T, x, Q = template_model(cs, K, seed, **kw)
    cs["P"] = np.stack([expm_ref.reference(q) for q in Q])
    cs["name"] = f"{cs['name']}_K{K}_{seed}"
    return cs, T, x, Q


def template_model(cs, K, seed, lo=0.01, hi=0.05, zero_rows=True, tiny=True):
    """(T [K, D, D], x [B, K], Q [B, D, D]): random non-negative templates (not reversible; with ``zero_rows`` the last template has
    two all-zero rows), coefficients in [lo, hi] with x[0, 0] = 1e-13 (``tiny``), and the rate matrices build_q forms."""
    D, B = int(cs["D"]), len(cs["flat_parents"]) - 1
    rng = np.random.default_rng([int(cs["seed"]), K, seed])
    T = (rng.random((K, D, D)) + 0.05) * (rng.random((K, D, D)) < 0.5)
    T[:, np.arange(D), np.arange(D)] = 0.0
    if zero_rows:
        T[K - 1, [0, D - 1], :] = 0.0
    x = rng.uniform(lo, hi, size=(B, K))
    if tiny:
        x[0, 0] = 1e-13
    return T, x, np.stack([build_q(T, x[b]) for b in range(B)])
