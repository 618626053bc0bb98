"""A componentwise-accurate reference for the per-site fits (sitefit.hip), and the cases on which that kernel can go wrong.

The kernel applies exp(Q_{b,s}) to a vector by uniformisation and never forms a matrix.  This reference forms every matrix.  It
is uniformisation too (R = I + Q / mu), but with a relative, per-entry stopping rule, squarings and no 2^64 scheme; what makes it
independent is that tests/test_sitefit_ref_cpu.py pins it, entry by entry, to mpmath at 50 digits:

``transition(Q)``: mu = max_i |Q_ii|, R = I + Q / mu (entrywise >= 0; its diagonal is formed as (mu - d_i) / mu from the row sums d_i
of the off-diagonal entries), s with h = mu / 2^s <= 1, E = e^-h sum_j h^j R^j / j! summed until a further term changes no entry
(relative, per entry: no absolute cut-off, so an entry first reached after d steps of R is summed from its own leading term on),
then s squarings.  Every operation adds or multiplies non-negative numbers; an exact zero appears only where the sparsity graph has
no path.  Arithmetic is float64 by default: with J terms and D states an entry carries at most 2^s (J (D + 2) + D) u relative
error, u = 2^-53 (every non-negative dot product of length D: D u; every squaring doubles what it is given and adds D u) —
``transition_bound``.  ``extended=True`` runs the same in ``np.longdouble``; on the x86-64 hosts this was written on that is the
80-bit format (u = 2^-64, 5.4e-20) and a 61 x 61 product takes 1.5 ms against 25 us, which is why it is the check
(tests/test_sitefit_ref_cpu.py pins both to mpmath at 50 digits) and not the default.

``site_fit_logl``: per site Q_b = sum_k m[s][g(b)][k] c[b][k] T_k, for mixtures sum_m w_m transition(Q_b^(m)), pruned by
tests/scalefree.prune (no 2^64 scheme), -inf where the likelihood is exactly zero.

Largest relative deviation of the oracle route (one OraclePartition per site fed oracle.expm matrices, the route of
tests/test_gpu_parity.py::test_site_fits_*) from this reference over ``cases()``, patterns where the oracle route is finite,
measured by tests/test_sitefit_ref_cpu.py::test_oracle_route_agrees_where_it_is_finite (|dev| / max(1, |ref|)):

    ORACLE_MAX_REL         = 0.39       (0.381 measured, mg94_alpha0)
    ORACLE_MAX_REL_SHALLOW = 2e-10      (1.77e-10 measured, shape_D64; every case outside oracle_deep)

``oracle_deep(name)`` marks the cases whose patterns need entries five and more steps of the rate matrix away on short branches: the chain
templates, and the two cases with a template switched off (mg94_alpha0: 0.381, dense_off_chain20: 0.258, chain20_far: 0.066).

oracle.expm (Taylor with the negative diagonal, then squarings) is accurate in absolute terms only: an entry that needs more than
a few substitutions on a short branch lies below its rounding noise, so on the oracle_deep cases (5 .. 19 steps between the leaves
of a pattern) the oracle route is no yardstick, and on the other templates it is one to 1e-10, not to the rounding unit.  That is
why the GPU tests of these cases use this reference and not the oracle route, at the bar the entry point already carries:
|got - ref| <= 1e-9 max(1, |ref|) per site (tests/test_gpu_parity.py::test_site_fits_match_per_site_reference).

Node numbering as in tests/scalefree.py: leaf l has node code l, internal node i has code L + i; branch b is the one above code b.
"""
import types

import numpy as np

from tests import scalefree as sf

ORACLE_MAX_REL = 0.39                # over the whole list (mg94_alpha0)
ORACLE_MAX_REL_SHALLOW = 2e-10       # over the cases outside oracle_deep (shape_D64)
GPU_TOL = 1e-9          # |got - ref| <= GPU_TOL * max(1, |ref|): the bar of test_gpu_parity.py::test_site_fits_*

K_MU_STEP = 64.0        # sitefit.hip: kMuStep
K_TAIL_EPS = 1e-18      # sitefit.hip: kTailEps
K_REL_TAIL_EPS = 1e-13  # sitefit.hip: kRelTailEps
MAX_RATE = 4096.0       # common.h: kSiteFitMaxRate


# ---- the exponential ------------------------------------------------------------------------------------------------------------

def transition_bound(D, mu, terms=30):
    """Relative error bound per entry of ``transition`` in float64 (module docstring)."""
    s = 0 if mu <= 1 else int(np.ceil(np.log2(mu)))
    return 2.0 ** s * (terms * (D + 2) + D) * 2.0 ** -53


def transition(Q, extended=False):
    """exp(Q) for a rate matrix with non-negative off-diagonal entries (the diagonal of ``Q`` is ignored and taken as minus the
    row sum), componentwise accurate; float64 result."""
    ft = np.longdouble if extended else np.float64
    A = np.array(Q, dtype=ft)
    D = A.shape[0]
    idx = np.arange(D)
    A[idx, idx] = 0
    assert A.min() >= 0, "off-diagonal entries must be non-negative"
    d = A.sum(axis=1)
    mu = d.max()
    if not mu > 0:
        return np.eye(D)
    R = A / mu
    R[idx, idx] = (mu - d) / mu
    s = 0
    while float(mu) / 2.0 ** s > 1.0:
        s += 1
    h = mu / ft(2.0 ** s)
    term = np.eye(D, dtype=ft)
    E = term.copy()
    j = 0
    while True:
        j += 1
        term = (term @ R) * (h / j)
        new = E + term
        if np.array_equal(new, E):
            break
        E = new
        assert j < 200
    E = E * np.exp(-h)
    for _ in range(s):
        E = E @ E
    return np.asarray(E, dtype=np.float64)


def build_Q(T, x):
    """sum_k x_k T_k with the diagonal set to minus the row sum."""
    Q = np.tensordot(np.asarray(x, dtype=np.float64), np.asarray(T, dtype=np.float64), axes=(0, 0))
    idx = np.arange(Q.shape[0])
    Q[idx, idx] = 0.0
    Q[idx, idx] = -Q.sum(axis=1)
    return Q


class _Cache:
    def __init__(self, T, fn):
        self.T, self.fn, self.store = np.asarray(T, dtype=np.float64), fn, {}

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = x.tobytes()
        if key not in self.store:
            self.store[key] = self.fn(self.T, x)
        return self.store[key]


def site_fit_logl(D, flat_parents, L, codes, ambig, pi, T, bgroup, bcoef, smult, smix=None, matrix=None, cache=None, scheme=False):
    """[n_sets, S] site log-likelihoods of hyphy_hip_site_fits_evaluate (``smult`` [n_sets, S, G, K]) or, with ``smix``
    [n_sets, S, n_mix], of _mixture (``smult`` [n_sets, S, n_mix, G, K]).  ``matrix(T, x)``: the exponential of sum_k x_k T_k
    (default: ``transition``); it is called once per distinct coefficient vector (``cache``: a dict kept between calls).
    ``scheme=True``: prune with the 2^64 rule in float64 at every node, up to 15 steps (scalefree.model_logl), not scale-free."""
    D, L = int(D), int(L)
    fp = np.asarray(flat_parents, dtype=np.int64)
    B = len(fp) - 1
    codes = np.asarray(codes, dtype=np.int64)
    bgroup = np.asarray(bgroup, dtype=np.int64)
    bcoef = np.asarray(bcoef, dtype=np.float64)
    smult = np.asarray(smult, dtype=np.float64)
    if smix is None:
        smult = smult[:, :, None]
        w = np.ones(smult.shape[:3])
    else:
        w = np.asarray(smix, dtype=np.float64)
    n_sets, S, M = smult.shape[:3]
    store = cache
    cache = _Cache(T, matrix if matrix is not None else (lambda T_, x: transition(build_Q(T_, x))))
    if store is not None:
        cache.store = store
    freq = np.ones(codes.shape[1], dtype=np.int64)
    out = np.zeros((n_sets, S))
    for st in range(n_sets):
        for s in range(S):
            P = np.zeros((B, D, D))
            for m in range(M):
                if w[st, s, m] == 0.0:
                    continue
                x = smult[st, s, m][bgroup] * bcoef            # [B, K]
                for b in range(B):
                    P[b] += w[st, s, m] * cache(x[b])
            if scheme:
                out[st, s] = sf.model_logl(dict(D=D, L=L, flat_parents=fp, leaf_codes=codes[:, s:s + 1], ambig=ambig, root_freqs=pi, P=P))[0]
            else:
                out[st, s] = sf.prune(D, fp, L, codes, ambig, freq, P, pi, patterns=[s])["site_logl"][0]
    return out


def oracle_site_fit_reference(D, flat, codes, ambig, pi, T, bgroup, bcoef, smult, smix=None):
    """The reference's way (FEL.bf:609+): one single-site likelihood function per site — exponentiate every branch's
    own rate matrix (oracle restatement of _Matrix::Exponentiate), then prune that one pattern.  With ``smix``:
    P_b = sum_m w_m Exp(Q_b^(m)) (tree.cpp:3047-3090), ``smult`` [n_sets, S, n_mix, G, K]."""
    from oracle import oracle
    smult = np.asarray(smult, dtype=np.float64)
    if smix is None:
        smult = smult[:, :, None]
        w = np.ones(smult.shape[:3])
    else:
        w = np.asarray(smix, dtype=np.float64)
    n_sets, S, M = smult.shape[:3]
    B = flat.n_branches
    nodes = np.arange(B, dtype=np.int64)
    out = np.zeros((n_sets, S))
    idx = np.arange(D)
    for st in range(n_sets):
        for s in range(S):
            P = None
            for m in range(M):
                x = smult[st, s, m][bgroup] * bcoef  # [B][K]
                Q = np.einsum("bk,kij->bij", x, T)
                Q[:, idx, idx] = -Q.sum(2)
                E = oracle.expm(Q, True)
                P = E if smix is None else (w[st, s, m] * E if P is None else P + w[st, s, m] * E)
            op = oracle.OraclePartition(D, flat.flat_parents, flat.L, codes[:, s:s + 1], ambig, np.ones(1, dtype=np.int64))
            op.set_P(nodes, P)
            out[st, s] = op.site_log_likelihoods(nodes, pi)[0]
    return out


# ---- the kernel's series in numpy -----------------------------------------------------------------------------------------------

def template_reach(T):
    """Largest finite graph distance in the union sparsity pattern of the templates (0 for diagonal templates)."""
    A = (np.asarray(T).sum(axis=0) > 0)
    D = A.shape[0]
    np.fill_diagonal(A, False)
    best = 0
    for i in range(D):
        dist = np.full(D, -1)
        dist[i] = 0
        front = [i]
        while front:
            nxt = []
            for u in front:
                for v in np.flatnonzero(A[u]):
                    if dist[v] < 0:
                        dist[v] = dist[u] + 1
                        nxt.append(v)
            front = nxt
        best = max(best, int(dist.max()))
    return best


def subset_reach(T):
    """Largest ``template_reach`` over the non-empty subsets of the templates: a zero (or negligible) multiplier takes a template
    out of a site's graph, which can lengthen finite distances (MG94: 3 in the union, 5 without the synonymous template)."""
    T = np.asarray(T)
    K = T.shape[0]
    return max(template_reach(T[[k for k in range(K) if mask >> k & 1]]) for mask in range(1, 1 << K))


def model_series(Q_parts, x, v, tail="absolute", mu_max=None, reach=0):
    """exp(sum_k x_k T_k) v as ONE lane of site_fit_kernel computes it, in float64: mu = sum_k x_k dmax_k, n_sub = ceil(mu_max / 64)
    sub-series of term += Q term / mu, wgt *= mu_sub / j, sum += wgt term.  ``v``: [D] or [D, n].  ``mu_max``: the largest rate of
    the lane's tile (default: the lane's own — a tile of its like).
    tail = "absolute": stop when r < 0.5 and wgt_max r / (1 - r) < kTailEps, r = mu_sub_max / (j + 1) — the rule that bounds the
    neglected Poisson mass in absolute terms;  "reach": ``reach`` terms past that point;  "relative": the kernel's present rule —
    the absolute one and the Poisson mass beyond term j - reach below kRelTailEps;  "none": until a term changes no entry of
    the sum (the untruncated series in the kernel's sub-series order)."""
    T = np.asarray(Q_parts, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    K, D = T.shape[0], T.shape[1]
    idx = np.arange(D)
    off = T.copy()
    off[:, idx, idx] = 0.0
    dmax = off.sum(axis=2).max(axis=1)
    mu = float(np.dot(x, dmax))
    mu_max = mu if mu_max is None else float(mu_max)
    term = np.array(v, dtype=np.float64)
    if not mu_max > 0:
        return term
    Q = build_Q(off, x)
    n_sub = int(np.ceil(mu_max / K_MU_STEP))
    mu_sub, mu_sub_max = mu / n_sub, mu_max / n_sub
    inv_mu = 1.0 / mu if mu > 0 else 0.0
    w0 = np.exp(-mu_sub)
    wmax0 = np.exp(-mu_sub_max)
    for _ in range(n_sub):
        wgt, wmax = w0, wmax0
        wlag = wmax0
        total = term * wgt
        extra = reach
        j = 0
        while True:
            j += 1
            wgt *= mu_sub / j
            wmax *= mu_sub_max / j
            term = term + (Q @ term) * inv_mu
            new = total + term * wgt
            same = np.array_equal(new, total)
            total = new
            r = mu_sub_max / (j + 1)
            # (the kernel takes the largest weight of the tile: from the mode on that is the fastest lane's)
            fired = r < 0.5 and max(wgt, wmax) * r / (1.0 - r) < K_TAIL_EPS
            if j > reach:
                wlag *= mu_sub_max / (j - reach)
            if tail == "none":
                if same and fired:
                    break
            elif tail == "relative":
                if fired and j >= reach:
                    rl = mu_sub_max / (j - reach + 1)
                    if rl < 0.5 and wlag * rl / (1.0 - rl) < K_REL_TAIL_EPS:
                        break
            elif fired:
                if tail == "absolute" or extra == 0:
                    break
                extra -= 1
            if j > 4096:
                break
        term = total
    return term


def model_matrix(tail="absolute", reach=0, mu_max=None):
    """A ``matrix`` argument for site_fit_logl: the lane model applied to every unit vector."""
    def fn(T, x):
        return model_series(T, x, np.eye(T.shape[1]), tail=tail, reach=reach, mu_max=mu_max)
    return fn


# ---- cases ----------------------------------------------------------------------------------------------------------------------

POS_FREQS = np.array([[0.3, 0.2, 0.25, 0.25], [0.2, 0.3, 0.3, 0.2], [0.25, 0.25, 0.2, 0.3]])
REV = dict(AC=0.5, AG=1.0, AT=0.4, CG=0.4, CT=1.2, GT=0.4)


def mg94_templates(pad=0):
    """(synonymous, non-synonymous) MG94 x REV templates [2, 61 + pad, 61 + pad] and F3x4 frequencies; ``pad`` extra states that
    nothing reaches (a 64-state alphabet whose last three symbols never occur)."""
    from hyphy_amd import models
    D = 61 + pad
    T = np.zeros((2, D, D))
    for (i, j, name, ns, pf) in models.mg94rev_template(POS_FREQS):
        T[1 if ns else 0, i, j] = REV[name] * pf
    pi = np.zeros(D)
    pi[:61] = models.f3x4_codon_freqs(POS_FREQS)
    if pad:
        pi[:61] *= 0.97
        pi[61:] = 0.03 / pad
    return T, pi


def codon(c):
    from hyphy_amd import models
    return models.CODON_INDEX[c]


def chain_templates(rng, D, K=1):
    """Nearest-neighbour chain (tridiagonal, graph diameter D - 1); link i <-> i + 1 belongs to template i mod K."""
    T = np.zeros((K, D, D))
    for i in range(D - 1):
        T[i % K, i, i + 1] = rng.uniform(0.5, 1.5)
        T[i % K, i + 1, i] = rng.uniform(0.5, 1.5)
    return T


def sparse_templates(rng, D, K, extra=2):
    """A ring plus ``extra`` random links per state, split over K templates: connected, diameter well above 2."""
    T = np.zeros((K, D, D))
    for i in range(D):
        for j in [(i + 1) % D] + list(rng.integers(0, D, size=extra)):
            if j != i:
                k = int(rng.integers(0, K))
                T[k, i, j] = rng.uniform(0.2, 2.0)
                T[k, j, i] = rng.uniform(0.2, 2.0)
    return T


def dense_templates(rng, D, K, pi):
    """The templates of test_gpu_parity.py::_site_fit_case: random, about 64 % dense after symmetrising."""
    T = np.zeros((K, D, D))
    for k in range(K):
        R = rng.uniform(0.1, 2.0, (D, D)) * (rng.random((D, D)) < 0.4)
        R = np.maximum(R, R.T) + np.diag(np.full(D - 1, 0.05), 1) + np.diag(np.full(D - 1, 0.05), -1)
        T[k] = R * pi[None, :]
        np.fill_diagonal(T[k], 0.0)
    return T / max(float((T.sum(0).sum(1) * pi).sum()), 1e-9)


def dyadic_template(D):
    """One template whose entries are multiples of 1/4 and whose largest row sum is exactly 2: the kernel's uniformisation rate
    x * dmax is then exact, so a case can sit exactly at a sub-series boundary."""
    T = np.zeros((1, D, D))
    for i in range(D - 1):
        T[0, i, i + 1] = 1.0 if i % 2 == 0 else 0.75
        T[0, i + 1, i] = 0.5 if i % 2 == 0 else 1.0
    for i in range(1, D - 2, 4):
        T[0, i, i + 2] = 0.25
    assert T[0].sum(axis=1).max() == 2.0
    return T


def near_patterns(rng, L, D, S, spread):
    """Leaf codes [L, S]: per pattern a base state and leaves within ``spread[s]`` states above it (chain templates: that many
    steps apart), in every four patterns one with ambiguity codes."""
    codes = np.zeros((L, S), dtype=np.int64)
    spread = np.broadcast_to(np.asarray(spread), (S,))
    for s in range(S):
        sp = int(spread[s])
        base = int(rng.integers(0, D - sp))
        codes[:, s] = base + rng.integers(0, sp + 1, size=L)
        if sp:
            codes[0, s], codes[1, s] = base, base + sp       # the lowest cherry spans the whole spread
        if s % 4 == 2:
            m = rng.random(L) < 0.2
            codes[m, s] = -rng.integers(1, 3, size=int(m.sum()))
    return codes


def _rates(rng, B, K, G, S, n_sets, c_range, m_range, site_scale=None, n_mix=0, npal=6):
    """Branch coefficients drawn from a palette of ``npal`` rows (few distinct exponentials per site) and one zero-length branch,
    log-uniform multipliers times ``site_scale`` [S]; some multipliers exactly zero."""
    pal = np.exp(rng.uniform(np.log(c_range[0]), np.log(c_range[1]), (npal, K)))
    bcoef = pal[rng.integers(0, npal, size=B)]
    bcoef[rng.integers(0, B)] = 0.0
    bgroup = rng.integers(0, G, size=B)
    shape = (n_sets, S, G, K) if not n_mix else (n_sets, S, n_mix, G, K)
    smult = np.exp(rng.uniform(np.log(m_range[0]), np.log(m_range[1]), shape))
    if site_scale is not None:
        smult = smult * np.asarray(site_scale).reshape((1, S) + (1,) * (smult.ndim - 2))
    if S > 6:
        smult[0, 3] = 0.0                 # a site whose every rate is zero
        smult[-1, 5, ..., 0] = 0.0        # the first template switched off
    return bgroup, bcoef, smult


def _ambig(rng, D):
    a = (rng.random((2, D)) < 0.5).astype(np.float64)
    a[:, 0] = 1.0
    a[0, :] = 1.0        # a full gap
    return a


def _case(name, fp, L, codes, ambig, pi, T, bgroup, bcoef, smult, smix=None, **tags):
    T = np.asarray(T, dtype=np.float64)
    return dict(name=name, D=int(T.shape[1]), L=int(L), flat_parents=np.asarray(fp, dtype=np.int64),
                codes=np.asarray(codes, dtype=np.int64), ambig=ambig, pi=np.asarray(pi, dtype=np.float64), T=T,
                bgroup=np.asarray(bgroup, dtype=np.int64), bcoef=bcoef, smult=smult, smix=smix,
                short=bool(tags.pop("short", False)), ordinary=bool(tags.pop("ordinary", False)),
                impossible=bool(tags.pop("impossible", False)), **tags)


def case_reference(cs, **kw):
    return site_fit_logl(cs["D"], cs["flat_parents"], cs["L"], cs["codes"], cs["ambig"], cs["pi"], cs["T"], cs["bgroup"], cs["bcoef"],
                         cs["smult"], cs["smix"], **kw)


def case_flat(cs):
    fp = cs["flat_parents"]
    return types.SimpleNamespace(flat_parents=fp, L=cs["L"], n_branches=len(fp) - 1)


def case_rates(cs):
    """The kernel's uniformisation rates [n_sets, S, (n_mix,) B] = sum_k x_k dmax_k."""
    off = cs["T"].copy()
    idx = np.arange(cs["D"])
    off[:, idx, idx] = 0.0
    dmax = off.sum(axis=2).max(axis=1)
    sm = cs["smult"]
    x = sm[..., cs["bgroup"], :] * cs["bcoef"]
    return x @ dmax


def _codon_forced(codes, L, pad_ok=True):
    """Patterns that force multi-step entries, written over every eighth pattern and the three after it: sibling leaves 3 and 2
    nucleotides apart, one odd leaf against a conserved column (3 and 2 apart)."""
    A, C3, C2, G, G2 = codon("AAA"), codon("CCC"), codon("ACC"), codon("GGG"), codon("GCC")
    S = codes.shape[1]
    for s in range(0, S - 3, 8):
        codes[:, s] = A
        codes[1, s] = C3
        codes[:, s + 1] = A
        codes[1, s + 1] = C2
        codes[:, s + 2] = A
        codes[L - 1, s + 2] = C3
        codes[:, s + 3] = G
        codes[L // 2, s + 3] = G2
    return codes


SLOW = 1e-9            # the multiplier of the slow site of the tile-neighbour cases
NEIGHBOURS = ("neigh_like", "neigh_fast", "neigh_alone_S1", "neigh_alone_S17")


def cases():
    return list(_enumerate())


def oracle_deep(name):
    """Module docstring: the cases on which the oracle route is held to ORACLE_MAX_REL, not to ORACLE_MAX_REL_SHALLOW."""
    return "chain" in name or name == "mg94_alpha0"


def cases_by_name():
    return {c["name"]: c for c in cases()}


def _enumerate():
    """The fixed list of named, seeded cases.  Keys: name, D, L, flat_parents, codes [L, S], ambig, pi, T [K, D, D], bgroup [B],
    bcoef [B, K], smult [n_sets, S, G, K] (mixtures: [n_sets, S, n_mix, G, K] and smix [n_sets, S, n_mix]); tags ``short`` (the
    absolute stopping rule loses it), ``ordinary`` (it does not), ``impossible`` (may hold more than 10 % patterns of zero
    likelihood), ``probe`` (tile-neighbour cases: the index of the slow site).  Enumerated here, filtered nowhere else."""
    seed = 0

    def rng_for():
        nonlocal seed
        seed += 1
        return np.random.default_rng(7100 + seed)

    mgT, mgpi = mg94_templates()
    mgT64, mgpi64 = mg94_templates(pad=3)

    # -- structured templates, coefficients spanning 1e-13 .. 1e-2 over the sites of a tile
    for (name, T, pi) in (("mg94_span", mgT, mgpi), ("mg94_span_D64", mgT64, mgpi64)):
        rng = rng_for()
        fp, L = sf.balanced_tree(2, 3)
        S = 32
        codes = _codon_forced(sf._patterns(rng, L, 61, S, 2), L)
        bg, bc, sm = _rates(rng, len(fp) - 1, 2, 2, S, 2, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-13, -2, S))
        yield _case(name, fp, L, codes, _ambig(rng, T.shape[1]), pi, T, bg, bc, sm, short=True)

    rng = rng_for()
    fp, L = sf.ladder_tree(10)
    S = 32
    T = chain_templates(rng, 20)
    bg, bc, sm = _rates(rng, len(fp) - 1, 1, 1, S, 2, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-13, -2, S))
    yield _case("chain20_span", fp, L, near_patterns(rng, L, 20, S, 3), _ambig(rng, 20), np.full(20, 0.05), T, bg, bc, sm, short=True)

    rng = rng_for()
    fp, L = sf.balanced_tree(2, 2)
    S = 20
    T = chain_templates(rng, 20)
    bg, bc, sm = _rates(rng, len(fp) - 1, 1, 2, S, 1, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-4, -2, S))
    yield _case("chain20_far", fp, L, near_patterns(rng, L, 20, S, np.arange(S) % 20), _ambig(rng, 20), np.full(20, 0.05), T, bg, bc, sm,
                short=True)

    rng = rng_for()
    fp, L = sf.ladder_tree(7)
    S = 24
    T = chain_templates(rng, 20, K=2)
    bg, bc, sm = _rates(rng, len(fp) - 1, 2, 2, S, 2, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-9, -3, S))
    yield _case("chain20_K2", fp, L, near_patterns(rng, L, 20, S, 4), _ambig(rng, 20), np.full(20, 0.05), T, bg, bc, sm, short=True)

    # -- a dense random template at ordinary rates (the shape of the present tests)
    rng = rng_for()
    fp, L = sf.ladder_tree(9)
    S = 24
    pi = rng.dirichlet(np.full(61, 5.0))
    T = dense_templates(rng, 61, 2, pi)
    bg, bc, sm = _rates(rng, len(fp) - 1, 2, 2, S, 2, (0.01, 0.5), (0.01, 5.0))
    yield _case("dense_ordinary", fp, L, sf._patterns(rng, L, 61, S, 2), _ambig(rng, 61), pi, T, bg, bc, sm, ordinary=True)

    # -- a block template with one isolated state: impossible patterns, and patterns that carry the isolated state everywhere
    rng = rng_for()
    D = 17
    fp, L = sf.balanced_tree(2, 3)
    S = 32
    T = np.zeros((2, D, D))
    T[:, :16, :16] = sparse_templates(rng, 16, 2)
    codes = near_patterns(rng, L, 16, S, 2)
    for s in range(1, S, 4):           # impossible: the isolated state at one leaf, another state at its sibling
        codes[:, s] = np.arange(L) % 16
        codes[s % L, s] = 16
    for s in range(2, S, 8):           # possible: the isolated state everywhere, one leaf a full gap
        codes[:, s] = 16
        codes[3, s] = -1
    pi = rng.dirichlet(np.full(D, 5.0))
    bg, bc, sm = _rates(rng, len(fp) - 1, 2, 2, S, 2, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-8, 0, S))
    yield _case("block_isolated_impossible", fp, L, codes, _ambig(rng, D), pi, T, bg, bc, sm, impossible=True)

    # -- rates at the sub-series boundaries: n_sub = 1, 1, 2, 10, 64
    for rate in (60.0, 64.0, 65.0, 640.0, 4095.0):
        rng = rng_for()
        D = 16
        fp, L = sf.balanced_tree(2, 2)
        S = 16
        T = dyadic_template(D)
        B = len(fp) - 1
        bcoef = np.full((B, 1), rate / 2.0)
        bcoef[1::2] = rate / 64.0
        bcoef[2] = 0.0
        smult = (1.0 / (1.0 + np.arange(S) % 8)).reshape(1, S, 1, 1).copy()     # sites 0 and 8 at the full rate
        smult[0, 7] = 0.0
        pi = rng.dirichlet(np.full(D, 5.0))
        yield _case(f"rate_{int(rate)}", fp, L, near_patterns(rng, L, D, S, 5), _ambig(rng, D), pi, T, np.zeros(B, dtype=np.int64), bcoef,
                    smult, ordinary=rate < 100, n_sub=int(np.ceil(rate / K_MU_STEP)))

    # -- tile neighbours: the same slow site in a tile of its like, beside a site near the rate limit, alone in a padded tile
    for name in NEIGHBOURS:
        rng = np.random.default_rng(7177)              # the same draws for all four
        fp, L = sf.ladder_tree(6)
        B = len(fp) - 1
        S = {"neigh_like": 16, "neigh_fast": 16, "neigh_alone_S1": 1, "neigh_alone_S17": 17}[name]
        probe = {"neigh_like": 4, "neigh_fast": 4, "neigh_alone_S1": 0, "neigh_alone_S17": 16}[name]
        bgroup = rng.integers(0, 2, size=B)
        bcoef = rng.uniform(0.5, 2.0, (B, 2))
        col = np.full(L, codon("AAA"))
        col[1] = codon("CCC")                           # the cherry (0, 1) three nucleotides apart
        col[4] = codon("ACC")
        codes = np.repeat(col[:, None], S, axis=1)
        smult = np.full((1, S, 2, 2), SLOW)
        smult[..., 1] *= 0.5
        if name == "neigh_fast":
            dmax = mgT.sum(axis=2).max(axis=1)
            smult[0, 9] = 4000.0 / float((bcoef.max(axis=0) * dmax).sum())
        if name == "neigh_alone_S17":                   # the first tile: ordinary sites
            codes[:, :16] = sf._patterns(rng, L, 61, 16, 2)
            smult[0, :16] = rng.uniform(0.05, 2.0, (16, 2, 2))
        yield _case(name, fp, L, codes, _ambig(rng, 61), mgpi, mgT, bgroup, bcoef, smult, probe=probe, short=True)

    # -- row blocks and shape: every NW and both sides of each boundary; K = 1 .. 4, G = 1 and 16, n_sets > 1
    for n, D in enumerate((5, 16, 17, 20, 32, 33, 48, 49, 61, 64)):
        rng = rng_for()
        K, G, n_sets = 1 + n % 4, (1, 16)[n % 2], 1 + n % 3
        fp, L = sf.ladder_tree(4, hang=(2, 2)) if n % 2 else sf.balanced_tree(3, 2)
        S = 20
        T = sparse_templates(rng, D, K)
        pi = rng.dirichlet(np.full(D, 5.0))
        bg, bc, sm = _rates(rng, len(fp) - 1, K, G, S, n_sets, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-10, 0, S))
        yield _case(f"shape_D{D}", fp, L, sf._patterns(rng, L, D, S, 3), _ambig(rng, D), pi, T, bg, bc, sm)

    # -- a template switched off (multiplier exactly 0, or 1e-30): the site's graph is that of the remaining templates, where
    #    finite distances are longer than in the union (MG94 without the synonymous template: ACC -> CCT takes 5 steps, not 2)
    rng = rng_for()
    fp, L = sf.ladder_tree(6)
    B = len(fp) - 1
    S = 24
    pairs = [("ACC", "CCT"), ("AAA", "CCC"), ("ACC", "ACC"), ("TTT", "CTG")]
    codes = np.zeros((L, S), dtype=np.int64)
    for s_ in range(S):
        a_, b_ = pairs[s_ % 4]
        codes[:, s_] = codon(a_)
        codes[1 + (s_ // 4) % 3, s_] = codon(b_)
    bgroup = rng.integers(0, 2, size=B)
    bcoef = rng.uniform(0.5, 2.0, (B, 2))
    smult = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (2, S, 2, 2))) * np.logspace(-12, -6, S).reshape(1, S, 1, 1)
    smult[0, :, :, 0] = 0.0                          # alpha = 0 in every branch group
    smult[1, :, :, 0] = 1e-30                        # ... and negligible
    smult[1, S // 2:, 1, 0] = smult[1, S // 2:, 1, 1]   # (the second group keeps its synonymous rate on half the sites)
    yield _case("mg94_alpha0", fp, L, codes, _ambig(rng, 61), mgpi, mgT, bgroup, bcoef, smult, short=True)

    rng = rng_for()
    fp, L = sf.balanced_tree(2, 3)
    B = len(fp) - 1
    S = 24
    pi = rng.dirichlet(np.full(20, 5.0))
    T = np.concatenate([dense_templates(rng, 20, 1, pi), chain_templates(rng, 20)])
    bgroup = rng.integers(0, 2, size=B)
    bcoef = rng.uniform(0.5, 2.0, (B, 2))
    smult = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (2, S, 2, 2))) * np.logspace(-10, -4, S).reshape(1, S, 1, 1)
    smult[0, :, :, 0] = 0.0                          # the dense template off: the chain alone, up to 19 steps
    smult[1, :, :, 0] = 1e-30
    yield _case("dense_off_chain20", fp, L, near_patterns(rng, L, 20, S, 1 + np.arange(S) % 6), _ambig(rng, 20), pi, T, bgroup, bcoef,
                smult, short=True)

    # -- mixtures: n_mix = 2, 3, 8; a weight of exactly 0; a component whose rates are all zero
    for (name, n_mix, T, pi, D, scale) in (("mix2_mg94", 2, mgT, mgpi, 61, (-11, -1)), ("mix3_chain20", 3, None, None, 20, (-9, -2)),
                                           ("mix8_D33", 8, None, None, 33, (-8, 0))):
        rng = rng_for()
        if T is None:
            T = chain_templates(rng, D, K=2) if D == 20 else sparse_templates(rng, D, 2)
            pi = rng.dirichlet(np.full(D, 5.0))
        fp, L = sf.balanced_tree(2, 3)
        S = 20
        codes = _codon_forced(sf._patterns(rng, L, 61, S, 2), L) if D == 61 else near_patterns(rng, L, D, S, 3)
        bg, bc, sm = _rates(rng, len(fp) - 1, 2, 2, S, 2, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(scale[0], scale[1], S),
                            n_mix=n_mix)
        sw = rng.dirichlet(np.full(n_mix, 2.0), size=(2, S))
        sw[0, 1::4, 0] = 0.0                             # a weight of exactly zero (the others keep their draws: sum < 1 is allowed)
        sw[1, 2] = np.eye(n_mix)[n_mix - 1]              # degenerate
        sm[:, 0::4, n_mix - 1] = 0.0                     # a component whose rates are all zero
        yield _case(name, fp, L, codes, _ambig(rng, D), pi, T, bg, bc, sm, smix=sw, short=True)

    # -- the kernel's own 2^64 steps and spills, on the structured templates, ambiguity codes in the tile
    deep = (("ladder120_mg94", sf.ladder_tree(120), 2), ("ladder300_mg94", sf.ladder_tree(300), 2),
            ("balanced128_mg94", sf.balanced_tree(2, 7), 2), ("conflict_k4_d2_mg94", sf.balanced_tree(4, 2), 4),
            ("conflict_k4_d3_mg94", sf.balanced_tree(4, 3), 4), ("conflict_k8_d2_mg94", sf.balanced_tree(8, 2), 8))
    for (name, (fp, L), k) in deep:
        rng = rng_for()
        S = 20
        codes = sf._patterns(rng, L, 61, S, k)
        if name.startswith("conflict"):
            codes = _codon_forced(codes, L)
        scale = np.logspace(-9, -5, S) if name.startswith("conflict") else np.logspace(-6, -1, S)
        bg, bc, sm = _rates(rng, len(fp) - 1, 2, 2, S, 1, (0.3, 3.0), (0.5, 2.0), site_scale=scale)
        yield _case(name, fp, L, codes, _ambig(rng, 61), mgpi, mgT, bg, bc, sm, short=name.startswith("conflict"))

    rng = rng_for()
    fp, L = sf.ladder_tree(40, hang=(4, 2))
    S = 20
    T = chain_templates(rng, 20)
    bg, bc, sm = _rates(rng, len(fp) - 1, 1, 2, S, 2, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-9, -3, S))
    yield _case("ladder40_on_k4d2_chain20", fp, L, near_patterns(rng, L, 20, S, 3), _ambig(rng, 20), np.full(20, 0.05), T, bg, bc, sm,
                short=True)

    # -- a 4-ary conflict tree of depth 3 on the chain template: several steps of 2^64 at one node, away from the codon cases
    rng = rng_for()
    fp, L = sf.balanced_tree(4, 3)
    S = 20
    T = chain_templates(rng, 20)
    bg, bc, sm = _rates(rng, len(fp) - 1, 1, 2, S, 1, (0.3, 3.0), (0.5, 2.0), site_scale=np.logspace(-9, -6, S))
    codes = near_patterns(rng, L, 20, S, 3)
    codes[:, 0::2] = (codes[:1, 0::2] - codes[:1, 0::2].min(axis=0)) + (np.arange(L)[:, None] % 4)     # siblings 0 .. 3 steps apart
    yield _case("conflict_k4_d3_chain20", fp, L, codes, _ambig(rng, 20), np.full(20, 0.05), T, bg, bc, sm, short=True)
