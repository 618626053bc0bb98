"""The recursion behind hyphy_hip_branch_derivatives restated in numpy, its generators, and the allowances.

``outside`` is tests/test_branch_trials_cpu.py's pre-order pass once more — U_root = pi, V_c = U_p * prod_{s != c} E_s, U_c = P_c^T V_c,
every vector divided by its largest element with the logarithm of the divisor beside it, no 2^64 scheme — run in ``np.longdouble``
from the leaves up (the inside pass too), and keeping per branch V_c, E_c = P_c in_c and the logarithm of what was divided out of both.
``values`` forms per pattern
    l0 = V . E      l1 = V . (G E)      l2 = V . (G (G E))      (mixed over the classes by weight, aligned on the largest magnitude)
    r1 = L1 / L0    r2 = L2 / L0 - r1^2
and the magnitudes the allowances are written in,  A1 = (|V|^T |G| |E|) / l0,  A2 = (|V|^T |G| |G| |E|) / l0.

Allowances (per pattern; the totals get their f-weighted sums):  |dr1| <= GPU_RTOL A1,  |dr2| <= GPU_RTOL (A2 + 2 |r1| A1).
scalefree.GPU_RTOL (3.1e-13, about 1400 eps) is the project's bar for per-pattern values built from the same vectors; worst-case
rounding of three nested length-D dot products is about 3 D eps <= 200 eps in units of A1 and A2 at D = 64, and the float64 form of
this recursion lies within a few eps of the longdouble one in those units (tests/test_branch_derivatives_cpu.py prints it)."""
import numpy as np

from tests import branchcache_cases as bc
from tests import scalefree as sf

RTOL = sf.GPU_RTOL
KINDS = ("sparse", "row_scaled", "quarter_identity", "zero")
MISTAKES = ("g_transposed", "u_for_v", "no_r1_squared", "unaligned")


def d4_case():
    return bc._make("bal2x4_D4", "bal2x4", 4, 7004)


def ladder_class_case():
    """branchcache_cases.class_cases' recipe (three rate classes, off-diagonals 1e-2, 1e-12, 1e-30) on the 40-taxon ladder at 20
    states.  Just below the root of a ladder V_c is pi times ONE leaf's edge product — no exponent in any class — and in_c carries the
    whole tree's: the classes are aligned right only if in_c's exponent is counted, which the balanced tree of ``class_cases`` cannot
    show (there the exponent of V_c alone already tells the classes apart by the same 2^64 steps)."""
    D, n = 20, 40
    rng = np.random.default_rng(7350)
    fp, L = sf.ladder_tree(n)
    codes = bc._mixed_patterns(rng, fp, L, D, 20, 2, lambda l: l % 5 == 0, False)
    B = len(fp) - 1
    P = np.stack([sf.near_identity(rng, B, D, e, spread=D * e < 0.3) for e in (1e-2, 1e-12, 1e-30)])
    pi = rng.random(D) + 0.1
    cs = sf._case(f"ladder{n}_classes_D{D}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum(), weights=np.array([0.5, 0.3, 0.2]))
    cs["seed"] = 7350
    cs["eps"] = 1e-12
    cs["branches"] = bc.spread_ladder_branches(n)
    return cs


def generators(cs, node, cls=0):
    """[(kind, G)] for branch ``node`` (class ``cls``), in KINDS' order; seeded by the case, the branch and the class."""
    D = int(cs["D"])
    rng = np.random.default_rng([int(cs["seed"]), int(node), 977 + int(cls)])
    keep = rng.random((D, D)) < 0.3
    M = (rng.random((D, D)) + 0.05) * keep
    M[np.arange(D), np.arange(D)] = 0.0
    if not M.any():
        M[0, 1] = 1.0
    M *= 0.5 / M.sum(axis=1).max()                       # largest row sum 0.5
    G = M.copy()
    G[np.arange(D), np.arange(D)] = -M.sum(axis=1)
    scale = 10.0 ** (-13.0 * rng.permutation(D) / max(D - 1, 1))   # rows scaled over 1e-13 .. 1
    return [("sparse", G), ("row_scaled", G * scale[:, None]), ("quarter_identity", -0.25 * np.eye(D)), ("zero", np.zeros((D, D)))]


def _norm(v, lg):
    m = v.max(axis=1)
    ok = m > 0
    with np.errstate(divide="ignore"):
        return np.where(ok[:, None], v / np.where(ok, m, 1)[:, None], 0), lg + np.log(m)


def _leaf_vectors(cs, c, ft):
    D = int(cs["D"])
    k = np.asarray(cs["leaf_codes"], dtype=np.int64)[c]
    amb = np.asarray(cs["ambig"], dtype=np.float64) if cs["ambig"] is not None and len(cs["ambig"]) else np.zeros((1, D))
    return np.where((k < 0)[:, None], amb[np.maximum(-k - 1, 0)], np.eye(D)[np.maximum(k, 0)]).astype(ft)


def outside(cs, P=None, ft=np.longdouble, mistake=None):
    """Per branch c of one class: (V_c [S, D], E_c = P_c in_c [S, D], log of what was divided out of V_c and in_c together [S]).
    ``mistake`` "u_for_v": U_c = P_c^T V_c in place of V_c."""
    D, L = int(cs["D"]), int(cs["L"])
    fp = np.asarray(cs["flat_parents"], dtype=np.int64)
    P = np.asarray(cs["P"] if P is None else P).astype(ft)
    pi = np.asarray(cs["root_freqs"]).astype(ft)
    S = np.asarray(cs["leaf_codes"]).shape[1]
    ch = sf.children_of(fp, L)
    I = len(ch)
    cond, lg, E = [None] * I, [None] * I, {}
    for n in range(I):                                   # inside pass
        v, acc = np.ones((S, D), dtype=ft), np.zeros(S, dtype=ft)
        for c in ch[n]:
            inv = cond[c - L] if c >= L else _leaf_vectors(cs, c, ft)
            E[c] = inv @ P[c].T
            v, acc = _norm(v * E[c], acc + (lg[c - L] if c >= L else 0))
        cond[n], lg[n] = v, acc
    U, lU = [None] * I, [None] * I
    U[I - 1], lU[I - 1] = np.broadcast_to(pi, (S, D)).copy(), np.zeros(S, dtype=ft)
    out = {}
    for n in range(I - 1, -1, -1):                       # children are numbered before their parents: this is a pre-order
        for c in ch[n]:
            V, lV = U[n].copy(), lU[n].copy()
            for s in ch[n]:
                if s != c:
                    V, lV = _norm(V * E[s], lV + (lg[s - L] if s >= L else 0))
            Uc, lUc = _norm(V @ P[c], lV)
            if c >= L:
                U[c - L], lU[c - L] = Uc, lUc
            lin = lg[c - L] if c >= L else np.zeros(S, dtype=ft)
            out[c] = (Uc, E[c], lUc + lin) if mistake == "u_for_v" else (V, E[c], lV + lin)
    return out


def values(cs, outs, node, Gs, weights=None, mistake=None):
    """``outs``: one ``outside`` result per class; ``Gs``: one generator per class.  Returns a dict of per-pattern arrays r1, r2,
    A1, A2, allow1, allow2, skipped (bool: positive frequency and L0 == 0), and the totals d1, d2, allow_d1, allow_d2, n_skipped."""
    ft = outs[0][node][0].dtype
    f = np.asarray(cs["pattern_freq"], dtype=np.float64)
    w = np.ones(1) if weights is None else np.asarray(weights, dtype=np.float64)
    rows = []
    for o, G in zip(outs, Gs):
        V, E, lm = o[node]
        G = np.asarray(G).astype(ft)
        if mistake == "g_transposed":
            G = G.T
        GE = E @ G.T
        aG = np.abs(G)
        aGE = np.abs(E) @ aG.T
        rows.append(((V * E).sum(axis=1), (V * GE).sum(axis=1), (V * (GE @ G.T)).sum(axis=1),
                     (np.abs(V) * aGE).sum(axis=1), (np.abs(V) * (aGE @ aG.T)).sum(axis=1), lm))
    lm = np.stack([r[5] for r in rows])
    live = np.stack([(w[c] != 0) & ((rows[c][0] != 0) | (rows[c][3] != 0) | (rows[c][4] != 0)) for c in range(len(rows))])
    with np.errstate(invalid="ignore"):
        top = np.where(live, lm, -np.inf).max(axis=0)
    top = np.where(np.isfinite(top), top, 0)
    L = []
    for j in range(5):
        tot = np.zeros(len(f), dtype=ft)
        for c in range(len(rows)):
            with np.errstate(invalid="ignore", over="ignore"):
                sc = 1.0 if mistake == "unaligned" else np.where(live[c], np.exp(np.where(live[c], lm[c] - top, 0)), 0)
            tot = tot + w[c] * sc * rows[c][j]
        L.append(tot)
    L0, L1, L2, B1, B2 = L
    ok = L0 != 0
    den = np.where(ok, L0, 1)
    r1 = np.where(ok, L1 / den, np.nan)
    r2 = np.where(ok, L2 / den - (0 if mistake == "no_r1_squared" else r1 * r1), np.nan)
    A1, A2 = np.where(ok, B1 / den, np.nan), np.where(ok, B2 / den, np.nan)
    allow1, allow2 = RTOL * A1, RTOL * (A2 + 2 * np.abs(r1) * A1)
    use = ok & (f > 0)
    fs = f.astype(ft)
    tot = lambda x: np.sum(np.where(use, fs * np.where(use, x, 0), 0))
    return dict(r1=r1, r2=r2, A1=A1, A2=A2, allow1=allow1, allow2=allow2, skipped=(~ok) & (f > 0), d1=tot(r1), d2=tot(r2),
                allow_d1=tot(allow1), allow_d2=tot(allow2), n_skipped=int(np.sum((~ok) & (f > 0))))


_outs = {}


def outs_of(cs):
    """The longdouble ``outside`` of every class of the case, computed once per case name."""
    if cs["name"] not in _outs:
        P = np.asarray(cs["P"])
        _outs[cs["name"]] = [outside(cs)] if P.ndim == 3 else [outside(cs, P[c]) for c in range(P.shape[0])]
    return _outs[cs["name"]]


def miss(got_r1, got_r2, got_d1, got_d2, ref):
    """Largest deviation / allowance over the per-pattern values and the totals (0 / 0 counts as 0; inf where NaN sits in the wrong
    place or an exact value is missed)."""
    worst = 0.0
    for got, want, allow in ((got_r1, ref["r1"], ref["allow1"]), (got_r2, ref["r2"], ref["allow2"])):
        if got is None:
            continue
        got = np.asarray(got)
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            return np.inf
        fin = ~np.isnan(want)
        dev, al = np.abs(got[fin] - want[fin]).astype(np.float64), allow[fin].astype(np.float64)
        if np.any((al == 0) & (dev != 0)):
            return np.inf
        if fin.any():
            worst = max(worst, float(np.max(np.where(dev == 0, 0.0, dev / np.where(al > 0, al, 1.0)))))
    for got, want, allow in ((got_d1, ref["d1"], ref["allow_d1"]), (got_d2, ref["d2"], ref["allow_d2"])):
        dev, al = float(abs(got - want)), float(allow)
        if dev != 0:
            worst = max(worst, dev / al if al > 0 else np.inf)
    return worst


def site_logl(cs, P, ft=np.longdouble):
    """Per-pattern log-likelihood by the inside pass of ``outside`` alone, in ``ft`` throughout (-inf where it is zero)."""
    D, L = int(cs["D"]), int(cs["L"])
    P = np.asarray(P).astype(ft)
    S = np.asarray(cs["leaf_codes"]).shape[1]
    ch = sf.children_of(cs["flat_parents"], L)
    cond, lg = [None] * len(ch), [None] * len(ch)
    for n in range(len(ch)):
        v, acc = np.ones((S, D), dtype=ft), np.zeros(S, dtype=ft)
        for c in ch[n]:
            inv = cond[c - L] if c >= L else _leaf_vectors(cs, c, ft)
            v, acc = _norm(v * (inv @ P[c].T), acc + (lg[c - L] if c >= L else 0))
        cond[n], lg[n] = v, acc
    root = cond[-1] @ np.asarray(cs["root_freqs"]).astype(ft)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(root > 0, np.log(root) + lg[-1], -np.inf)


FIT_TREE_6 = (np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, -1], dtype=np.int64), 6)                 # three cherries below the root
FIT_TREE_8 = (np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 5, -1], dtype=np.int64), 8)     # ((c0, c1), c2, c3)


# ---- a small model to fit branch lengths on ---------------------------------------------------------------------------------------

def fit_case(name, tree, D, n_sites, seed, max_patterns=None, t_range=(0.05, 0.4)):
    """Per-branch unit rate matrices (random, not reversible, mean rate 1), a random pi, and ``n_sites`` sites drawn from the model at
    lengths uniform in 0.05 .. 0.4, compressed to patterns with their counts.  ``P`` is the model at t = 0.1 everywhere."""
    from tests import expm_ref
    rng = np.random.default_rng(seed)
    fp, L = tree
    fp = np.asarray(fp, dtype=np.int64)
    B = len(fp) - 1
    Q = rng.uniform(0.2, 1.0, size=(B, D, D))
    Q[:, np.arange(D), np.arange(D)] = 0.0
    Q /= Q.sum(axis=2).mean(axis=1)[:, None, None]
    Q[:, np.arange(D), np.arange(D)] = -Q.sum(axis=2)
    pi = rng.random(D) + 0.3
    pi /= pi.sum()
    t_true = rng.uniform(t_range[0], t_range[1], size=B)
    P = np.stack([expm_ref.reference(t_true[b] * Q[b]) for b in range(B)])
    states = np.zeros((len(fp), n_sites), dtype=np.int64)
    states[len(fp) - 1] = rng.choice(D, size=n_sites, p=pi)
    order = sorted(range(B), key=lambda c: -(L + int(fp[c])))   # a node after its parent
    for c in order:
        rows = P[c][states[L + int(fp[c])]]
        rows = rows / rows.sum(axis=1, keepdims=True)
        states[c] = (rng.random(n_sites)[:, None] > np.cumsum(rows, axis=1)).sum(axis=1).clip(0, D - 1)
    pats, counts = np.unique(states[:L], axis=1, return_counts=True)
    if max_patterns is not None:                          # the most frequent ones, in np.unique's order
        keep = np.sort(np.argsort(-counts, kind="stable")[:max_patterns])
        pats, counts = pats[:, keep], counts[keep]
    cs = dict(name=name, D=D, L=L, flat_parents=fp, leaf_codes=pats.astype(np.int64), ambig=np.zeros((1, D)),
              pattern_freq=counts.astype(np.float64), root_freqs=pi, unit_Q=Q, t_true=t_true, seed=seed)
    cs["P"] = fit_model(cs, np.full(B, 0.1))
    return cs


def fit_model(cs, t, rates=None):
    """Transition matrices [B, D, D] at branch lengths ``t`` ([C, B, D, D] with class ``rates``)."""
    from tests import expm_ref
    Q = cs["unit_Q"]
    one = lambda r: np.stack([expm_ref.reference(r * float(t[b]) * Q[b]) for b in range(len(Q))])
    return one(1.0) if rates is None else np.stack([one(float(r)) for r in rates])


def fit_derivatives(cs, t, rates=None, weights=None):
    """(d1, d2) of every branch at lengths ``t`` with G = rates[c] t_b unit_Q[b], by the float64 recursion."""
    P = fit_model(cs, t, rates)
    outs = [outside(cs, P, ft=np.float64)] if rates is None else [outside(cs, P[c], ft=np.float64) for c in range(len(rates))]
    rs = [1.0] if rates is None else list(rates)
    v = [values(cs, outs, b, [r * t[b] * cs["unit_Q"][b] for r in rs], weights) for b in range(len(t))]
    return np.array([x["d1"] for x in v], dtype=np.float64), np.array([x["d2"] for x in v], dtype=np.float64)


def fit_logl(cs, t, rates=None, weights=None):
    return sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], fit_model(cs, t, rates),
                    cs["root_freqs"], weights=weights)["logl"]
