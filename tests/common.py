"""Shared helpers for the parity tests: load a golden fixture and rebuild the numeric rate
matrices the reference evaluated (same templates as oracle/hbl.py wrote into the HBL)."""
import os

import numpy as np

from hyphy_amd import models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REV_KEYS = ("AC", "AT", "CG", "CT", "GT")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def fixture_Q(fx, cat_value=1.0):
    """[B, D, D] rate matrices (already multiplied by branch length) for a fixture."""
    rev = dict(zip(REV_KEYS, (float(x) for x in fx["rev"])))
    t = np.asarray(fx["t"], dtype=np.float64) * cat_value
    if str(fx["kind"]) == "codon":
        return models.mg94rev_Q_batch(t, float(fx["omega"]), rev, fx["pos_freqs"])
    return np.stack([models.nuc_rev_Q(float(tt), rev, fx["root_freqs"]) for tt in t])


def all_nodes(fx):
    return np.arange(len(fx["flat_parents"]) - 1, dtype=np.int64)


def busted_components(fx):
    """Rate matrices [B, 3, 61, 61] and weights [B, 3] of the unconstrained BUSTED model stored in a `ref_busted_*` fixture
    (test branches and background branches carry their own omega distribution; BS_REL.bf: P_b = sum_k w_k Exp(Q_b(omega_k)))."""
    from hyphy_amd import models
    rev = dict(zip(REV_KEYS, (float(x) for x in fx["rev"])))
    t = np.asarray(fx["t"], dtype=np.float64)
    B = len(t)
    Qc = np.zeros((B, 3, 61, 61))
    W = np.zeros((B, 3))
    by_set = {True: (fx["omega_test"], fx["weights_test"]), False: (fx["omega_background"], fx["weights_background"])}
    for b in range(B):
        om, w = by_set[bool(fx["tested"][b])]
        W[b] = w
        for k in range(3):
            Qc[b, k] = models.mg94rev_Q(t[b], float(om[k]), rev, fx["pos_freqs"])
    return Qc, W


def fubar_site_fit_args(fx, grid_points=None, sites=None):
    """Arguments of hyphy_hip_site_fits_evaluate for a `ref_fubar_*` fixture: one branch group, per-branch (synonymous, non-synonymous)
    factors, and one parameter set per grid point — every site of a set carries that point's (alpha, beta).
    Returns (templates [2, 61, 61], branch_group [B], branch_coeffs [B, 2], site_mult [n, S, 1, 2], leaf_codes [L, S], expected [n, S])."""
    from hyphy_amd import models
    rev = dict(zip(REV_KEYS, (float(x) for x in fx["rev"])), AG=1.0)
    T = np.zeros((2, 61, 61))
    for (i, j, name, ns, f) in models.mg94rev_template(fx["pos_freqs"]):
        T[1 if ns else 0, i, j] = rev[name] * f
    gp = np.arange(fx["grid"].shape[0]) if grid_points is None else np.asarray(grid_points)
    st = np.arange(fx["leaf_codes"].shape[1]) if sites is None else np.asarray(sites)
    B = len(fx["syn_factor"])
    coeffs = np.ascontiguousarray(np.stack([fx["syn_factor"], fx["nonsyn_factor"]], axis=1))
    mult = np.ascontiguousarray(np.broadcast_to(fx["grid"][gp][:, None, None, :], (len(gp), len(st), 1, 2)))
    return T, np.zeros(B, dtype=np.int64), coeffs, mult, np.ascontiguousarray(fx["leaf_codes"][:, st]), fx["site_logl"][np.ix_(gp, st)]


# state counts the class-compressed form is held to off its two golden paths (61, 4): NW = ceil(D / 16) = 1 .. 4 row blocks, each
# with and without padding rows (4 states is the separate nucleotide path)
REPEAT_STATE_COUNTS = (2, 5, 16, 17, 20, 32, 33, 48, 49, 61, 64)


def random_rates(rng, n, D):
    """[n, D, D] random rate matrices (rows sum to zero), one per branch, scaled between 0.01 and 0.4."""
    Q = rng.random((n, D, D)) * rng.uniform(0.01, 0.4, size=(n, 1, 1))
    Q[:, np.arange(D), np.arange(D)] = 0.0
    Q[:, np.arange(D), np.arange(D)] = -Q.sum(axis=2)
    return Q


def compressible_case(D, seed, taxa=None, S=None):
    """A synthetic partition whose subtrees repeat at any compression threshold, seeded: a random multifurcating tree (2-4 children
    per node), leaf codes with a few states per column drawn from a small palette that holds the highest state (the last row block),
    every pattern twice with different weights, ambiguity codes (3 % on the variable leaves, fewer on the conserved ones), random rate matrices per branch and random root frequencies.
    Keys as the golden fixtures' (what hip.HipPartition and oracle.OraclePartition take) plus "Q" [B, D, D]."""
    from hyphy_amd import tree
    rng = np.random.default_rng(seed)
    taxa = int(taxa or rng.integers(12, 29))
    S = int(S or 2 * rng.integers(100, 160))
    pool = [tree.Node(name=f"T{k + 1}") for k in range(taxa)]
    joins = 0
    while len(pool) > 4:
        m = int(min(rng.choice([2, 2, 2, 3, 4]), len(pool) - 1))
        idx = sorted(rng.choice(len(pool), size=m, replace=False), reverse=True)
        kids = [pool.pop(i) for i in idx]
        joins += 1
        node = tree.Node(name=f"N{joins}", children=kids)
        for c in kids:
            c.parent = node
        pool.append(node)
    root = tree.Node(name="root", children=pool)
    for c in pool:
        c.parent = root
    flat = tree.flatten(root)
    L, B = flat.L, flat.n_branches
    palette = np.unique(np.r_[rng.choice(D, size=min(D, 3), replace=False), D - 1])
    half = S // 2
    base = rng.choice(palette, size=half)
    p_leaf = rng.choice([0.0, 0.0, 0.0, 0.03, 0.15], size=(L, 1))   # (conserved leaves: subtrees of a handful of classes even at 5 %)
    fp = np.asarray(flat.flat_parents, dtype=np.int64)
    only_leaves = sorted(set(fp[:L].tolist()) - set(fp[L:].tolist()))
    cherry = fp[:L] == only_leaves[int(rng.integers(len(only_leaves)))]
    p_leaf[cherry] = -1.0                                               # (one node below leaves alone: compressed at any threshold)
    codes = np.where(rng.random((L, half)) < p_leaf, rng.choice(palette, size=(L, half)), base[None, :])
    codes = np.concatenate([codes, codes], axis=1).astype(np.int64)
    n_amb = 3
    ambig = (rng.random((n_amb, D)) < 0.5).astype(np.float64)
    ambig[:, D - 1] = 1.0
    mask = rng.random((L, S)) < np.where(p_leaf > 0, 0.03, np.where(p_leaf == 0, 0.004, 0.0))
    codes[mask] = -rng.integers(1, n_amb + 1, size=int(mask.sum()))
    pi = rng.random(D) + 0.05
    return dict(D=np.int64(D), L=np.int64(L), flat_parents=fp, leaf_codes=codes,
                ambig=ambig, pattern_freq=rng.integers(1, 5, size=S).astype(np.int64), root_freqs=pi / pi.sum(),
                Q=random_rates(rng, B, D))
