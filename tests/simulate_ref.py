"""numpy restatement of hyphy_hip_simulate (include/hyphy_hip.h; the reference's _LikelihoodFunction::Simulate with BuildLeafProbs,
likefunc.cpp:12584-13259, and DrawFromDiscrete, function_templates.h:404-413).

A column is (replicate r, site j) with rate class c = class_of_site[r][j].  Nodes parent-first; per node n of a column:
    root (node code L+I-1):  row = pi (or the supplied root state);   otherwise:  row = P[c][n][state of the parent]
    cum_i = row[0] + ... + row[i], ascending i, every addition rounded (np.add.accumulate is that serial sum);  total = cum_{D-1}
    x = u * total;   state = the smallest i with cum_i >= x and cum_i > 0
Three deviations from the reference: x = u * total instead of x = u; u == 0 picks the first state of positive weight; total <= 0
or NaN gives -1 and every descendant of a -1 node is -1."""
import numpy as np

from tests import sample_ref as sr


def uniforms(seed, n_rep, n_nodes, n_sites, sites=None, reps=None):
    """[n_rep, n_nodes, n_sites] uniforms of the draws: key = (seed low, seed high), counter = (site, node code, replicate, 1),
    u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53.  ``sites`` / ``reps``: the site / replicate numbers to use instead of 0 .. n - 1."""
    seed = int(seed) & (2 ** 64 - 1)
    j = np.arange(n_sites, dtype=np.uint64) if sites is None else np.asarray(sites, dtype=np.uint64)
    r = np.arange(n_rep, dtype=np.uint64) if reps is None else np.asarray(reps, dtype=np.uint64)
    n = np.arange(n_nodes, dtype=np.uint64)
    ctr = np.ones((len(r), n_nodes, len(j), 4), dtype=np.uint64)            # the last word: 1 (sample_ancestral: 0)
    ctr[..., 0] = j[None, None, :]
    ctr[..., 1] = n[None, :, None]
    ctr[..., 2] = r[:, None, None]
    x = sr.philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    return (((x[..., 0] >> np.uint64(5)) << np.uint64(26)) + (x[..., 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def draw(row, u, use_max=False):
    """One node of many columns: ``row`` [..., D], ``u`` [...] -> (state [...] with -1 where total <= 0 or NaN, cum, x, total).
    ``use_max``: search the running maximum of cum instead of cum (what the device does; the same answer)."""
    cum = np.add.accumulate(row, axis=-1)                               # serial, ascending i
    total = cum[..., -1]
    x = u * total
    key = np.maximum.accumulate(cum, axis=-1) if use_max else cum
    with np.errstate(invalid="ignore"):
        hit = (key >= x[..., None]) & (key > 0)
        ok = total > 0
    return np.where(hit.any(axis=-1) & ok, hit.argmax(axis=-1), -1), cum, x, total


def simulate_ref(flat_parents, L, P, pi, u, class_of_site=None, root_states=None, near_tol=None, use_max=False):
    """States int8 [n_rep, L + I, n_sites] by node code.  ``P``: [B, D, D] by node code, or [C, B, D, D]; ``u``: [n_rep, L + I, n_sites];
    ``class_of_site`` / ``root_states``: [n_rep, n_sites] or None.  ``near_tol``: also return a boolean [n_rep, n_sites]: some node of
    the column has |cum_i - u total| <= near_tol * total for some i (a near-tie: another rounding of P could draw another state)."""
    fp = np.asarray(flat_parents, dtype=np.int64)
    L = int(L)
    rows = len(fp)
    I = rows - L
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        P = P[None]
    D = P.shape[-1]
    pi = np.asarray(pi, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    R, n_sites = u.shape[0], u.shape[2]
    assert u.shape[1] == rows
    cls = np.zeros((R, n_sites), dtype=np.int64) if class_of_site is None else np.asarray(class_of_site, dtype=np.int64)
    assert cls.shape == (R, n_sites)
    states = np.full((R, rows, n_sites), -1, dtype=np.int8)
    near = np.zeros((R, n_sites), dtype=bool)
    for node in list(range(rows - 1, L - 1, -1)) + list(range(L)):      # internal nodes in descending index, then the leaves
        if node == rows - 1:
            alive = np.ones((R, n_sites), dtype=bool)
            row = np.broadcast_to(pi, (R, n_sites, D))
        else:
            ps = states[:, L + int(fp[node]), :].astype(np.int64)
            alive = ps >= 0
            row = P[cls, node, np.maximum(ps, 0)]                       # [R, n_sites, D]
        st, cum, x, total = draw(row, u[:, node, :], use_max)
        if node == rows - 1 and root_states is not None:
            st = np.asarray(root_states, dtype=np.int64)
            assert st.shape == (R, n_sites) and st.min() >= 0 and st.max() < D
        else:
            st = np.where(alive, st, -1)
            if near_tol is not None:
                with np.errstate(invalid="ignore"):
                    close = (np.abs(cum - x[..., None]) <= near_tol * total[..., None]).any(axis=-1)
                near |= close & alive & (total > 0)
        states[:, node, :] = st
    return (states, near) if near_tol is not None else states


# ---- the 3-leaf, 4-state distribution case of the CPU and the device test -----------------------------------------------------------
DIST_FP, DIST_L, DIST_D = np.array([0, 0, 1, 1, -1], dtype=np.int64), 3, 4      # ((leaf 0, leaf 1) node 0, leaf 2) root
DIST_COLUMNS = 200_000
CHI2_BOUND = 132.0      # the 1 - 1e-6 quantile of chi^2 with 63 degrees of freedom (Wilson-Hilferty: 63 (1 - 2/567 + 4.7534 sqrt(2/567))^3)
CHI2_SEED_BOUND = 92.0  # its 0.99 quantile: the fixed seed's statistic lies below it


def dist_case(seed=2024):
    """Random non-reversible rate matrices Q [4, 4, 4] (by node code; moderate branch lengths) and a random pi."""
    rng = np.random.default_rng(seed)
    Q = rng.random((4, 4, 4)) * rng.uniform(0.1, 0.6, size=(4, 1, 1))
    Q[:, np.arange(4), np.arange(4)] = 0.0
    Q[:, np.arange(4), np.arange(4)] = -Q.sum(axis=2)
    pi = rng.random(4) + 0.1
    return Q, pi / pi.sum()


def pattern_probabilities(P, pi):
    """Brute force over the internal states: probability of each of the 64 leaf patterns, index = 16 a + 4 b + c (leaves 0, 1, 2)."""
    # root state r, node-0 state k: pi[r] P3[r][k] P0[k][a] P1[k][b] P2[r][c]   (node codes: leaves 0-2, node 0 -> 3)
    pr = np.einsum("r,rk,ka,kb,rc->abc", pi, P[3], P[0], P[1], P[2])
    return pr.reshape(64)


def chi2_of_leaves(states, prob):
    """Pearson chi^2 of the leaf patterns of ``states`` [n_rep, >= 3, n_sites] against ``prob`` [64] (of the patterns' total)."""
    leaves = states[:, :3, :].astype(np.int64)
    assert leaves.min() >= 0
    idx = (16 * leaves[:, 0] + 4 * leaves[:, 1] + leaves[:, 2]).reshape(-1)
    n = np.bincount(idx, minlength=64).astype(np.float64)
    e = prob / prob.sum() * len(idx)
    return float(((n - e) ** 2 / e).sum())
