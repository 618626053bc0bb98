"""numpy restatement of hyphy_hip_sample_ancestral (include/hyphy_hip.h; the reference's _TheTree::SampleAncestorsBySequence,
tree.cpp:4133-4174), taking the conditionals as input, and a numpy Philox4x32-10.

Per draw (replicate r, site j, internal node n), with s = pattern_of_site[j], c = class_of_pattern[s] and in_n = cond[c][n][s]:
    root (n = I-1):  w[i] = pi[i] * in_n[i];   otherwise:  w[i] = P[c][L + n][state of the parent][i] * in_n[i]
    cum_i = w[0] + ... + w[i], ascending i, every addition rounded (np.add.accumulate is that serial sum);  total = cum_{D-1}
    x = u * total;   state = the smallest i with cum_i >= x and cum_i > 0
Two deviations from the reference: total == 0 or NaN gives -1 and every descendant of a -1 node is -1; u == 0 picks the first
state of positive weight."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10: ``counter`` [..., 4], ``key`` [..., 2] (32-bit words, broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] & MASK for i in range(4))
    k0, k1 = k[..., 0] & MASK, k[..., 1] & MASK
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SH) ^ c1 ^ k0, p1 & MASK, (p0 >> SH) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def uniforms(seed, n_rep, I, n_sites, sites=None, reps=None):
    """[n_rep, I, n_sites] uniforms of the draws: key = (seed low, seed high), counter = (site, node, replicate, 0),
    u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53.  ``sites`` / ``reps``: the site / replicate numbers to use instead of
    0 .. n - 1 (a call split into parts)."""
    seed = int(seed) & (2 ** 64 - 1)
    j = np.arange(n_sites, dtype=np.uint64) if sites is None else np.asarray(sites, dtype=np.uint64)
    r = np.arange(n_rep, dtype=np.uint64) if reps is None else np.asarray(reps, dtype=np.uint64)
    n = np.arange(I, dtype=np.uint64)
    ctr = np.zeros((len(r), I, len(j), 4), dtype=np.uint64)
    ctr[..., 0] = j[None, None, :]
    ctr[..., 1] = n[None, :, None]
    ctr[..., 2] = r[:, None, None]
    x = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    return (((x[..., 0] >> np.uint64(5)) << np.uint64(26)) + (x[..., 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def sample_ref(flat_parents, L, cond, P, pi, u, pattern_of_site=None, class_of_pattern=None, near_tol=None):
    """States int8 [n_rep, I, n_sites] (-1: impossible pattern, and everything below it).
    ``cond``: [I, S, D] stored conditionals, or [C, I, S, D]; ``P``: [B, D, D] by node code, or [C, B, D, D]; ``u``: [n_rep, I, n_sites].
    ``near_tol``: also return a boolean [n_rep, n_sites]: some node of the column has |cum_i - u total| <= near_tol * total for some i."""
    fp = np.asarray(flat_parents, dtype=np.int64)
    L = int(L)
    I = len(fp) - L
    cond = np.asarray(cond, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    if cond.ndim == 3:
        cond, P = cond[None], P[None]
    S, D = cond.shape[2], cond.shape[3]
    pi = np.asarray(pi, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    R, n_sites = u.shape[0], u.shape[2]
    assert u.shape[1] == I
    pos = np.arange(S) if pattern_of_site is None else np.asarray(pattern_of_site, dtype=np.int64)
    assert pos.shape == (n_sites,)
    cls = (np.zeros(S, dtype=np.int64) if class_of_pattern is None else np.asarray(class_of_pattern, dtype=np.int64))[pos]
    states = np.full((R, I, n_sites), -1, dtype=np.int8)
    near = np.zeros((R, n_sites), dtype=bool)
    for n in range(I - 1, -1, -1):
        inn = cond[cls, n, pos]                                       # [n_sites, D]
        if n == I - 1:
            alive = np.ones((R, n_sites), dtype=bool)
            row = np.broadcast_to(pi, (R, n_sites, D))
        else:
            ps = states[:, int(fp[L + n]), :].astype(np.int64)         # [R, n_sites]
            alive = ps >= 0
            row = P[cls[None, :], L + n, np.maximum(ps, 0)]           # [R, n_sites, D]
        w = row * inn[None]                                           # one rounded product
        cum = np.add.accumulate(w, axis=2)                            # serial, ascending i
        total = cum[..., -1]
        x = u[:, n, :] * total
        with np.errstate(invalid="ignore"):
            hit = (cum >= x[..., None]) & (cum > 0)
            ok = alive & (total > 0)
        st = np.where(hit.any(axis=2) & ok, hit.argmax(axis=2), -1)
        states[:, n, :] = st
        if near_tol is not None:
            with np.errstate(invalid="ignore"):
                close = (np.abs(cum - x[..., None]) <= near_tol * total[..., None]).any(axis=2)
            near |= close & ok
    return (states, near) if near_tol is not None else states
