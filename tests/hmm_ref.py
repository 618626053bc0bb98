"""Extended-precision references for the hidden-Markov rate-class entry points (include/hyphy_hip.h, "Hidden-Markov rate classes").

Inputs everywhere: ``l`` [C, S] per-class per-pattern likelihoods, ``c`` [C, S] their 2^64 exponents (value = l * 2^(-64 c)),
``T`` [C, C] row-major transition matrix, ``pi`` [C], ``sites`` [N] pattern of each site (None: site j = pattern j).

  forward_mp   log of  pi^T [ prod_{i=0}^{N-2} T diag(e_i) ] e_{N-1}  in 60 digits (-inf: the sum is 0; nan: a used value is NaN)
  viterbi_mp   a path maximising log(pi[z0] e_0[z0]) + sum_{i>=1} log(T[z_{i-1}][z_i] e_i[z_i]), and `margins` of its recursion
  brute        both by enumeration of all C^N state sequences
  margins      the smallest gap between the best and the second-best candidate over every decision of the Viterbi recursion
  bar          the absolute bound on log L a float64 forward sum is held to
"""
import itertools
import math

import mpmath as mp
import numpy as np

DPS = 60


def bar(N, C, logl):
    """2 [ (N+2)(C+2) 2^-53 + 4 2^-53 |log L| ]: every term is non-negative and goes through at most N-1 matrix products (gamma_C each)
    and one T.e rounding per site; rescaling is exact; the final dot, the log and exponent*ln2 add a few ulps of |log L|; margin 2."""
    return 2.0 * ((N + 2) * (C + 2) * 2.0 ** -53 + 4 * 2.0 ** -53 * abs(logl))


def _prep(l, c, T, pi, sites):
    l = np.asarray(l, dtype=np.float64)
    c = np.asarray(c, dtype=np.int64)
    T = np.asarray(T, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64)
    sites = np.arange(l.shape[1]) if sites is None else np.asarray(sites, dtype=np.int64)
    used = l[:, sites]
    has_nan = bool(np.isnan(used).any() or np.isnan(T).any() or np.isnan(pi).any())
    return l, c, T, pi, sites, has_nan


def _emissions(l, c, sites):
    C = l.shape[0]
    two = mp.mpf(2)
    cache = {}
    out = []
    for s in sites:
        s = int(s)
        if s not in cache:
            cache[s] = [mp.mpf(float(l[m, s])) * two ** (-64 * int(c[m, s])) for m in range(C)]
        out.append(cache[s])
    return out


def forward_mp(l, c, T, pi, sites=None):
    l, c, T, pi, sites, has_nan = _prep(l, c, T, pi, sites)
    if has_nan:
        return mp.nan
    with mp.workdps(DPS):
        C = l.shape[0]
        e = _emissions(l, c, sites)
        Tm = [[mp.mpf(float(T[k, m])) for m in range(C)] for k in range(C)]
        v = list(e[-1])
        for i in range(len(sites) - 2, -1, -1):
            w = [e[i][m] * v[m] for m in range(C)]
            v = [mp.fsum(Tm[k][m] * w[m] for m in range(C)) for k in range(C)]
        L = mp.fsum(mp.mpf(float(pi[k])) * v[k] for k in range(C))
        return mp.log(L) if L > 0 else -mp.inf


def _log(x):
    return mp.log(x) if x > 0 else -mp.inf


def _viterbi(l, c, T, pi, sites):
    """(path or None, smallest decision margin)"""
    C = l.shape[0]
    N = len(sites)
    e = _emissions(l, c, sites)
    lT = [[_log(mp.mpf(float(T[k, m]))) for m in range(C)] for k in range(C)]
    le_cache = {}

    def le(i):
        s = int(sites[i])
        if s not in le_cache:
            le_cache[s] = [_log(x) for x in e[i]]
        return le_cache[s]

    def decide(cands):
        order = sorted(range(len(cands)), key=lambda k: (-cands[k], k))
        best = order[0]
        if cands[best] == -mp.inf:
            return best, mp.inf  # (nothing to decide: every candidate is impossible)
        gap = cands[best] - cands[order[1]] if len(cands) > 1 else mp.inf
        return best, gap

    delta = [_log(mp.mpf(float(pi[k]))) + le(0)[k] for k in range(C)]
    back = []
    gap_min = mp.inf
    for i in range(1, N):
        lei = le(i)
        nd, bp = [], []
        for m in range(C):
            k, gap = decide([delta[k] + lT[k][m] for k in range(C)])
            gap_min = min(gap_min, gap)
            nd.append(delta[k] + lT[k][m] + lei[m])
            bp.append(k)
        delta = nd
        back.append(bp)
    z, gap = decide(delta)
    gap_min = min(gap_min, gap)
    if delta[z] == -mp.inf:
        return None, gap_min
    path = [z]
    for bp in reversed(back):
        path.append(bp[path[-1]])
    return np.array(path[::-1], dtype=np.int8), gap_min


def viterbi_mp(l, c, T, pi, sites=None):
    """The path (all -1: no path of positive probability, or a used value is NaN)."""
    l, c, T, pi, sites, has_nan = _prep(l, c, T, pi, sites)
    if has_nan:
        return np.full(len(sites), -1, dtype=np.int8)
    with mp.workdps(DPS):
        path, _ = _viterbi(l, c, T, pi, sites)
    return np.full(len(sites), -1, dtype=np.int8) if path is None else path


def margins(l, c, T, pi, sites=None):
    l, c, T, pi, sites, has_nan = _prep(l, c, T, pi, sites)
    if has_nan:
        return 0.0
    with mp.workdps(DPS):
        _, gap = _viterbi(l, c, T, pi, sites)
        return float(gap)


def brute(l, c, T, pi, sites=None):
    """(log L of the forward sum, a best Viterbi path, its log score) over all C^N state sequences."""
    l, c, T, pi, sites, has_nan = _prep(l, c, T, pi, sites)
    assert not has_nan
    with mp.workdps(DPS):
        C = l.shape[0]
        N = len(sites)
        e = _emissions(l, c, sites)
        Tm = [[mp.mpf(float(T[k, m])) for m in range(C)] for k in range(C)]
        pm = [mp.mpf(float(x)) for x in pi]
        total = mp.mpf(0)
        best, best_path = -mp.inf, None
        for z in itertools.product(range(C), repeat=N):
            # the forward sum's term: site i < N-1 is read in the state AFTER its transition, the last site in the last state
            t = pm[z[0]]
            for i in range(N - 1):
                t *= Tm[z[i]][z[i + 1]] * e[i][z[i + 1]]
            total += t * e[N - 1][z[N - 1]]
            s = pm[z[0]] * e[0][z[0]]
            for i in range(1, N):
                s *= Tm[z[i - 1]][z[i]] * e[i][z[i]]
            ls = _log(s)
            if ls > best:
                best, best_path = ls, z
        return _log(total), (None if best_path is None else np.array(best_path, dtype=np.int8)), best


def path_score(l, c, T, pi, sites, path):
    l, c, T, pi, sites, _ = _prep(l, c, T, pi, sites)
    with mp.workdps(DPS):
        e = _emissions(l, c, sites)
        s = _log(mp.mpf(float(pi[path[0]])) * e[0][path[0]])
        for i in range(1, len(sites)):
            s += _log(mp.mpf(float(T[path[i - 1], path[i]])) * e[i][path[i]])
        return s


def to_float(x):
    return float("nan") if mp.isnan(x) else float(x)


def random_chain(rng, C, lo=0.02):
    """An asymmetric transition matrix with entries >= lo whose columns do not sum to 1, and an initial vector that is not stationary."""
    while True:  # (redraw until it is all of that)
        R = rng.uniform(0.0, 1.0, size=(C, C)) ** 2 + np.diag(rng.uniform(1.0, 3.0, size=C))
        T = lo + (1.0 - C * lo) * R / R.sum(axis=1, keepdims=True)
        pi = rng.uniform(0.2, 1.0, size=C)
        pi /= pi.sum()
        if (T.min() >= lo and np.abs(T.sum(axis=0) - 1).max() > 1e-2 and np.abs(T - T.T).max() > 1e-2
                and np.abs(pi @ T - pi).max() > 1e-2):
            return T, pi
