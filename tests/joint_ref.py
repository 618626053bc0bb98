"""The joint maximum-likelihood reconstruction of _TheTree::RecoverAncestralSequences (src/core/tree.cpp:4209-4510), restated in
numpy with unbounded range: every number is a pair (mantissa in [0.5, 1) or 0, integer exponent), renormalised by ``frexp`` after
every multiplication.  frexp / ldexp are exact and a product of two mantissas in [0.5, 1) rounds as the product of the doubles they
stand for does, so every decision is the one float64 arithmetic takes wherever it neither underflows nor overflows — and the one
it would take with unbounded exponents where it does.

The contract, per pattern, with the matrices of ONE rate class (catAssignments, tree.cpp:4303-4308):
  upward (:4252-4407), nodes in ascending node code (leaves 0..L-1, internal L+i, the root excluded): the parent's vector starts at
  all ones (:4266-4271); a leaf with state s >= 0 does m_parent[p] *= P[p][s] (:4315-4327, backpointer s for every p); otherwise
  v = the leaf's ambiguity row or the internal node's own vector: all D entries exactly 1.0 -> completely unresolved (:4350-4355,
  backpointer -1, no contribution), else msg[p] = max_c P[p][c] v[c], arg[p] the FIRST c attaining it (strict >, from 0: :4357-4377)
  and m_parent[p] *= msg[p] (:4390-4394);
  root (:4434-4457): all D entries exactly 1 -> every node -1 (:4484-4486), else the first argmax of pi[c] m_root[c];
  traceback (:4458-4483): state[n] = arg_n[state[parent]], -1 when the parent is -1.
Node numbering as in tests/scalefree.py.
"""
import numpy as np

from tests.scalefree import children_of


def _norm(m, e):
    m2, de = np.frexp(m)
    return m2, np.where(m2 == 0, 0, e + de)


def _mul(a, b):
    return _norm(a[0] * b[0], a[1] + b[1])


def _split(x):
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return m, e.astype(np.int64)


def _first_max(m, e):
    """Along the last axis: index of the first maximum under strict > starting from 0 (an all-zero row: 0), and the margin
    1 - runner-up / best (1 when the best is 0 or stands alone against zeros)."""
    nz = m > 0
    big = np.where(nz, e, np.iinfo(np.int64).min)
    top = big.max(axis=-1, keepdims=True)
    cand = nz & (big == top)
    mm = np.where(cand, m, 0.0)
    arg = mm.argmax(axis=-1)                     # (argmax returns the first of equal values)
    best = np.take_along_axis(mm, arg[..., None], axis=-1)[..., 0]
    # runner-up: the largest value at another index
    rest_m = m.copy()
    np.put_along_axis(rest_m, arg[..., None], 0.0, axis=-1)
    de = np.clip(np.where(rest_m > 0, e - top, -4000), -4000, 0)
    ratio = np.where(best[..., None] > 0, np.ldexp(rest_m, de.astype(np.int32)) / np.where(best > 0, best, 1.0)[..., None], 0.0)
    return arg, 1.0 - ratio.max(axis=-1)


def _maxprod(Pm, Pe, v):
    """msg[p] = max_c P[p][c] v[c] (normalised pairs), its first argmax and the margin of each row."""
    m, e = _norm(Pm * v[0][None, :], Pe + v[1][None, :])
    arg, margin = _first_max(m, e)
    idx = np.arange(m.shape[0])
    return (m[idx, arg], e[idx, arg]), arg, margin


def _one_pattern(D, L, I, ch, fp, codes, amb, Ps, pi, do_leaves):
    """states [I + L] (leaves filled only with do_leaves) and the smallest margin on the traced path."""
    ones = lambda: (np.full(D, 0.5), np.ones(D, dtype=np.int64))      # noqa: E731  (1.0 = 0.5 x 2^1)
    vec = [None] * I
    arg_of = {}          # node code -> (arg [D] or None for a resolved leaf's constant / -1, margins [D])
    for n in range(I):
        m = ones()
        for c in ch[n]:
            Pm, Pe = Ps[c]
            if c < L and codes[c] >= 0:
                s = int(codes[c])
                m = _mul(m, (Pm[:, s], Pe[:, s]))
                arg_of[c] = (np.full(D, s), np.ones(D))
                continue
            v = _split(amb[-int(codes[c]) - 1]) if c < L else vec[c - L]
            if np.all((v[0] == 0.5) & (v[1] == 1)):
                arg_of[c] = (np.full(D, -1), np.ones(D))
                continue
            msg, arg, margin = _maxprod(Pm, Pe, v)
            arg_of[c] = (arg, margin)
            m = _mul(m, msg)
        vec[n] = m
    states = np.full(I + L, -1, dtype=np.int64)
    worst = 1.0
    root = vec[I - 1]
    if np.all((root[0] == 0.5) & (root[1] == 1)):
        return states, worst
    pm, pe = _split(pi)
    rm, re = _norm(pm * root[0], pe + root[1])
    arg, margin = _first_max(rm[None, :], re[None, :])
    states[I - 1] = int(arg[0])
    worst = min(worst, float(margin[0]))
    for n in range(I - 2, -1, -1):
        ps = states[fp[L + n]]
        if ps >= 0:
            a, mg = arg_of[L + n]
            states[n] = a[ps]
            if a[ps] >= 0:
                worst = min(worst, float(mg[ps]))
    if do_leaves:
        for l in range(L):
            ps = states[fp[l]]
            if ps >= 0:
                a, mg = arg_of[l]
                states[I + l] = a[ps]
                if a[ps] >= 0 and codes[l] < 0:
                    worst = min(worst, float(mg[ps]))
    return states, worst


def joint_ref(D, flat_parents, L, leaf_codes, ambig, P, root_freqs, class_of_pattern=None, do_leaves=True):
    """states int64 [I (+ L), S] (rows as hyphy_hip_joint_ancestral's) and the smallest decision margin of each pattern [S].
    ``P``: [B, D, D] by node code, or [C, B, D, D] with ``class_of_pattern`` [S]."""
    D, L = int(D), int(L)
    fp = np.asarray(flat_parents, dtype=np.int64)
    I = len(fp) - L
    codes = np.asarray(leaf_codes, dtype=np.int64)
    S = codes.shape[1]
    amb = np.asarray(ambig, dtype=np.float64) if ambig is not None and len(ambig) else np.ones((1, D))
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        P = P[None]
    cls = np.zeros(S, dtype=np.int64) if class_of_pattern is None else np.asarray(class_of_pattern, dtype=np.int64)
    ch = children_of(fp, L)
    split = {}
    out = np.full((I + (L if do_leaves else 0), S), -1, dtype=np.int64)
    margins = np.ones(S)
    for s in range(S):
        c = int(cls[s])
        if c not in split:
            split[c] = [_split(P[c, b]) for b in range(P.shape[1])]
        st, worst = _one_pattern(D, L, I, ch, fp, codes[:, s], amb, split[c], root_freqs, do_leaves)
        out[:, s] = st[: out.shape[0]]
        margins[s] = worst
    return out, margins


def joint_plain(D, flat_parents, L, leaf_codes, ambig, P, root_freqs, do_leaves=True):
    """The same pass in plain float64 with the reference's own rescaling only — msg multiplied by 2^64 ONCE when its maximum is
    below 2^-64 (:4379-4383), the factors of resolved leaves never: what the device must NOT copy (it underflows on wide
    polytomies and then returns state 0 everywhere)."""
    D, L = int(D), int(L)
    fp = np.asarray(flat_parents, dtype=np.int64)
    I = len(fp) - L
    codes = np.asarray(leaf_codes, dtype=np.int64)
    S = codes.shape[1]
    amb = np.asarray(ambig, dtype=np.float64) if ambig is not None and len(ambig) else np.ones((1, D))
    P = np.asarray(P, dtype=np.float64)
    ch = children_of(fp, L)
    out = np.full((I + (L if do_leaves else 0), S), -1, dtype=np.int64)

    def first_max(x):
        best, arg = 0.0, 0
        for c in range(len(x)):
            if x[c] > best:
                best, arg = x[c], c
        return best, arg
    for s in range(S):
        vec = [None] * I
        args = {}
        for n in range(I):
            m = np.ones(D)
            for c in ch[n]:
                if c < L and codes[c, s] >= 0:
                    m = m * P[c][:, codes[c, s]]
                    args[c] = np.full(D, codes[c, s])
                    continue
                v = amb[-codes[c, s] - 1] if c < L else vec[c - L]
                if np.all(v == 1.0):
                    args[c] = np.full(D, -1)
                    continue
                pairs = [first_max(P[c][p] * v) for p in range(D)]
                msg = np.array([b for b, _ in pairs])
                args[c] = np.array([a for _, a in pairs])
                if 0.0 < msg.max() < 2.0 ** -64:
                    msg = msg * 2.0 ** 64
                m = m * msg
            vec[n] = m
        st = np.full(I + L, -1, dtype=np.int64)
        if not np.all(vec[I - 1] == 1.0):
            st[I - 1] = first_max(np.asarray(root_freqs) * vec[I - 1])[1]
            for n in range(I - 2, -1, -1):
                ps = st[fp[L + n]]
                st[n] = args[L + n][ps] if ps >= 0 else -1
            for l in range(L):
                ps = st[fp[l]]
                st[I + l] = args[l][ps] if ps >= 0 else -1
        out[:, s] = st[: out.shape[0]]
    return out


def joint_probability(states, D, flat_parents, L, leaf_codes, ambig, P, root_freqs):
    """Probability of ONE pattern's complete assignment ``states`` [I + L] (leaf_codes [L]) as (mantissa, exponent): pi at the
    root, P[child][state of parent][state of child] on every branch whose two ends have states, amb[state] at a leaf with an
    ambiguity code; a node at -1 (and so its whole subtree) is marginalised: factor 1."""
    D, L = int(D), int(L)
    fp = np.asarray(flat_parents, dtype=np.int64)
    I = len(fp) - L
    st = np.asarray(states, dtype=np.int64)
    amb = np.asarray(ambig, dtype=np.float64) if ambig is not None and len(ambig) else np.ones((1, D))
    m, e = 0.5, 1
    if st[I - 1] < 0:
        return m, e

    def mul(x):
        nonlocal m, e
        xm, xe = np.frexp(float(x))
        mm, de = np.frexp(m * xm)
        m, e = float(mm), (0 if mm == 0 else e + int(xe) + int(de))
    mul(root_freqs[st[I - 1]])
    for n in range(I - 1):
        ps = st[fp[L + n]]
        if ps >= 0 and st[n] >= 0:
            mul(P[L + n][ps, st[n]])
    for l in range(L):
        ps, x = st[fp[l]], st[I + l]
        if ps >= 0 and x >= 0:
            mul(P[l][ps, x])
            if leaf_codes[l] < 0:
                mul(amb[-int(leaf_codes[l]) - 1][x])
    return m, e


# ---- cases shared by the CPU and the GPU tests -----------------------------------------------------------------------------------

def tie_case():
    """Equal rates at 4 states, every leaf of the 4-leaf tree in another state: every comparison is a tie, the first index wins."""
    fp = np.array([0, 0, 1, 1, 2, 2, -1], dtype=np.int64)
    P = np.full((6, 4, 4), 0.125)
    P[:, np.arange(4), np.arange(4)] = 0.625
    codes = np.array([[0], [1], [2], [3]], dtype=np.int64)
    return 4, fp, 4, codes, np.ones((1, 4)), P, np.full(4, 0.25)


def wide_star(n=96, eps=1e-6):
    """A star of ``n`` leaves below the root at 4 states, branch lengths ~eps, the leaf states cycling; one cherry beside it so
    that the tree has an internal branch."""
    L = n + 2
    fp = np.array([1] * n + [0, 0] + [1, -1], dtype=np.int64)
    P = np.full((L + 1, 4, 4), eps)
    P[:, np.arange(4), np.arange(4)] = 1.0 - 3 * eps
    codes = np.zeros((L, 3), dtype=np.int64)              # (the cherry's leaves: state 0)
    for s in range(3):
        codes[:n, s] = (np.arange(n) + s) % 4
        codes[:8, s] = s + 1                              # state s + 1 has 30 leaves or more, every other at most 24
    return 4, fp, L, codes, np.ones((1, 4)), P, np.array([0.1, 0.2, 0.3, 0.4])
