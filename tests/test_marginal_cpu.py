"""CPU-only checks of marginal ancestral reconstruction (hyphy_hip_marginal_ancestral): the ABI names, the NULL-partition error,
the pre-order program the device pass walks, and a numpy restatement that executes that program on the golden fixture and
reproduces the REAL reference's support matrix (ReconstructAncestors (lf, MARGINAL))."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hyphy_hip_marginal_ancestral", "hyphy_hip_plan_marginal")


def _hip():
    import __graft_entry__ as g
    g.build()
    from hyphy_amd import hip
    return hip


def test_header_library_and_exports_agree():
    hip = _hip()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyphy_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hyphy_hip_[a-z_]+)\s*\(", txt))
    lib = ctypes.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in hip.EXPORTS, n


def test_null_partition_is_a_hard_error():
    hip = _hip()
    lib = hip.load()
    assert lib.hyphy_hip_marginal_ancestral(None, 0, None, None, None, None) < 0
    assert b"NULL" in lib.hyphy_hip_last_error()


def test_plan_rejects_bad_trees():
    hip = _hip()
    with pytest.raises(hip.HipError):
        hip.plan_marginal(np.array([0, 0, 5, -1]), 2)   # (parent index out of range)


def _children(fp, L):
    I = len(fp) - L
    ch = [[] for _ in range(I)]
    for c in range(L + I - 1):
        ch[int(fp[c])].append(c)
    return ch


def _check_program(fp, L):
    hip = _hip()
    fp = np.asarray(fp, dtype=np.int64)
    I = len(fp) - L
    B = L + I - 1
    plan = hip.plan_marginal(fp, L)
    ent = plan["entries"]
    ch = _children(fp, L)
    seen_node, pairs, pos, k = set(), set(), 0, 0
    # what the kernel does per node of k children: k edge products (prefix pass), k - 1 prefix and k - 1 suffix multiplications
    # (+ 1 for the node's own support), a transposed product per internal child, and per leaf child in the leaf form
    edge_products = elementwise = transposed_internal = transposed_leaf = 0
    while pos < len(ent):
        kind, n, kids, is_root = ent[pos]
        assert kind == 0
        assert is_root == (1 if n == I - 1 else 0)
        if n != I - 1:
            assert int(fp[L + n]) in seen_node, "visited before its parent"
        assert n not in seen_node
        seen_node.add(n)
        assert kids == len(ch[n])
        edge_products += kids
        elementwise += 2 * kids - 1
        for j in range(kids):
            kind, c, ci, p = ent[pos + 1 + j]
            assert kind == 1 and p == j
            assert ci == (c - L if c >= L else -1)
            assert int(fp[c]) == n
            assert (n, c) not in pairs
            pairs.add((n, c))
            if ci >= 0:
                transposed_internal += 1
            else:
                transposed_leaf += 1
        pos += 1 + kids
        k = max(k, kids)
    assert seen_node == set(range(I))
    assert len(pairs) == B
    assert plan["maxk"] == k
    assert edge_products == B and transposed_internal == I - 1 and transposed_leaf == L
    assert edge_products + transposed_internal <= 2 * B                     # the internal form
    assert edge_products + transposed_internal + transposed_leaf <= 2 * B + L   # the leaf form
    assert elementwise <= 2 * B                                             # sibling products: linear, not k^2 per node
    return plan


@pytest.mark.parametrize("name", ["codon_small_marginal", "codon_deep"])
def test_plan_visits_parents_first_fixtures(name):
    fx = common.load(name)
    _check_program(fx["flat_parents"], int(fx["L"]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plan_visits_parents_first_multifurcating(seed):
    fx = common.compressible_case(20, seed)
    ch = _children(fx["flat_parents"], int(fx["L"]))
    assert max(len(c) for c in ch) >= 3
    _check_program(fx["flat_parents"], int(fx["L"]))


def numpy_marginal(plan, P, fp, L, leaf_codes, ambig, pi, which="internal"):
    """Execute the decoded program in numpy (no rescaling: small trees only).  P [B, D, D]; returns [rows, S, D]."""
    fp = np.asarray(fp, dtype=np.int64)
    I = len(fp) - L
    D = P.shape[1]
    S = leaf_codes.shape[1]
    amb = np.asarray(ambig, dtype=np.float64).reshape(-1, D)

    def leafvec(l):
        c = leaf_codes[l]
        v = np.zeros((S, D))
        pos = c >= 0
        v[np.flatnonzero(pos), c[pos]] = 1.0
        if (~pos).any():
            v[~pos] = amb[-c[~pos] - 1]
        return v

    ch = _children(fp, L)
    inside = [None] * I
    for n in range(I):   # (children before parents)
        v = np.ones((S, D))
        for c in ch[n]:
            v = v * ((leafvec(c) if c < L else inside[c - L]) @ P[c].T)
        inside[n] = v
    U = [None] * I
    out = np.zeros((I if which == "internal" else L, S, D))
    ent = plan["entries"]
    pos = 0
    while pos < len(ent):
        _, n, k, is_root = ent[pos]
        u = np.broadcast_to(pi, (S, D)).copy() if is_root else U[n]
        kids = [ent[pos + 1 + j] for j in range(k)]
        E = [((leafvec(c) if ci < 0 else inside[ci]) @ P[c].T) for _, c, ci, _ in kids]
        pre = [u]
        for e in E[:-1]:
            pre.append(pre[-1] * e)
        suf = np.ones((S, D))
        for j in range(k - 1, -1, -1):
            _, c, ci, _ = kids[j]
            V = pre[j] * suf
            Uc = V @ P[c]
            if ci >= 0:
                U[ci] = Uc
            elif which == "leaves":
                out[c] = Uc / (Uc * leafvec(c)).sum(1, keepdims=True)
            suf = suf * E[j]
        if which == "internal":
            num = pre[-1] * E[-1]
            out[n] = num / num.sum(1, keepdims=True)
        pos += 1 + k
    return out


def _match_rows(ours, ref):
    used = set()
    for i in range(ours.shape[0]):
        match = [r for r in range(ref.shape[0]) if r not in used and np.allclose(ours[i], ref[r], rtol=1e-9, atol=1e-12)]
        assert match, i
        used.add(match[0])


def test_numpy_restatement_of_program_reproduces_reference_support():
    from oracle import oracle
    fx = common.load("codon_small_marginal")
    L = int(fx["L"])
    hip = _hip()
    plan = hip.plan_marginal(fx["flat_parents"], L)
    P = oracle.expm(common.fixture_Q(fx), True)
    sup = numpy_marginal(plan, P, fx["flat_parents"], L, fx["leaf_codes"], fx["ambig"], fx["root_freqs"])
    I, S = sup.shape[:2]
    ref = fx["support"].reshape(I, S, 61)
    assert np.allclose(sup.sum(2), 1.0, rtol=0, atol=1e-12)
    ours = sup.copy()
    ours[:, :, 60] = 1.0 - sup[:, :, :60].sum(2)
    _match_rows(ours, ref)
