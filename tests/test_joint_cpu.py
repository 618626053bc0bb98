"""CPU-only checks of the joint ancestral reconstruction: the C-ABI names, the NULL-partition error, and tests/joint_ref.py — the
reference the GPU tests hold hyphy_hip_joint_ancestral to — against brute-force enumeration, the tie rule, the wide star and the states of the reference binary (tests/golden/joint_*.npz)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests import joint_ref as jr
from tests import scalefree as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_names():
    import __graft_entry__ as g
    g.build()
    from hyphy_amd import hip
    assert "hyphy_hip_joint_ancestral" in open(os.path.join(ROOT, "include", "hyphy_hip.h")).read()
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "hyphy_hip_joint_ancestral")
    assert "hyphy_hip_joint_ancestral" in hip.EXPORTS
    assert hasattr(hip.HipPartition, "joint_ancestral")


def test_null_partition_is_an_error():
    from hyphy_amd import hip
    lib = hip.load()
    out = np.zeros(4, dtype=np.int64)
    assert lib.hyphy_hip_joint_ancestral(None, 0, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) < 0
    assert b"NULL" in lib.hyphy_hip_last_error()


# ---- brute force ------------------------------------------------------------------------------------------------------------------

def _random_P(rng, B, D):
    M = rng.random((B, D, D)) + 0.02
    return M / M.sum(axis=2, keepdims=True)


def _brute(D, fp, L, codes, amb, P, pi):
    """The largest probability over every assignment of the internal nodes that have a resolved or partially ambiguous leaf below
    them and every resolution of the partially ambiguous leaves; subtrees with nothing but fully unresolved leaves count 1."""
    I = len(fp) - L
    ch = sf.children_of(fp, L)

    def unresolved_leaf(l):
        return codes[l] < 0 and np.all(amb[-codes[l] - 1] == 1.0)
    informative = [False] * I
    for n in range(I):
        informative[n] = any((c < L and not unresolved_leaf(c)) or (c >= L and informative[c - L]) for c in ch[n])
    if not informative[I - 1]:
        return 1.0
    nodes = [n for n in range(I) if informative[n]]
    best = 0.0
    for assign in itertools.product(range(D), repeat=len(nodes)):
        st = dict(zip(nodes, assign))
        pr = pi[st[I - 1]]
        for n in nodes:
            if n != I - 1:
                pr *= P[L + n][st[fp[L + n]], st[n]]
        for l in range(L):
            if unresolved_leaf(l):
                continue
            row = P[l][st[fp[l]]]
            pr *= row[codes[l]] if codes[l] >= 0 else (row * amb[-codes[l] - 1]).max()
        best = max(best, pr)
    return best


BRUTE = [
    ("D4_I3_binary", 4, np.array([0, 0, 1, 1, 2, 2, -1]), 4),
    ("D4_I4_binary", 4, np.array([0, 0, 1, 1, 2, 3, 2, 3, -1]), 5),        # ((a,b),(c,d)) and e under the root's other child
    ("D4_I3_trifurcation", 4, np.array([0, 0, 0, 1, 1, 2, 2, -1]), 5),     # (a,b,c), (d,e), root
    ("D20_I2", 20, np.array([0, 0, 1, 1, -1]), 3),
]


@pytest.mark.parametrize("name,D,fp,L", BRUTE, ids=[b[0] for b in BRUTE])
def test_brute_force(name, D, fp, L):
    rng = np.random.default_rng(len(name) * 101 + D)
    I = len(fp) - L
    P = _random_P(rng, len(fp) - 1, D)
    pi = rng.random(D) + 0.1
    pi /= pi.sum()
    amb = (rng.random((3, D)) < 0.5).astype(np.float64)
    amb[:, 0] = 1.0
    amb[1, 1] = 0.0
    amb[0, :] = 1.0                                       # code -1: fully unresolved
    S = 12
    codes = rng.integers(0, D, size=(L, S))
    codes[0, 1] = -2                                      # partially ambiguous
    codes[1, 2], codes[L - 1, 2] = -3, -2
    codes[0, 3] = codes[1, 3] = -1                        # a cherry (or part of a polytomy) unresolved
    if name == "D4_I3_trifurcation":
        codes[2, 3] = -1                                  # ... the whole trifurcation: an internal node at -1
    codes[:, 4] = -1                                      # everything unresolved
    codes[L - 1, 5] = -1
    states, margins = jr.joint_ref(D, fp, L, codes, amb, P, pi)
    assert states.shape == (I + L, S)
    assert np.all(states[:, 4] == -1)
    if name != "D20_I2":
        assert states[0, 3] == -1 and states[I - 1, 3] >= 0   # internal node 0 sits above unresolved leaves only
    for s in range(S):
        m, e = jr.joint_probability(states[:, s], D, fp, L, codes[:, s], amb, P, pi)
        got = float(np.ldexp(m, e))
        want = _brute(D, fp, L, codes[:, s], amb, P, pi)
        assert abs(got - want) <= 1e-13 * want, (name, s, got, want)
        resolved = codes[:, s] >= 0
        assert np.array_equal(states[I:, s][resolved] >= 0, np.full(int(resolved.sum()), states[I - 1, s] >= 0))
        assert np.array_equal(states[I:, s][resolved & (states[I:, s] >= 0)], codes[:, s][resolved & (states[I:, s] >= 0)])


def test_tie_rule():
    D, fp, L, codes, amb, P, pi = jr.tie_case()
    states, margins = jr.joint_ref(D, fp, L, codes, amb, P, pi)
    # every entry is 5^a / 2^b, so the products are exact.  The root: all four states tie -> 0.  Node 1 above leaves (2, 3) under
    # root state 0: staying at 0 (5/8 x 1/64) ties with moving to 2 or 3 (1/8 x 5/64) -> 0; a last-index rule would give 3.
    assert states[:3, 0].tolist() == [0, 0, 0]
    assert margins[0] == 0.0


def test_wide_star():
    D, fp, L, codes, amb, P, pi = jr.wide_star()
    I = len(fp) - L
    states, _ = jr.joint_ref(D, fp, L, codes, amb, P, pi)
    # the enumerable optimum: the root takes the state that maximises pi[x] * prod over the leaves and the cherry
    for s in range(codes.shape[1]):
        logs = []
        for x in range(4):
            v = np.log(pi[x]) + sum(np.log(P[l][x, codes[l, s]]) for l in range(L - 2))
            cherry = max(np.log(P[L][x, y]) + np.log(P[L - 2][y, codes[L - 2, s]]) + np.log(P[L - 1][y, codes[L - 1, s]]) for y in range(4))
            logs.append(v + cherry)
        assert states[I - 1, s] == int(np.argmax(logs)), (s, logs)
        assert np.sort(logs)[-1] - np.sort(logs)[-2] > 1.0
    plain = jr.joint_plain(D, fp, L, codes, amb, P, pi)
    assert np.all(plain[:I] == 0), "96 factors of 1e-6 underflow without per-factor rescaling: every comparison fails, state 0"
    assert not np.array_equal(plain[:I], states[:I])


# ---- the reference binary's own states ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["joint_codon_small", "joint_nuc_ambig", "joint_codon_cat3"])
def test_joint_ref_reproduces_the_goldens(name):
    """tests/golden/joint_*.npz (tools/make_joint_golden.py): the states the unmodified reference binary printed for
    ReconstructAncestors (lf, DOLEAVES).  joint_ref on oracle.expm matrices reproduces every one of them, -1 included, with the
    recorded per-pattern classes, and every pattern's smallest decision margin is the recorded one and at least 1e-6."""
    from oracle import oracle
    from tests import common
    fx = common.load(name)
    values = fx["cat_values"] if "cat_values" in fx else [1.0]
    P = np.stack([oracle.expm(common.fixture_Q(fx, float(v)), str(fx["kind"]) == "codon") for v in values])
    states, margins = jr.joint_ref(fx["D"], fx["flat_parents"], fx["L"], fx["leaf_codes"], fx["ambig"], P, fx["root_freqs"],
                                   class_of_pattern=fx["pattern_class"])
    assert fx["states"].shape == states.shape == (len(fx["flat_parents"]), fx["leaf_codes"].shape[1])
    assert len(fx["node_names"]) == len(fx["flat_parents"])
    assert np.array_equal(states, fx["states"])
    assert np.array_equal(margins, fx["margins"]) and margins.min() == float(fx["min_margin"]) >= 1e-6
    if name == "joint_nuc_ambig":
        assert len(fx["ambig"]) > 1 and (fx["states"] < 0).any() and (fx["states"][:, (fx["states"] < 0).all(axis=0)]).size > 0
    if name == "joint_codon_cat3":
        assert sorted(set(fx["pattern_class"].tolist())) == [0, 1, 2]
