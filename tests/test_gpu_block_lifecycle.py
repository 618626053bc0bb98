"""Every path that allocates a shard's blocks after creation, run twice on one partition — the second time larger, so that each
buffer is dropped and allocated again through the shard's block owner (hyphy_amd/csrc/blocks.h) — against a fresh partition that
was only ever given the larger size: templates (K = 2, then 3), mixture components (2, then 3 per branch), per-site fit sets (1,
then 3; 61 states), the per-site export, the marginal pass's scratch, the deposits of a forced chain schedule, subtree repeats off
and on.  Smallest shapes that reach each path: 4 and 61 states, 8 leaves, 33 patterns (three tiles, the last partial), 2 classes.

Held: every result of the grown partition equals the fresh one's bit for bit; two partitions taken through the same sequence
report the same schedule_info(); the device memory it reports grows by at least K D D 8 bytes across set_q_templates.  No
allocation failure is provoked (tests/test_blocks_cpu.py covers those on the host)."""
import re

import numpy as np
import pytest

from tests import scalefree as sf

pytestmark = pytest.mark.gpu

TREE = sf.balanced_tree(2, 3)      # 8 leaves
S, C = 33, 2
CLASS_WEIGHTS = np.array([0.4, 0.6])


def _rates(rng, n, D, scale):
    """``n`` rate matrices: non-negative off the diagonal, rows summing to zero."""
    Q = rng.random((n, D, D)) * scale / D
    Q[:, np.arange(D), np.arange(D)] = 0.0
    Q[:, np.arange(D), np.arange(D)] = -Q.sum(axis=2)
    return Q


def _case(D):
    fp, L = TREE
    rng = np.random.default_rng(100 + D)
    B = len(fp) - 1
    # few distinct columns below each cherry (subtree repeats find classes), ambiguity codes in every tile
    base = rng.integers(0, D, size=(L // 2, 5))
    pick = rng.integers(0, 5, size=(L // 2, S))
    codes = np.repeat(np.take_along_axis(base, pick, axis=1), 2, axis=0).astype(np.int64)
    codes[rng.random((L, S)) < 0.15] = rng.integers(0, D)
    codes[1, 1::8] = -1
    codes[6, 5::16] = -2
    amb = np.ones((2, D))
    amb[1, D // 2:] = 0.0
    pi = rng.random(D) + 0.1
    pi /= pi.sum()
    cs = dict(D=D, fp=fp, L=L, B=B, codes=codes, amb=amb, pi=pi, nodes=np.arange(B, dtype=np.int64),
              Q=[_rates(rng, B, D, 0.3 * (c + 1)) for c in range(C)],
              T={K: _rates(rng, K, D, 1.0) for K in (2, 3)},
              coef={K: [rng.uniform(0.05, 0.3, size=(B, K)) for _ in range(C)] for K in (2, 3)},
              mixQ={M: _rates(rng, B * M, D, 0.4).reshape(B, M, D, D) for M in (2, 3)},
              mixw={M: rng.dirichlet(np.ones(M), size=B) for M in (2, 3)},
              bgroup=rng.integers(0, 2, size=B).astype(np.int64), bcoef=rng.uniform(0.05, 0.3, size=(B, 3)),
              smult={n: rng.uniform(0.2, 2.0, size=(n, S, 2, 3)) for n in (1, 3)})
    return cs


def _mk(cs):
    from hyphy_amd import hip
    return hip.HipPartition(cs["D"], cs["fp"], cs["L"], cs["codes"], cs["amb"], np.ones(S, dtype=np.int64), C)


def _mem(part):
    m = re.search(r"device memory, first shard: [0-9.]+ MB = (\d+) bytes", part.schedule_info())
    assert m, part.schedule_info()
    return int(m.group(1))


def _full(part, cs, per_site=False):
    """A full pass of both classes over dense rate matrices."""
    return [part.evaluate(cs["nodes"], cs["nodes"], cs["Q"][c], cs["pi"], cat=c, per_site=per_site) for c in range(C)]


def _sequence(part, cs, grow, monkeypatch):
    """The lazily allocating paths in a fixed order; ``grow``: each first at its smaller size.  Returns the results of the larger
    calls, the memory figures around the first set_q_templates, and its K."""
    out = {}
    out["first"] = _full(part, cs)
    K0 = 2 if grow else 3
    before = _mem(part)
    for K in ((2, 3) if grow else (3,)):
        part.set_q_templates(cs["T"][K])
        if K == K0:
            after = _mem(part)
        built = []
        for c in range(C):
            part.build_q(cs["coef"][K][c])
            built.append(part.evaluate_built(cs["nodes"], cs["nodes"], cs["pi"], cat=c, per_site=True))
        out["built"] = built
    for M in ((2, 3) if grow else (3,)):
        out["mixture"] = [part.evaluate_mixture(cs["nodes"], cs["nodes"], cs["mixQ"][M], cs["mixw"][M], cs["pi"], cat=c, per_site=True)
                          for c in range(C)]
    if cs["D"] == 61:
        for n in ((1, 3) if grow else (3,)):
            out["site_fits"] = part.site_fits_evaluate(cs["bgroup"], cs["bcoef"], cs["smult"][n], cs["pi"])
    out["export"] = _full(part, cs, per_site=True)
    out["marginal"] = part.marginal_ancestral("internal", weights=CLASS_WEIGHTS, support=True, map=True)
    monkeypatch.setenv("HYPHY_HIP_CHAIN_M", "2")   # (61 states: a chain schedule, which deposits edge products)
    out["chain"] = _full(part, cs, per_site=True)
    monkeypatch.delenv("HYPHY_HIP_CHAIN_M")
    part.set_repeats(False)
    out["repeats_off"] = _full(part, cs, per_site=True)
    part.set_repeats(True)
    out["repeats_on"] = _full(part, cs, per_site=True)
    out["marginal_again"] = part.marginal_ancestral("leaves", weights=CLASS_WEIGHTS, support=True, map=True)
    return out, (before, after, K0), part.schedule_info()


def _flat(x):
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _flat(y)]
    return [np.asarray(x)]


@pytest.mark.parametrize("D", [4, 61])
def test_grown_buffers_give_the_results_of_a_fresh_partition(D, monkeypatch):
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")     # (class-compressed whatever the size)
    monkeypatch.setenv("HYPHY_HIP_NUCGEN", "0")      # (4 states: the run-time generated kernel would arrive after a number of evaluations)
    if D != 4:
        monkeypatch.setenv("HYPHY_HIP_KERNEL", "1")
    cs = _case(D)
    with _mk(cs) as grown, _mk(cs) as twin, _mk(cs) as fresh:
        assert grown.repeat_stats()["available"] == 1     # (set_repeats below switches between two real forms)
        got, (before, after, K0), info = _sequence(grown, cs, True, monkeypatch)
        got2, _, info2 = _sequence(twin, cs, True, monkeypatch)
        want, (fbefore, fafter, fK0), _ = _sequence(fresh, cs, False, monkeypatch)
    print(f"D={D}: device memory {before} -> {after} bytes across set_q_templates(K={K0}); fresh partition {fbefore} -> {fafter} (K={fK0}); {info}")
    assert sorted(got) == sorted(want)
    for key in want:
        a, b = _flat(got[key]), _flat(want[key])
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (D, key)
        for x, y in zip(a, _flat(got2[key])):
            assert np.array_equal(x, y, equal_nan=True), (D, key, "twin")
    for x in _flat(want["first"]) + _flat(want["built"][0][0]) + _flat(want["mixture"][0][0]):
        assert np.isfinite(x).all()
    assert info == info2
    assert after - before >= K0 * D * D * 8, (before, after)
    assert fafter - fbefore >= fK0 * D * D * 8, (fbefore, fafter)
