"""The class-compressed form (repeats.hip) at 2-64 states through every pass: synthetic compressible partitions
(common.compressible_case) at NW = 1 .. 4 row blocks with and without padding rows, under each form of the trunk — the row-split walk
(trunk_walk_kernel, one and two chains per tile) with the kernel behind it that serves the passes the walk does not, the wave-per-tile
trunk, the two workgroup trunks — through persisting and lazy full passes, partial updates, pure re-evaluations, new root frequencies,
downloads, pinned states, the branch cache, rate classes, mixtures and the schedule tuner.

Every result is held to the CPU oracle (RTOL, per site too) and to a second partition of the same data that runs the plain form (SAME
on log-L, SITE_ABS on per-pattern log values).  The matrices change between passes: a trunk left stale changes the number."""
import functools

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

RTOL = 1e-10       # against the oracle
SAME = 1e-13       # compressed against plain
SITE_ABS = 1e-11   # per-pattern log values, compressed against plain
LOG_SCALER = 64.0 * np.log(2.0)
NONE = np.zeros(0, dtype=np.int64)


def _site(lik, sc):
    return np.log(lik) - sc * LOG_SCALER


def _mk(fx, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(fx["D"]), fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], C)


class _Oracle:
    """The CPU oracle in both of its modes: log-L (compute_block) and per pattern (site_block) — one partition each, since the per-site
    mode keeps cumulative site corrections of its own."""

    def __init__(self, fx, C=1):
        from oracle import oracle
        args = (int(fx["D"]), fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], C)
        self.blk, self.per_site = oracle.OraclePartition(*args), oracle.OraclePartition(*args)

    def set_P(self, nodes, Q, cat=0):
        from oracle import oracle
        P = oracle.expm(Q, False)
        self.blk.set_P(nodes, P, cat)
        self.per_site.set_P(nodes, P, cat)

    def set_branch(self, node=None, states=None):   # (the oracle's pin is global state: one call serves both partitions)
        self.blk.set_branch(node, states)

    def compute_block(self, nodes, pi, cat=0):
        return self.blk.compute_block(nodes, pi, cat)

    def site_block(self, nodes, pi, cat=0):
        return self.per_site.site_block(nodes, pi, cat)


def _ref(op, nodes, pi):
    """(log-L, per-pattern log values) of the oracle, every node recomputed."""
    return op.compute_block(nodes, pi), _site(*op.site_block(nodes, pi))


def _dirty(fx, rng):
    """A dirty list with a leaf branch and an internal branch (and sometimes one more of either)."""
    L, B = int(fx["L"]), len(fx["flat_parents"]) - 1
    ch = {int(rng.integers(L)), int(rng.integers(L, B))}
    if rng.random() < 0.5:
        ch.add(int(rng.integers(B)))
    return np.array(sorted(ch), dtype=np.int64)


def _sequence(fx, seed):
    """The pass sequence of test_pass_sequence: (what, update nodes, matrix nodes, matrices, root frequencies)."""
    D, B = int(fx["D"]), len(fx["flat_parents"]) - 1
    rng = np.random.default_rng(seed)
    nodes = np.arange(B, dtype=np.int64)
    pi = fx["root_freqs"]
    Q = fx["Q"].copy()
    steps = [("full 1 (persists)", nodes, nodes, Q.copy(), pi)]
    for k in (2, 3):
        Q = common.random_rates(rng, B, D)
        steps.append((f"full {k}" + (" (lazy)" if k == 3 else ""), nodes, nodes, Q.copy(), pi))
    for k in range(6):
        ch = _dirty(fx, rng)
        Q[ch] = common.random_rates(rng, len(ch), D)
        steps.append((f"partial {k + 1} {ch.tolist()}", ch, ch, Q[ch].copy(), pi))
    steps.append(("again", NONE, NONE, None, pi))
    pi2 = rng.random(D) + 0.05
    pi2 /= pi2.sum()
    steps.append(("root frequencies", NONE, NONE, None, pi2))
    for k in (4, 5):
        Q = common.random_rates(rng, B, D)
        steps.append((f"full {k}" + (" (lazy)" if k == 5 else ""), nodes, nodes, Q.copy(), pi2))
    return steps


def _case(D):
    return common.compressible_case(D, 1000 + D)


@functools.lru_cache(maxsize=None)
def _oracle_sequence(D):
    """The oracle's results of _sequence at D (the same for every trunk form and threshold)."""
    fx = _case(D)
    op = _Oracle(fx)
    nodes = np.arange(len(fx["flat_parents"]) - 1, dtype=np.int64)
    out = []
    for _, _, qn, Q, pi in _sequence(fx, D):
        if len(qn):
            op.set_P(qn, Q)
        out.append(_ref(op, nodes, pi))
    return out


def _check(what, got, plain, ref, info=""):
    """got / plain: (log-L, likelihoods, exponents) of the compressed and the plain partition; ref: the oracle's (log-L, log values)."""
    ll, site = got[0], _site(got[1], got[2])
    assert abs(ll - ref[0]) <= RTOL * abs(ref[0]), (what, ll, ref[0], info)
    assert np.max(np.abs(site - ref[1]) / np.abs(ref[1])) < RTOL, (what, info)
    assert abs(ll - plain[0]) <= SAME * abs(plain[0]), (what, ll, plain[0], info)
    assert np.max(np.abs(site - _site(plain[1], plain[2]))) < SITE_ABS, (what, info)


def _forms(D):
    """The trunk forms that exist at NW = ceil(D / 16): (label, environment, kernel expected on lazy full passes)."""
    nw = (D + 15) // 16
    forms = [("wave", dict(HYPHY_HIP_TRUNK_WALK="0"), "prune_wave_kernel")]
    if nw >= 2:
        forms += [(f"walk/{c}", dict(HYPHY_HIP_TRUNK_WALK="1", HYPHY_HIP_WALK_CHAINS=str(c)), "trunk_walk_kernel") for c in (1, 2)]
    if nw == 4:
        forms += [(f"wg/{k}", dict(HYPHY_HIP_TRUNK_WALK="0", HYPHY_HIP_TRUNK_KERNEL=str(k)), "prune_mfma_kernel") for k in (0, 2)]
    return forms


_CASES = [(D, theta, label) for D in common.REPEAT_STATE_COUNTS for theta in ("0.05", "0.3", "0.9") for label, _, _ in _forms(D)]


@pytest.mark.parametrize("D,theta,form", _CASES)
def test_pass_sequence_under_each_trunk_form(D, theta, form, monkeypatch):
    """Three full passes (the first persists, the others are lazy: the walk where it is in force), six partial updates whose dirty lists
    hold a leaf and an internal branch (under the walk: the kernel behind it, after the copies are restored), a pure re-evaluation, new
    root frequencies only, two last full passes — with new matrices wherever the step takes any.  The kernel of the lazy passes is the
    form's own: a case cannot fall back to another form unnoticed."""
    env, kernel = {lab: (e, k) for lab, e, k in _forms(D)}[form]
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_REP_THETA", theta)
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fx = _case(D)
    refs = _oracle_sequence(D)
    with _mk(fx) as part, _mk(fx) as plain:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        plain.set_repeats(False)
        for i, (what, un, qn, Q, pi) in enumerate(_sequence(fx, D)):
            got = part.evaluate(un, qn, Q, pi, per_site=True)
            _check(what, got, plain.evaluate(un, qn, Q, pi, per_site=True), refs[i], part.schedule_info())
            if what.endswith("(lazy)"):
                assert part.prune_kernel_name() == kernel, (what, part.prune_kernel_name(), part.schedule_info())
        assert part.repeat_stats()["in_use"] == 1


def _full_and_partial(part, plain, op, fx, Q, rng, what):
    """After a plain-only entry point: two full passes (the second lazy) and a partial update, compressed against plain and oracle."""
    D, B = int(fx["D"]), len(Q)
    nodes = np.arange(B, dtype=np.int64)
    pi = fx["root_freqs"]
    for k in range(2):
        Q[:] = common.random_rates(rng, B, D)
        op.set_P(nodes, Q)
        _check(f"{what}: full {k}", part.evaluate(nodes, nodes, Q, pi, per_site=True), plain.evaluate(nodes, nodes, Q, pi, per_site=True),
               _ref(op, nodes, pi), part.schedule_info())
    assert part.prune_kernel_name() == "trunk_walk_kernel", (what, part.prune_kernel_name(), part.schedule_info())
    ch = _dirty(fx, rng)
    Q[ch] = common.random_rates(rng, len(ch), D)
    op.set_P(ch, Q[ch])
    _check(f"{what}: partial {ch.tolist()}", part.evaluate(ch, ch, Q[ch], pi, per_site=True), plain.evaluate(ch, ch, Q[ch], pi, per_site=True),
           _ref(op, nodes, pi), part.schedule_info())


@pytest.mark.parametrize("D", [17, 20, 33, 48, 61])
def test_plain_only_entry_points_with_the_walk_in_force(D, monkeypatch):
    """Downloads of the conditionals, pinned states at a leaf and at an internal node, the branch cache and a partial update of its
    branch run on the partition's own tree while the walk serves the compressed form's lazy passes; after each, full passes and a
    partial update back on the compressed form."""
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_REP_THETA", "0.3")
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_TRUNK_WALK", "1")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    fx = common.compressible_case(D, 2000 + D)
    L, S = int(fx["L"]), fx["leaf_codes"].shape[1]
    Q = fx["Q"].copy()
    B = len(Q)
    nodes = np.arange(B, dtype=np.int64)
    pi = fx["root_freqs"]
    rng = np.random.default_rng(D)
    op = _Oracle(fx)
    with _mk(fx) as part, _mk(fx) as plain:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        plain.set_repeats(False)
        op.set_P(nodes, Q)
        _check("first", part.evaluate(nodes, nodes, Q, pi, per_site=True), plain.evaluate(nodes, nodes, Q, pi, per_site=True), _ref(op, nodes, pi))
        _full_and_partial(part, plain, op, fx, Q, rng, "start")
        # conditionals of every node, reference layout
        c1, n1 = part.download_partials()
        c0, n0 = plain.download_partials()
        assert np.array_equal(n1, n0)
        assert np.allclose(c1, c0, rtol=1e-12, atol=0)
        _full_and_partial(part, plain, op, fx, Q, rng, "after the download")
        # pinned states at an internal node and at a leaf
        for node in (L + 1, 1):
            states = rng.integers(0, D, size=S).astype(np.int64)
            part.set_pinned_states(node, states)
            plain.set_pinned_states(node, states)
            op.set_branch(node, states)
            try:
                a = part.evaluate(nodes, NONE, None, pi)
                b = plain.evaluate(nodes, NONE, None, pi)
                want = op.compute_block(nodes, pi)
            finally:
                op.set_branch(None)
                part.set_pinned_states(None)
                plain.set_pinned_states(None)
            assert abs(a - want) <= RTOL * abs(want), (node, a, want)
            assert abs(a - b) <= SAME * abs(b), (node, a, b)
            _full_and_partial(part, plain, op, fx, Q, rng, f"after the pin at {node}")
        # branch cache: one branch varies, then an ordinary partial update of the same branch
        node = L + 2
        part.branch_cache_build(node)
        Q[node] = Q[node] * 1.3
        a = part.branch_cache_evaluate(node, Q[node])
        op.set_P([node], Q[node:node + 1])
        want = op.compute_block(nodes, pi)
        assert abs(a - want) <= RTOL * abs(want), (a, want)
        ch = np.array([node], dtype=np.int64)
        _check("partial of the cached branch", part.evaluate(ch, ch, Q[ch], pi, per_site=True), plain.evaluate(nodes, nodes, Q, pi, per_site=True),
               _ref(op, nodes, pi))
        _full_and_partial(part, plain, op, fx, Q, rng, "after the branch cache")
        assert part.repeat_stats()["in_use"] == 1


@pytest.mark.parametrize("D", [20, 48])
def test_rate_classes_and_mixtures_with_the_walk_in_force(D, monkeypatch):
    """Three rate classes in one launch (against the oracle per class, mixed by oracle.mix_categories) and a three-component mixture
    (against the plain form), full passes with new matrices and a partial update, the walk forced."""
    from oracle import oracle
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_REP_THETA", "0.3")
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_TRUNK_WALK", "1")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    fx = common.compressible_case(D, 3000 + D)
    B = len(fx["Q"])
    nodes = np.arange(B, dtype=np.int64)
    pi = fx["root_freqs"]
    rng = np.random.default_rng(D)
    w = np.array([0.5, 0.3, 0.2])
    scale = np.array([0.4, 1.0, 2.2])
    op = _Oracle(fx, C=3)
    with _mk(fx, C=3) as part, _mk(fx, C=3) as plain:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        plain.set_repeats(False)
        R = fx["Q"].copy()
        names = []
        for step in range(4):
            if step < 3:
                R = common.random_rates(rng, B, D)
                un = qn = nodes
            else:
                un = qn = _dirty(fx, rng)
                R[qn] = common.random_rates(rng, len(qn), D)
            Qc = np.stack([R[qn] * s for s in scale])
            for c in range(3):
                op.set_P(qn, Qc[c], cat=c)
            ll, lik, sc = part.evaluate_categories(un, qn, Qc, w, pi, per_site=True)
            ll0, lik0, sc0 = plain.evaluate_categories(un, qn, Qc, w, pi, per_site=True)
            names.append(part.prune_kernel_name())
            blocks = [op.site_block(nodes, pi, cat=c) for c in range(3)]
            want, mixed, msc = oracle.mix_categories(w, np.stack([b[0] for b in blocks]), np.stack([b[1] for b in blocks]), fx["pattern_freq"])
            assert abs(ll - want) <= RTOL * abs(want), (step, ll, want, part.schedule_info())
            assert np.max(np.abs(_site(lik, sc) - _site(mixed, msc)) / np.abs(_site(mixed, msc))) < RTOL, step
            assert abs(ll - ll0) <= SAME * abs(ll0), (step, ll, ll0)
            assert np.max(np.abs(_site(lik, sc) - _site(lik0, sc0))) < SITE_ABS, step
        assert names[2] == "trunk_walk_kernel", (names, part.schedule_info())
    W = np.tile(w, (B, 1))
    with _mk(fx) as part, _mk(fx) as plain:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        plain.set_repeats(False)
        R = np.zeros((B, 3, D, D))
        for step in range(4):
            if step < 3:
                un = qn = nodes
            else:
                un = qn = _dirty(fx, rng)
            for m in range(3):
                R[qn, m] = common.random_rates(rng, len(qn), D)
            a, la, sa = part.evaluate_mixture(un, qn, R[qn], W[qn], pi, per_site=True)
            b, lb, sb = plain.evaluate_mixture(un, qn, R[qn], W[qn], pi, per_site=True)
            assert abs(a - b) <= SAME * abs(b), (step, a, b, part.schedule_info())
            assert np.max(np.abs(_site(la, sa) - _site(lb, sb))) < SITE_ABS, step


@pytest.mark.parametrize("D", [20, 33, 48])
def test_schedule_tuner_on_a_compressed_partition(D, monkeypatch):
    """The tuner decides the trunk's form (the walk among its candidates at NW >= 2) on the lazy passes; whatever it picks, full passes,
    partial updates, a download and a pinned evaluation stay the oracle's.  (Trees of their own: the tuner's per-process cache.)"""
    for k in ("HYPHY_HIP_TUNE", "HYPHY_HIP_TRUNK_WALK", "HYPHY_HIP_TRUNK_KERNEL", "HYPHY_HIP_WALK_CHAINS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_REP_THETA", "0.3")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    fx = common.compressible_case(D, 5000 + D)
    L, S = int(fx["L"]), fx["leaf_codes"].shape[1]
    B = len(fx["Q"])
    nodes = np.arange(B, dtype=np.int64)
    pi = fx["root_freqs"]
    rng = np.random.default_rng(D)
    op = _Oracle(fx)
    with _mk(fx) as part, _mk(fx) as plain:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        plain.set_repeats(False)
        Q = fx["Q"].copy()
        for k in range(4):
            if k:
                Q = common.random_rates(rng, B, D)
            op.set_P(nodes, Q)
            _check(f"full {k}", part.evaluate(nodes, nodes, Q, pi, per_site=True), plain.evaluate(nodes, nodes, Q, pi, per_site=True),
                   _ref(op, nodes, pi), part.schedule_info())
        for k in range(4):
            ch = _dirty(fx, rng)
            Q[ch] = common.random_rates(rng, len(ch), D)
            op.set_P(ch, Q[ch])
            _check(f"partial {k}", part.evaluate(ch, ch, Q[ch], pi, per_site=True), plain.evaluate(ch, ch, Q[ch], pi, per_site=True),
                   _ref(op, nodes, pi), part.schedule_info())
        c1, n1 = part.download_partials()
        c0, n0 = plain.download_partials()
        assert np.array_equal(n1, n0), part.schedule_info()
        assert np.allclose(c1, c0, rtol=1e-12, atol=0), part.schedule_info()
        states = rng.integers(0, D, size=S).astype(np.int64)
        part.set_pinned_states(L + 1, states)
        op.set_branch(L + 1, states)
        try:
            a = part.evaluate(nodes, NONE, None, pi)
            want = op.compute_block(nodes, pi)
        finally:
            op.set_branch(None)
            part.set_pinned_states(None)
        assert abs(a - want) <= RTOL * abs(want), (a, want, part.schedule_info())
        for k in range(2):
            Q = common.random_rates(rng, B, D)
            op.set_P(nodes, Q)
            _check(f"full after {k}", part.evaluate(nodes, nodes, Q, pi, per_site=True), plain.evaluate(nodes, nodes, Q, pi, per_site=True),
                   _ref(op, nodes, pi), part.schedule_info())
        ch = _dirty(fx, rng)
        Q[ch] = common.random_rates(rng, len(ch), D)
        op.set_P(ch, Q[ch])
        _check("last partial", part.evaluate(ch, ch, Q[ch], pi, per_site=True), plain.evaluate(ch, ch, Q[ch], pi, per_site=True),
               _ref(op, nodes, pi), part.schedule_info())
        assert part.repeat_stats()["in_use"] == 1, part.schedule_info()
