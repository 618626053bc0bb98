"""Admission of the cases of tests/template_cases.py (conditions, not measurements: a case that fails one is changed):

(a) the project's oracle (oracle.expm + OraclePartition), played over the same sequences, lies within one half of the allowance of
    tests/hold.py of the reference at every pattern of every step, and within the recorded template_cases.ORACLE_MAX_RATIO;
(b) every mistake a step is there to catch moves the step's total by at least 1000 allowances;
(c) a hand-sized case against mpmath at 50 digits."""
import itertools

import numpy as np
import pytest

from tests import hold
from tests import template_cases as tc

NAMES = [c["name"] for c in tc.cases()]
BY = tc.cases_by_name()


def _allowance(ref):
    return hold.RTOL * np.abs(ref) + hold.ATOL


class Oracle:
    name = "oracle"

    @staticmethod
    def matrix(Q):
        from oracle import oracle
        return oracle.expm(Q, False)

    @staticmethod
    def sites(cs, P, pi, weights=None):
        from oracle import oracle
        nodes = np.arange(cs["B"], dtype=np.int64)
        per = []
        for Pc in (P if P.ndim == 4 else P[None]):
            op = oracle.OraclePartition(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"])
            op.set_P(nodes, Pc)
            per.append(op.site_log_likelihoods(nodes, pi))
        if weights is None:
            return per[0]
        z = np.stack(per) + np.log(weights)[:, None]
        top = z.max(axis=0)
        return top + np.log(np.exp(z - top).sum(axis=0))


@pytest.fixture(scope="module")
def oracle_ratios():
    from oracle import oracle
    oracle.build()
    out = {}
    for name in NAMES:
        for i, (ref, got) in enumerate(zip(tc.reference(name), tc.replay(name, backend=Oracle))):
            assert np.all(np.isfinite(ref["site_logl"])), (name, i)
            per = float(np.max(np.abs(got["site_logl"] - ref["site_logl"]) / _allowance(ref["site_logl"])))
            tot = abs(got["logl"] - ref["logl"]) / float(_allowance(ref["logl"]))
            out[(name, i)] = max(per, tot)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_within_half_the_allowance(name, oracle_ratios):
    for i in range(len(BY[name]["steps"])):
        r = oracle_ratios[(name, i)]
        assert r <= 0.5 and r <= tc.ORACLE_MAX_RATIO, (name, i, r)


def test_recorded_oracle_ratio(oracle_ratios):
    """The recorded value is not exceeded."""
    key = max(oracle_ratios, key=oracle_ratios.get)
    worst = oracle_ratios[key]
    print(f"largest oracle deviation / allowance: {worst:.4g} at {key}")
    assert worst <= tc.ORACLE_MAX_RATIO, (worst, key)


@pytest.mark.parametrize("name", NAMES)
def test_every_mistake_moves_the_total(name):
    ref = tc.reference(name)
    seen = set()
    for i, kind in itertools.product(range(len(ref)), tc.MISTAKES):
        alt = tc.replay(name, mistake=(kind, i))
        if alt is None:
            continue
        seen.add((i, kind))
        gap = abs(alt[i]["logl"] - ref[i]["logl"])
        assert gap >= 1000.0 * float(_allowance(ref[i]["logl"])), (name, i, kind, gap)
    cs = BY[name]
    for i, st in enumerate(cs["steps"]):
        live = any(r.any() for r in st["rows"].values())
        if not live:
            continue
        want = {"old_rows", "diagonal"} | ({"missing_template"} if cs["K"] >= 2 else set())
        if i and st["t"] is not None:
            want.add("old_templates")
            if len(st["rows"]) < cs["B"] and cs["kind"] != "percls":
                want.add("new_everywhere")
        assert want <= {k for j, k in seen if j == i}, (name, i, want, seen)


def test_the_list_is_what_the_device_tests_need():
    for D in tc.STATE_COUNTS:
        assert any(c["D"] == D and c["kind"] == k for c in tc.cases() for k in ("plain",)), D
        assert any(c["D"] == D and c["kind"] == "mix" for c in tc.cases())
        assert D == 4 or any(c["D"] == D and c["kind"] == "cat" for c in tc.cases())
    for D in (20, 61):
        assert {c["K"] for c in tc.cases() if c["D"] == D and c["name"].startswith("consumer")} == {1, 2, 4, 5}
    for D in tc.STATE_COUNTS[1:]:               # the site fits (5 states and up, at most four templates) meet every state count
        assert any(c["D"] == D and c["K"] <= 4 and c["name"].startswith("consumer") for c in tc.cases()), D
    lad = BY["ahead_ring_D20_K3"]
    assert lad["B"] * 3 > 400 >= lad["B"] * 2 and len(lad["live"]) == 6
    for c in tc.cases():
        for v in range(len(c["T"]) - 1):
            ratio = np.divide(c["T"][v + 1], c["T"][v], out=np.ones_like(c["T"][v]), where=c["T"][v] != 0)
            off = ~np.eye(c["D"], dtype=bool)
            moved = ratio[:, off][ratio[:, off] != 1.0]
            assert len(moved) and moved.min() >= 1.25 and moved.max() <= 3.0, (c["name"], v)
        assert (c["leaf_codes"] < 0).any()
        for st in c["steps"]:
            for r in st["rows"].values():
                m, _ = np.frexp(r[r != 0])
                assert not np.any(m == 0.5), c["name"]        # no powers of two


def test_hand_sized_case_against_mpmath():
    """3 leaves, 2 states, 2 templates, an update of the template values and a rebuild of two of the four branches in between: every
    pattern's log-likelihood by summing over the internal states with mpmath's own matrix exponential at 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    cs = BY["hand_D2_K2"]
    assert cs["D"] == 2 and cs["L"] == 3 and cs["K"] == 2
    fp, L, B = cs["flat_parents"], 3, 4
    assert list(fp) == [0, 0, 1, 1, -1]
    P = [mp.eye(2) for _ in range(B)]
    pi = [mp.mpf(float(x)) for x in cs["pis"][0]]
    for st, ref in zip(cs["steps"], tc.reference("hand_D2_K2")):
        T = cs["T"][st["t"]]
        for b, row in st["rows"].items():
            Q = mp.zeros(2)
            for i in range(2):
                off = sum(mp.mpf(float(row[k])) * mp.mpf(float(T[k][i, 1 - i])) for k in range(2))
                Q[i, 1 - i], Q[i, i] = off, -off
            P[b] = mp.expm(Q)
        for s in range(cs["leaf_codes"].shape[1]):
            def leaf(l, x):
                k = int(cs["leaf_codes"][l, s])
                if k >= 0:
                    return P[l][x, k]
                return sum(mp.mpf(float(cs["ambig"][-k - 1][y])) * P[l][x, y] for y in range(2))
            lik = mp.mpf(0)
            for r in range(2):                   # root = internal 1: (internal 0, leaf 2)
                inner = sum(P[L + 0][r, x] * leaf(0, x) * leaf(1, x) for x in range(2))
                lik += pi[r] * inner * leaf(2, r)
            want = mp.log(lik)
            assert abs(mp.mpf(float(ref["site_logl"][s])) - want) <= mp.mpf(2e-15) * abs(want) + mp.mpf(2e-16), (s, ref["site_logl"][s], want)
