"""The scale-free reference (tests/scalefree.py) is what it claims to be: it agrees with 50-digit arithmetic, with the reference's own
per-site values in the goldens, and with the CPU oracle on every case of the generator the GPU tests use (the condition that
keeps those cases honest: the reference's own scheme is accurate on each of them).  CPU only."""
import numpy as np
import pytest

from tests import common, scalefree as sf

CASES = sf.rescale_edge_cases()
NAMES = [c["name"] for c in CASES]


def _mp_site_logl(mp, cs, P, pinned=None):
    """Per-pattern log-likelihood in mpmath, no scaling of any kind (the exponent range of mpf has no practical end)."""
    D, L = int(cs["D"]), int(cs["L"])
    fp = cs["flat_parents"]
    I = len(fp) - L
    ch = sf.children_of(fp, L)
    S = cs["leaf_codes"].shape[1]
    Pm = [[[mp.mpf(float(x)) for x in row] for row in M] for M in P]
    out = []
    for s in range(S):
        cond = [None] * I
        for n in range(I):
            v = [mp.mpf(1)] * D
            if pinned is not None and pinned[0] == L + n:
                v = [mp.mpf(1) if x == pinned[1][s] else mp.mpf(0) for x in range(D)]
            for c in ch[n]:
                if c >= L:
                    w = cond[c - L]
                else:
                    k = int(cs["leaf_codes"][c, s])
                    if pinned is not None and pinned[0] == c:
                        k = int(pinned[1][s])
                    w = [mp.mpf(1) if x == k else mp.mpf(0) for x in range(D)] if k >= 0 else [mp.mpf(float(x)) for x in cs["ambig"][-k - 1]]
                v = [v[i] * mp.fsum(Pm[c][i][j] * w[j] for j in range(D)) for i in range(D)]
            cond[n] = v
        lik = mp.fsum(cond[I - 1][i] * mp.mpf(float(cs["root_freqs"][i])) for i in range(D))
        out.append(float(mp.log(lik)) if lik > 0 else -np.inf)
    return np.array(out)


def _small_cases():
    """Small trees (at most 12 taxa) at D = 4 and 5: near-identity matrices down to 1e-30, an unreachable state, ambiguity codes."""
    out = []
    for seed, (D, k, d, eps) in enumerate(((4, 3, 2, 1e-30), (5, 2, 3, 1e-30), (4, 2, 3, 1e-10), (5, 3, 2, 1e-3), (4, 12, 1, 1e-6))):
        rng = np.random.default_rng(70 + seed)
        fp, L = sf.balanced_tree(k, d)
        S = 10
        codes = sf._patterns(rng, L, D, S, k)
        P = sf._block_zero(sf.near_identity(rng, len(fp) - 1, D, eps), D)
        codes[:, 5] = (np.arange(L)) % (D - 1)
        codes[0, 5] = D - 1                                    # impossible
        pi = rng.random(D) + 0.1
        out.append(sf._case(f"small_D{D}_k{k}_d{d}_{eps:g}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum()))
    return out


@pytest.mark.parametrize("cs", _small_cases(), ids=lambda c: c["name"])
def test_agrees_with_fifty_digit_arithmetic(cs):
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    want = _mp_site_logl(mpmath.mp, cs, cs["P"])
    got = sf.case_reference(cs)["site_logl"]
    assert np.isneginf(want[5]) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0)) < 1e-13
    # pinned states: an internal node and a leaf
    L, S, D = int(cs["L"]), cs["leaf_codes"].shape[1], int(cs["D"])
    for node in (L, 1):
        pin = (node, (np.arange(S) * 3) % (D - 1))
        want = _mp_site_logl(mpmath.mp, cs, cs["P"], pinned=pin)
        got = sf.case_reference(cs, pinned=pin)["site_logl"]
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        assert np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0)) < 1e-13


def test_posteriors_and_conditionals_agree_with_brute_force():
    """Marginal posteriors against the joint enumerated over every assignment of the internal nodes (D = 4, three internal nodes), and
    the conditionals against the unnormalised recurrence."""
    rng = np.random.default_rng(5)
    fp, L = sf.balanced_tree(2, 2)
    D, S = 4, 8
    codes = sf._patterns(rng, L, D, S, 2)
    cs = sf._case("brute", D, fp, L, codes, sf.ordinary(rng, len(fp) - 1, D), rng, root_freqs=np.array([0.1, 0.2, 0.3, 0.4]))
    ref = sf.case_reference(cs, conditionals=True, posteriors=True)
    P, pi = cs["P"], cs["root_freqs"]
    leafv = lambda l, s: (np.eye(D)[codes[l, s]] if codes[l, s] >= 0 else cs["ambig"][-codes[l, s] - 1])
    for s in range(S):
        joint = np.zeros((D, D, D))                           # states of internal 0, 1, 2 (= root)
        for a in range(D):
            for b in range(D):
                for r in range(D):
                    x = pi[r] * P[L + 0][r, a] * P[L + 1][r, b]
                    x *= (P[0][a] @ leafv(0, s)) * (P[1][a] @ leafv(1, s)) * (P[2][b] @ leafv(2, s)) * (P[3][b] @ leafv(3, s))
                    joint[a, b, r] = x
        tot = joint.sum()
        assert abs(np.log(tot) - ref["site_logl"][s]) < 1e-13
        for n, ax in enumerate(((1, 2), (0, 2), (0, 1))):
            assert np.allclose(ref["post"][n, s], joint.sum(axis=ax) / tot, rtol=1e-12, atol=1e-15)
        c0 = (P[0] @ leafv(0, s)) * (P[1] @ leafv(1, s))
        assert np.allclose(ref["cond"][0, s], c0 / c0.max(), rtol=1e-13)
        assert abs(ref["log_mag"][0, s] - np.log(c0.max())) < 1e-13
        # leaves: the same enumeration with leaf l set to x in place of its data, over the pattern's own likelihood
        for l in range(L):
            want = np.zeros(D)
            for x in range(D):
                lv = [np.eye(D)[x] if m == l else leafv(m, s) for m in range(L)]
                for a in range(D):
                    for b in range(D):
                        want[x] += np.sum(pi * P[L + 0][:, a] * P[L + 1][:, b]) * (P[0][a] @ lv[0]) * (P[1][a] @ lv[1]) * (P[2][b] @ lv[2]) * (P[3][b] @ lv[3])
            assert np.allclose(ref["leaf_post"][l, s], want / tot, rtol=1e-12, atol=0)


def _spread(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("name", ["ladder_D4_300", "conflict_k4_d3_D61_1em15", "star_D20_n12_1em6", "classes_D20_k2", "mixed_D4_k4_1em20_S37"])
def test_posteriors_are_the_pinned_evaluations(name):
    """``post`` and ``leaf_post`` against the recurrence itself, not the pre-order code: the support of state x at node n is
    exp(site_logl with n pinned to x - site_logl), for a leaf (its data replaced by x) and an internal node alike; with rate
    classes both evaluations are the mixed ones.  Every state of three leaves and three internal nodes (the star has three internal
    nodes in all: the node above its leaves, the cherry and the root), possible patterns only.
    Where the identity does NOT hold, and no case here has it: a pattern impossible under one class and possible under another, in the
    row of a leaf, at a state x that the leaf's own data exclude.  The pinned evaluation sums w_c L_c(leaf = x) over every class, the
    impossible one included (its L_c(leaf = x) is not zero there); ``leaf_post`` mixes per-class ratios by likelihood share and passes
    a class of share 0 over, numerators and all, as hyphy_hip_marginal_ancestral does (include/hyphy_hip.h).  Internal rows, and leaf
    rows at the states the data allow, agree either way."""
    cs = CASES[NAMES.index(name)]
    L, D = int(cs["L"]), int(cs["D"])
    I = len(cs["flat_parents"]) - L
    with np.errstate(invalid="ignore"):
        ref = sf.case_reference(cs, posteriors=True)
    ok = np.flatnonzero(np.isfinite(ref["site_logl"]))
    assert len(ok) >= 8 and (name.startswith("mixed") or len(ok) == len(ref["site_logl"]))
    assert np.isnan(ref["post"][:, np.isneginf(ref["site_logl"])]).all() and np.isfinite(ref["post"][:, ok]).all()
    assert np.isnan(ref["leaf_post"][:, np.isneginf(ref["site_logl"])]).all() and np.isfinite(ref["leaf_post"][:, ok]).all()
    ld = np.longdouble       # (the logarithms are of size 1e3 and their difference is wanted to 1e-12: summed and subtracted in long double)
    base = sf.case_reference(cs, patterns=ok, log_dtype=ld)["site_logl"]
    assert np.allclose(base.astype(np.float64), ref["site_logl"][ok], rtol=1e-14, atol=0)
    for code, got in [(l, ref["leaf_post"][l]) for l in _spread(L)] + [(L + i, ref["post"][i]) for i in _spread(I)]:
        want = np.zeros((len(ok), D))
        for x in range(D):
            pin = (code, np.full(len(ref["site_logl"]), x))
            want[:, x] = np.exp(sf.case_reference(cs, pinned=pin, patterns=ok, log_dtype=ld)["site_logl"] - base)
        assert np.allclose(got[ok], want, rtol=1e-12, atol=0), (name, code, float(np.nanmax(np.abs(got[ok] - want) / want)))


def test_a_class_of_share_zero_does_not_poison_the_mix():
    """Two classes, a pattern impossible under the second: the mixed posteriors are the first class's, not NaN; impossible under
    both: NaN."""
    rng = np.random.default_rng(6)
    fp, L = sf.balanced_tree(2, 2)
    D = 4
    codes = np.array([[0, 3, 3], [1, 0, 3], [2, 1, 0], [0, 2, 1]], dtype=np.int64)
    P = np.stack([sf.ordinary(rng, len(fp) - 1, D), sf._block_zero(sf.ordinary(rng, len(fp) - 1, D), D)])
    cs = sf._case("share0", D, fp, L, codes, P, rng, weights=np.array([0.3, 0.7]))
    with np.errstate(invalid="ignore"):
        mix = sf.case_reference(cs, posteriors=True)
        cs["P"] = np.stack([P[1], P[1]])
        none = sf.case_reference(cs, posteriors=True)
    cs["P"] = P[0]
    one = sf.case_reference(cs, posteriors=True)
    assert np.isfinite(mix["class_site_logl"][0]).all() and np.isneginf(mix["class_site_logl"][1][1:]).all()
    for key in ("post", "leaf_post"):
        assert np.isfinite(mix[key]).all() and np.array_equal(mix[key][:, 1:], one[key][:, 1:])
        assert not np.allclose(mix[key][:, 0], one[key][:, 0])
        assert np.isnan(none[key][:, 1:]).all() and np.isfinite(none[key][:, 0]).all()


@pytest.mark.parametrize("name", ["codon_deep", "nuc_deep", "codon_ambig", "nuc_ambig"])
def test_agrees_with_the_reference_goldens(name):
    """site_logl of the goldens is the reference program's own output; the tolerance is test_oracle_golden.py's."""
    from oracle import oracle
    fx = common.load(name)
    P = oracle.expm(common.fixture_Q(fx), str(fx["kind"]) == "codon")
    got = sf.prune(fx["D"], fx["flat_parents"], fx["L"], fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], P, fx["root_freqs"])
    by_site = got["site_logl"][fx["site_to_pattern"]]
    assert by_site.shape == fx["site_logl"].shape
    assert np.max(np.abs(by_site - fx["site_logl"]) / np.abs(fx["site_logl"])) < 1e-11
    sub = np.arange(0, len(got["site_logl"]), 7)
    part = sf.prune(fx["D"], fx["flat_parents"], fx["L"], fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], P, fx["root_freqs"], patterns=sub)
    assert np.allclose(part["site_logl"], got["site_logl"][sub], rtol=1e-14, atol=0)   # (the matrix products block differently)


def _oracle_site_logl(cs, P):
    from oracle import oracle
    nodes = np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)
    op = oracle.OraclePartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"])
    op.set_P(nodes, P)
    with np.errstate(divide="ignore"):
        return op.site_log_likelihoods(nodes, cs["root_freqs"])


_worst = {}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_on_every_generated_case(name):
    """Per pattern (and per class) within 1e-12 relative, -inf exactly where the likelihood is zero.  Prints the deviation: the largest
    over the list is the figure in scalefree.py's docstring."""
    cs = CASES[NAMES.index(name)]
    ref = sf.case_reference(cs)
    if cs["P"].ndim == 4:
        got = np.stack([_oracle_site_logl(cs, cs["P"][c]) for c in range(cs["P"].shape[0])])
        want = ref["class_site_logl"]
    else:
        got, want = _oracle_site_logl(cs, cs["P"]), ref["site_logl"]
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), name
    fin = np.isfinite(want)
    rel = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
    _worst[name] = rel
    print(f"{name}: oracle against scale-free, largest relative deviation {rel:.3e} (largest so far {max(_worst.values()):.3e})")
    assert rel < 1e-12, (name, rel)
    assert rel <= sf.ORACLE_MAX_REL, (name, rel, "scalefree.ORACLE_MAX_REL is out of date")


def test_case_list_is_what_the_gpu_tests_expect():
    assert len(set(NAMES)) == len(NAMES) and not set(NAMES) & sf.REFERENCE_FAILS
    assert all(n in NAMES for n in sf.SUBSET)
    for cs in CASES:
        P = cs["P"]
        assert P.min() >= 0.0 and np.allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14), cs["name"]
    kinds = {n.split("_")[0] for n in NAMES}
    assert kinds == {"conflict", "mixed", "star", "threshold", "ladder", "classes"}
    for cs in CASES:                       # mixed tiles: every group of 16 patterns holds a zero, a conserved and an ambiguous pattern
        if not cs["name"].startswith("mixed"):
            continue
        site = sf.case_reference(cs)["site_logl"]
        S = len(site)
        for g in range(0, S - 15, 16):
            grp = slice(g, g + 16)
            assert np.isneginf(site[grp]).any() and np.isfinite(site[grp]).any()
            assert (cs["leaf_codes"][:, grp] < 0).any()
            assert (cs["leaf_codes"][:, grp] == cs["leaf_codes"][:1, grp]).all(axis=0).any()


def test_star_and_threshold_cases_do_what_their_names_say():
    """Stars: the node above the leaves needs 2 and 3 steps of 2^64 in one finalisation at some pattern.  Threshold: its sum is within
    a few ulps of 2^-64, below it in one case and at or above it in the other."""
    steps = set()
    for cs in CASES:
        if cs["name"].startswith("star"):
            n = int(cs["L"]) - 2
            v = np.ones((cs["leaf_codes"].shape[1], int(cs["D"])))
            for l in range(n):
                v = v * sf._edge(cs["P"][l], l, int(cs["L"]), cs["leaf_codes"], cs["ambig"], None, None, np.arange(v.shape[0]))
            tot = v.sum(axis=1)
            steps |= set(np.ceil((-64 - np.log2(tot[tot > 0])) / 64).astype(int).tolist())
        if cs["name"].startswith("threshold"):
            v = np.ones((cs["leaf_codes"].shape[1], int(cs["D"])))
            for l in range(6):
                v = v * cs["P"][l].T[cs["leaf_codes"][l]]
            tot = v.sum(axis=1)
            assert np.all(np.abs(tot / 2.0 ** -64 - 1.0) < 16 * np.finfo(float).eps), cs["name"]
            own = sf.threshold_node_sum(int(cs["D"]), sf.THRESHOLD_STATES, float(cs["P"][0][0, 1]))   # pattern 0, summed in order
            assert (own < 2.0 ** -64) == cs["name"].endswith("below"), (cs["name"], own)
    assert {2, 3} <= steps, steps


def test_skipping_tests_below_a_tested_parent_underflows_where_testing_everywhere_does_not():
    """The model behind the removal of the thinned rescaling tests (schedule.hip: build_schedule): the 2^64 rule in plain float64,
    applied at every node or only where the former rule kept the test (a node of at most four children whose internal children were
    all tested skipped its own).  On the 256-taxon four-way conflict tree at eps = 1e-15 testing everywhere is exact to rounding, the
    former rule returns zero likelihoods."""
    cs = CASES[NAMES.index("conflict_k4_d4_D4_1em15")]
    L = int(cs["L"])
    ch = sf.children_of(cs["flat_parents"], L)
    I = len(ch)
    tested = np.ones(I, dtype=bool)
    for n in range(I):
        kids = all(c < L or tested[c - L] for c in ch[n])
        tested[n] = n == I - 1 or not kids or len(ch[n]) > 4
    want = sf.case_reference(cs)["site_logl"]
    every = sf.model_logl(cs)
    assert np.max(np.abs(every - want) / np.abs(want)) < 1e-13
    with np.errstate(divide="ignore"):
        thin = sf.model_logl(cs, tested)
    assert np.isneginf(thin).any() and np.isfinite(want).all()
