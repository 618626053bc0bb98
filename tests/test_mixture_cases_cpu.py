"""Without a GPU: what makes tests/test_gpu_mixture.py meaningful.  The enclosure of tests/mixture_cases.py contains its own middle
and is narrower than 1e-9 at every pattern of every case and step (so it cannot hide more than the bar the suite already carries);
the CPU oracle, exponentiating every component and mixing on the host, lies inside it; the case list reaches what it claims; and
the binding packs ragged input as a hand-built flat array says.

Largest width hi - lo (log units) over the patterns and steps of a case, measured here:

    ladder_D4 7.6e-12   ladder_D20 5.5e-11   ladder_D33 7.7e-11   ladder_D61 1.7e-10   ladder_D64 1.2e-10   balanced_D61 1.5e-10
    poly12_D20 1.6e-10  deep_D61_40 2.1e-10  deep_D4_120 2.5e-11  classes_D61 1.6e-10  rep_D61 2.9e-10      rep_D20 4.5e-11
    built2_D4 8.3e-12   built2_D20 7.7e-11   built2_D61 2.9e-10   built3_D4 1.0e-11    built3_D20 1.1e-10   built3_D61 2.6e-10
    built2_D61_at400 2.0e-10   built2_D61_over400 2.0e-10   built3_D61_over400 1.9e-10
"""
import numpy as np
import pytest

from tests import expm_ref as er
from tests import mixture_cases as mc
from tests import scalefree as sf

NAMES = mc.names()


def _scenarios(name):
    cs = mc.cases_by_name()[name]
    return [mc.scenario(name, c) for c in range(cs["C"])]


@pytest.mark.parametrize("name", NAMES)
def test_enclosure_contains_its_middle_and_is_narrower_than_the_bar(name):
    worst = 0.0
    for sc in _scenarios(name):
        for step in sc.steps():
            r = sc.ref(step)
            assert np.all(np.isfinite(r["lo"])) and np.all(np.isfinite(r["hi"])), (name, step)
            assert np.all(r["lo"] <= r["mid"]) and np.all(r["mid"] <= r["hi"]), (name, step)
            assert r["lo_total"] <= r["mid_total"] <= r["hi_total"], (name, step)
            assert np.all(r["width"] > 0), (name, step)
            worst = max(worst, float(r["width"].max()))
            assert r["width"].max() <= mc.WIDTH_BAR, (name, step, int(np.argmax(r["width"])), float(r["width"].max()))
    print(f"{name}: largest width {worst:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_cpu_oracle_is_inside_the_enclosure(name):
    """oracle.expm of every component, mixed on the host, then OraclePartition: inside [lo, hi], each side widened by
    scalefree.ORACLE_MAX_REL x |log| for the oracle's own pruning."""
    from oracle import oracle
    cs = mc.cases_by_name()[name]
    by = er.cases_by_name()
    D = int(cs["D"])
    for sc in _scenarios(name):
        op = oracle.OraclePartition(D, cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"])
        for step in sc.steps():
            state = sc.state[6] if step == "pin" else sc.state[step]
            P = np.stack([sum(w * oracle.expm(by[n]["Q"], False) for n, w in zip(br.names, br.w)) for br in state])
            op.set_P(sc.nodes, P)
            if step == "pin":
                op.set_branch(sc.pin, sc.states)
            try:
                site = op.site_log_likelihoods(sc.nodes, cs["root_freqs"])
            finally:
                op.set_branch(None)
            r = sc.ref(step)
            t = sf.ORACLE_MAX_REL * np.abs(r["mid"])
            assert np.all(site >= r["lo"] - t) and np.all(site <= r["hi"] + t), (name, step, float(np.max(site - r["hi"])), float(np.max(r["lo"] - site)))


def test_the_list_reaches_what_it_claims():
    by = mc.cases_by_name()
    seen, zero, halves = set(), 0, 0
    for name in NAMES:
        for sc in _scenarios(name):
            for br in sc.state[1]:
                seen.add(len(br.w))
                zero += int(np.any(br.w == 0.0))
                halves += int(len(br.w) == 2 and br.names[0] == br.names[1] and br.w[0] == br.w[1] == 0.5)
            # the leaf branch goes 3 -> 16 -> 1, the inner one to 5, a plain one next to it
            assert [len(sc.state[k][sc.leaf].w) for k in (1, 3, 4)] == [3, 16, 1], name
            assert len(sc.state[5][sc.inner].w) == 5 and len(sc.state[6][sc.nxt].w) == 1, name
            assert sc.inner != sc.nxt and sc.inner >= int(by[name]["L"]) and sc.nxt >= int(by[name]["L"]), name
    assert seen >= set(mc.COUNTS), seen
    assert zero >= 1 and halves >= 2, (zero, halves)
    for name in ("ladder_D61", "ladder_D4"):
        counts = [len(br.w) for br in mc.scenario(name).state[1]]
        assert set(counts) == set(mc.COUNTS) and any(np.any(br.w == 0.0) for br in mc.scenario(name).state[1]), name
    # both sides of the kernel-argument block's limit, and the limit itself
    rows = {n: sum(by[n]["counts"]) * by[n]["K"] for n in NAMES if by[n]["K"]}
    assert rows["built2_D61_at400"] == mc.INLINE_LIMIT and rows["built2_D61_over400"] == mc.INLINE_LIMIT + 2, rows
    assert rows["built3_D61_over400"] > mc.INLINE_LIMIT and max(rows[f"built{K}_D61"] for K in (2, 3)) < mc.INLINE_LIMIT, rows
    for n in NAMES:
        if by[n]["K"] and "400" not in n:
            assert set(by[n]["counts"]) == {1, 2, 3}, n
    # the deep cases reach below one step of the rescale, with components that need no squaring
    for name in ("deep_D61_40", "deep_D4_120"):
        sc = mc.scenario(name)
        assert sc.ref(1)["mid"].min() < -sf.LOG_SCALER, name
        for k in (1, 3, 4, 5, 6):
            for br in sc.state[k]:
                assert all(er.plan(er.cases_by_name()[n]["Q"], br.kernel)[0] == 0 for n in br.names), (name, k, br.names)
    # a re-rooting path of at least three nodes on the ladders, the updated branches in its middle
    for name in NAMES:
        if name.startswith(("ladder_", "rep_", "built", "classes_")):
            sc = mc.scenario(name)
            L = int(by[name]["L"])
            assert len(sc.path) >= 3 and sc.inner - L in sc.path[1:] and sc.nxt - L in sc.path[1:], (name, sc.path)
    # on the ladders the full passes of step 7 carry more components than any call before them: the staging buffers regrow there
    for name in NAMES:
        if name.startswith(("ladder_", "rep_", "classes_")) or (by[name]["K"] and "400" not in name):
            sc = mc.scenario(name)
            tot = [sum(len(br.w) for br in sc.state[k]) for k in (1, 6)]
            assert tot[1] > max(tot[0], 2 * len(sc.state[1])), (name, tot)
    # all three exponential kernels of 49-64 states are named by some call's component total
    kernels = {br.kernel for n in NAMES for k in (1, 3, 4) for br in mc.scenario(n).state[k] if by[n]["D"] == 61}
    assert kernels == {"expm64_kernel<1>", "expm64_kernel<2>", "expm64_kernel<4>"}, kernels
    # the compressible variants repeat every pattern
    for name in ("rep_D61", "rep_D20"):
        codes = by[name]["leaf_codes"]
        assert np.array_equal(codes[:, :20], codes[:, 20:]), name


def test_built_components_are_the_named_cases_to_an_ulp():
    by = er.cases_by_name()
    for K in (2, 3):
        for D in (4, 20, 61):
            T = mc.templates(D, K)
            assert T.shape == (K, D, D) and np.all(T[:, np.arange(D), np.arange(D)] == 0)
            for n in mc._pool(D, False, K)[0]:
                Q = mc.host_built(D, K, n)
                assert np.abs(Q - by[n]["Q"]).max() <= mc.built_extra(n), (K, D, n)
                assert np.count_nonzero(mc.coefficient_row(D, K, n)) == 1


def test_ragged_packing_of_the_binding():
    """hip.pack_mixture against a flat array built by hand: counts, order and row totals; the rectangular form unchanged."""
    from hyphy_amd import hip
    D = 3
    q = [np.full((m, D, D), 10.0 * b) + np.arange(m)[:, None, None] for b, m in enumerate((2, 1, 16, 3))]
    w = [np.arange(m) + 100.0 * b for b, m in enumerate((2, 1, 16, 3))]
    flat, fw, cnt = hip.pack_mixture(4, q, w, 2)
    assert cnt.dtype == np.int64 and cnt.tolist() == [2, 1, 16, 3]
    assert flat.shape == (22, D, D) and flat.flags.c_contiguous and flat.dtype == np.float64
    want = [0., 1., 10.] + [20. + k for k in range(16)] + [30., 31., 32.]
    assert flat[:, 0, 0].tolist() == want and np.all(flat == flat[:, :1, :1])
    assert fw.tolist() == [0., 1., 100.] + [200. + k for k in range(16)] + [300., 301., 302.]
    co = [np.arange(m * 2, dtype=np.float64).reshape(m, 2) + 100 * b for b, m in enumerate((1, 3))]
    flat, fw, cnt = hip.pack_mixture(2, co, [[1.0], [0.2, 0.3, 0.5]], 1)
    assert flat.tolist() == [[0., 1.], [100., 101.], [102., 103.], [104., 105.]] and cnt.tolist() == [1, 3]
    assert fw.tolist() == [1.0, 0.2, 0.3, 0.5]
    rect = np.arange(2 * 3 * D * D, dtype=np.float64).reshape(2, 3, D, D)
    wr = np.arange(6, dtype=np.float64).reshape(2, 3)
    flat, fw, cnt = hip.pack_mixture(2, rect, wr, 2)
    assert np.shares_memory(flat, rect) and flat.tobytes() == rect.tobytes() and fw.tobytes() == wr.tobytes() and cnt.tolist() == [3, 3]
    # the same values as per-branch arrays: the same bytes
    flat2, fw2, cnt2 = hip.pack_mixture(2, [rect[0], rect[1]], [wr[0], wr[1]], 2)
    assert flat2.tobytes() == rect.tobytes() and fw2.tobytes() == wr.tobytes() and cnt2.tolist() == [3, 3]
    with pytest.raises(AssertionError):
        hip.pack_mixture(2, [rect[0], rect[1]], [wr[0], wr[1][:2]], 2)
    with pytest.raises(AssertionError):
        hip.pack_mixture(3, [rect[0], rect[1]], [wr[0], wr[1]], 2)
