"""Host-only checks of tests/catmix_cases.py: the enclosure of every case and step is narrower than the suite's bar, the mixed
reference is the host's mix of the per-class references, and the binding's packing helper and export list know the new entry points."""
import os
import re

import numpy as np
import pytest

from tests import catmix_cases as cm
from tests import mixture_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hyphy_hip_evaluate_categories_mixture", "hyphy_hip_evaluate_categories_mixture_built")


def test_case_list():
    by = cm.cases_by_name()
    assert sorted(by) == sorted([f"cm_ladder_D{D}_C3" for D in (4, 20, 33, 61, 64)] +
                                ["cm_classes_D61_C2", "cm_deep_D61_40_C3", "cm_rep_D61_C2", "cm_poly12_D20_C8", "cm_built2_D20_C2",
                                 "cm_built2_D61_C2", "cm_built3_D61_C3"])
    assert sum(by["cm_ladder_D61_C3"]["counts"]) == 49 and sum(by["cm_classes_D61_C2"]["counts"]) == 49
    # the coefficients of a full batched pass, C x rows x K, on both sides of the inline limit, and on it
    coef = {n: by[n]["C"] * sum(by[n]["counts"]) * by[n]["K"] for n in cm.names(lambda c: c["K"])}
    assert coef == {"cm_built2_D20_C2": 116, "cm_built2_D61_C2": mc.INLINE_LIMIT, "cm_built3_D61_C3": 414}, coef
    # the batched launch of the two-class case runs another kernel than a one-class call on the same components
    cs = by["cm_classes_D61_C2"]
    assert mc.kernel_for(cs, 98) == "expm64_kernel<2>" and mc.kernel_for(cs, 49) == "expm64_kernel<4>"
    assert mc.kernel_for(by["cm_deep_D61_40_C3"], 3 * sum(by["cm_deep_D61_40_C3"]["counts"])) == "expm64_kernel<1>"
    for w in cm.CLASS_WEIGHT_CASES.values():
        assert abs(sum(w) - 1.0) < 1e-15
    assert 0.0 in cm.CLASS_WEIGHT_CASES["zero"]


@pytest.mark.parametrize("name", cm.names())
def test_enclosure_is_narrower_than_the_bar(name):
    sc = cm.scenario(name)
    C = sc.C
    for step in sc.steps():
        r = sc.ref(step)
        assert np.all(np.isfinite(r["mid"])), (name, step)
        assert np.all(r["lo"] <= r["mid"]) and np.all(r["mid"] <= r["hi"]), (name, step)
        widest = float(r["width"].max())
        print(f"{name} step {step}: widest pattern {widest:.2e}")
        assert widest < cm.WIDTH_BAR, (name, step, widest)
        if step not in ("cls1",):   # the mixed width is at most the largest per-class width
            st = sc.state[6 if step == 7 else step]
            per = max(float(mc.enclosure(sc.cs, st[c])["width"].max()) for c in range(C)) if step in (1, 6) else None
            if per is not None:
                assert widest <= per * (1 + 1e-6) + 1e-15, (name, step, widest, per)
    # every class of every branch shares its component count, and the states of a step differ between the classes
    for step in (1, 3, 4, 5, 9):
        for b in range(len(sc.nodes)):
            assert len({len(sc.state[step][c][b].w) for c in range(C)}) == 1
    assert any(sc.state[1][0][b].names != sc.state[1][1][b].names for b in range(len(sc.nodes)))
    assert len(sc.state[3][0][sc.leaf].w) == 16 and len(sc.state[4][0][sc.leaf].w) == 1 and len(sc.state[5][0][sc.inner].w) == 5
    assert sc.state[6][0][sc.nxt] is sc.state[5][0][sc.nxt] and sc.state[6][1][sc.nxt].names == sc.single.names


@pytest.mark.parametrize("name", ["cm_classes_D61_C2", "cm_built2_D20_C2"])
def test_two_class_reference_is_the_host_mix_of_the_per_class_references(name):
    sc = cm.scenario(name)
    for step, w in ((1, sc.w), (6, sc.w), (7, sc.w_new)):
        st = sc.state[6 if step == 7 else step]
        per = np.stack([mc.enclosure(sc.cs, st[c])["mid"] for c in range(2)])
        host = np.logaddexp(np.log(w[0]) + per[0], np.log(w[1]) + per[1])
        got = sc.ref(step)["mid"]
        print(f"{name} step {step}: largest |reference - host mix| = {float(np.abs(got - host).max()):.2e}")
        assert np.all(np.abs(got - host) <= 1e-13), (name, step, float(np.abs(got - host).max()))


def test_class_weight_cases_stay_inside_the_bar():
    for name in ("cm_ladder_D61_C3", "cm_ladder_D20_C3"):
        sc = cm.scenario(name)
        for tag, w in cm.CLASS_WEIGHT_CASES.items():
            r = cm.enclosure(sc.cs, sc.state[1], np.array(w))
            assert np.all(np.isfinite(r["mid"])) and float(r["width"].max()) < cm.WIDTH_BAR, (name, tag)


def test_pack_class_mixture_shapes_and_refusals():
    from hyphy_amd import hip
    rng = np.random.default_rng(3)
    counts = [1, 3, 2]
    q = [[rng.random((m, 5, 5)) for m in counts] for _ in range(2)]
    w = [[rng.random(m) for m in counts] for _ in range(2)]
    pq, pw, cnt = hip.pack_class_mixture(3, q, w, 2)
    assert pq.shape == (12, 5, 5) and pw.shape == (12,) and cnt.tolist() == counts
    assert pq.flags.c_contiguous and pw.flags.c_contiguous and cnt.dtype == np.int64
    off = np.r_[0, np.cumsum(counts)]
    for c in range(2):          # class-major, inside a class branch-major: component (c, k, m) at c n_tot + off[k] + m
        for k in range(3):
            for m in range(counts[k]):
                assert np.array_equal(pq[c * 6 + off[k] + m], q[c][k][m]) and pw[c * 6 + off[k] + m] == w[c][k][m]
    rows = [[rng.random((m, 2)) for m in counts] for _ in range(2)]
    pc, _, _ = hip.pack_class_mixture(3, rows, w, 1)
    assert pc.shape == (12, 2)
    same = hip.pack_class_mixture(2, [rng.random((2, 4, 5, 5))] * 3, [rng.random((2, 4))] * 3, 2)     # the same M on every branch
    assert same[0].shape == (24, 5, 5) and same[2].tolist() == [4, 4]
    one = hip.pack_class_mixture(3, q[:1], w[:1], 2)                                                   # C == 1: pack_mixture
    ref = hip.pack_mixture(3, q[0], w[0], 2)
    assert all(np.array_equal(a, b) for a, b in zip(one, ref))
    with pytest.raises(ValueError, match="other component counts"):
        hip.pack_class_mixture(3, [q[0], q[1][:2] + [rng.random((1, 5, 5))]], [w[0], w[1][:2] + [rng.random(1)]], 2)
    with pytest.raises(ValueError, match="classes"):
        hip.pack_class_mixture(3, q, w[:1], 2)
    with pytest.raises(ValueError, match="classes"):
        hip.pack_class_mixture(3, [], [], 2)
    with pytest.raises(ValueError, match="another shape"):
        hip.pack_class_mixture(3, [q[0], [rng.random((m, 4, 4)) for m in counts]], w, 2)


def test_new_names_are_exported_and_declared():
    from hyphy_amd import hip
    txt = open(os.path.join(ROOT, "include", "hyphy_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(hyphy_hip_[a-z_]+)\s*\(", txt))
    for n in NEW:
        assert n in hip.EXPORTS and n in declared, n
    assert hasattr(hip.HipPartition, "evaluate_categories_mixture") and hasattr(hip.HipPartition, "evaluate_categories_mixture_built")
