"""The cases of tests/marginal_cases.py are what the GPU tests take them for, and the bar they are held to is one a correct
implementation of the device's scheme passes: a float64 model of the scheme against the scale-free reference on every case, the
share of MAP entries the margin leaves out, the exponent gap of the "impossible under one class" cases and what the two forms of the
class accumulation make of them.  CPU only."""
import numpy as np
import pytest

from tests import marginal_cases as mc, scalefree as sf

NAMES = list(mc.cases())
_worst = {}


@pytest.mark.parametrize("name", NAMES)
def test_model_of_the_scheme_passes_the_bar(name):
    """Prints the largest componentwise deviation above the floor; the largest over the list is marginal_cases.MODEL_MAX_REL."""
    cs, ref = mc.cases()[name], mc.reference(name)
    for which, key in ((0, "post"), (1, "leaf_post")):
        got, _ = mc.model_support(cs, which)
        assert np.array_equal(np.isnan(got).all(axis=2), np.isnan(ref[key]).all(axis=2)), (name, key)
        _worst[name, key] = mc.hold_support(f"{name} model {key}", got, ref[key], sums_to_one=which == 0)
        fin = np.isfinite(got).all(axis=2)               # the MAP check on the model's own first argmax
        mc.hold_map(f"{name} model {key}", np.where(fin, got.argmax(axis=2), -1).astype(np.int64), np.where(fin, got.max(axis=2), np.nan), got, ref[key])
    rel = max(_worst[name, k] for k in ("post", "leaf_post"))
    print(f"{name}: model against scale-free {rel:.3e} (largest so far {max(_worst.values()):.3e})")
    assert rel <= mc.MODEL_MAX_REL, (name, rel, "marginal_cases.MODEL_MAX_REL is out of date")
    assert 100 * mc.MODEL_MAX_REL <= mc.RTOL


def test_case_list():
    names = set(NAMES)
    assert {f"states_D{D}" for D in mc.STATE_COUNTS} <= names and set(mc.SCALEFREE) <= names and set(mc.ALL_IMPOSSIBLE) <= names
    assert {"wide_D4_n40", "wide_D20_n40"} <= names
    assert {f"{n}_{t}" for n in mc.CLASSES for t in ("given", "reversed", "1em30_first", "w0")} <= names
    assert {f"one_class_impossible_D{D}_{o}" for D in (4, 61) for o in ("AB", "BA")} <= names
    for name in NAMES:
        cs = mc.cases()[name]
        assert cs["P"].min() >= 0.0 and np.allclose(cs["P"].sum(axis=-1), 1.0, rtol=0, atol=1e-14), name
    for D in mc.STATE_COUNTS:
        cs = mc.cases()[f"states_D{D}"]
        assert cs["leaf_codes"].shape[1] == 17 and {-1, -2} <= set(cs["leaf_codes"].ravel().tolist())
        assert not np.allclose(cs["root_freqs"], 1.0 / D)
    for D in (4, 20):
        cs = mc.cases()[f"wide_D{D}_n40"]
        assert max(len(k) for k in sf.children_of(cs["flat_parents"], int(cs["L"]))) >= 40
        _, ex = mc.model_support(cs, 1)
        assert ex.max() >= 3, ex.max()                   # several steps of 2^64 along the prefix and suffix products
    for name in mc.ALL_IMPOSSIBLE:
        site = mc.reference(name)["site_logl"]
        assert np.isneginf(site).any() and np.isfinite(site).any()
    for name in mc.group("classes"):                     # the classes' exponents do differ where they are mixed
        _, ex = mc.model_support(mc.cases()[name], 0)
        assert (ex.max(axis=0) - ex.min(axis=0)).max() >= 2, name


def test_map_margin_leaves_out_few():
    """The share of (row, pattern) entries whose MAP state the reference decides by less than MAP_MARGIN, with the reference alone.
    Two kinds.  Ties: the two largest supports are the same number to rounding (within TIE = 32 ulp; 19 measured).  They occur
    only where a uniform matrix makes the tree treat states alike (stars, classes_D61_k2: 1 410 entries, asserted absent anywhere
    else), no margin decides them, and hold_map holds them to "one of the tied states".  Everything else the margin leaves out
    counts against MAP_LEFT_OUT over the whole list, uniform cases included (3 of 160 787 measured: two near-ties of relative size
    2e-9 in star_D4_n8_1em9 and one of 6e-7 on a ladder)."""
    TIE = 32 * np.finfo(float).eps
    out = ties = tot = 0
    for name in NAMES:
        uniform = mc.has_uniform_matrix(mc.cases()[name])
        for key in ("post", "leaf_post"):
            ref = mc.reference(name)[key]
            decided, fin, _ = mc.map_agreement(ref)
            left = fin & ~decided
            top2 = np.sort(np.where(np.isfinite(ref), ref, -1.0), axis=2)[:, :, -2:]
            tie = left & (top2[:, :, 1] - top2[:, :, 0] <= TIE * top2[:, :, 1])
            assert uniform or not tie.any(), (name, key, np.argwhere(tie)[:4])
            out, ties, tot = out + int((left & ~tie).sum()), ties + int(tie.sum()), tot + int(fin.sum())
    print(f"MAP: the margin leaves out {out} of {tot} entries ({out / tot:.2e}) and {ties} ties")
    assert tot > 100000 and out <= mc.MAP_LEFT_OUT * tot, (out, tot)
    assert ties <= 0.01 * tot, (ties, tot)


@pytest.mark.parametrize("name", mc.group("one_class_impossible"))
def test_impossible_under_one_class(name):
    """On the special patterns class A's root exponent is at least 17 above B's: 2^(-64 x 17) is zero in float64, so the
    min-exponent rule applied to B's zero contribution wipes A's out and the support is not finite; passing the zero contribution
    over keeps it, and the bar holds on every pattern (all are possible under A)."""
    cs, ref = mc.cases()[name], mc.reference(name)
    a, sp = int(cs["class_A"]), cs["special"]
    assert np.isfinite(ref["site_logl"]).all()
    assert np.isneginf(ref["class_site_logl"][1 - a][sp]).all() and np.isfinite(ref["class_site_logl"][a]).all()
    for which, key in ((0, "post"), (1, "leaf_post")):
        fixed, ex = mc.model_support(cs, which, add="skip")
        if which == 0:
            gap = ex[a][-1, sp] - ex[1 - a][-1, sp]      # the root is the last internal row
            assert gap.min() >= 17, gap
        mc.hold_support(f"{name} {key} zero contribution passed over", fixed, ref[key], sums_to_one=which == 0)
        today, _ = mc.model_support(cs, which, add="min")
        assert not np.isfinite(today[:, sp]).all(), (name, key)
