"""tests/grad_cases.py pinned: the reference gradient against deriv_cases' d1, against central differences of the longdouble log L and
against the forward form; every MISTAKE far outside the allowances; the fixed-point Frechet derivative against mpmath; and the float64
model of the device's algorithm against the fixed-point one (the deviations recorded in grad_cases' docstring)."""
import numpy as np
import pytest

from tests import deriv_cases as dc
from tests import grad_cases as gc

BRANCHES = (0, 5, 17, 29)          # two leaves (5: below an ambiguity-free cherry), two internal nodes


def _f(cs):
    return np.asarray(cs["pattern_freq"], dtype=np.float64)


@pytest.mark.parametrize("D", [4, 5, 20])
def test_gradient_contracts_to_d1(D):
    """sum_k x_bk d log L / d x_bk and <Q_b, S_b> both equal deriv_cases' d1 for G = Q_b, within allow_d1."""
    cs, T, x, Q = gc.built_case(D, 2)
    outs, douts = [gc.outside(cs)], [dc.outside(cs)]
    for node in BRANCHES:
        ref = gc.gradient(cs, outs, node, [Q[node]], T=T)
        v = dc.values(cs, douts, node, [Q[node]])
        for what, got in (("x . grad", np.sum(x[node] * ref["grad"][0])), ("<Q, S>", np.sum(Q[node] * ref["S"][0]))):
            assert abs(float(got) - float(v["d1"])) <= float(v["allow_d1"]), (D, node, what, float(got), float(v["d1"]))


def _logl(cs, P):
    ll = dc.site_logl(cs, P)
    f = _f(cs)
    return np.sum(np.where(f > 0, f * np.where(f > 0, ll, 0), 0))


@pytest.mark.parametrize("D,branches", [(4, BRANCHES), (5, BRANCHES), (20, BRANCHES), (61, (17,))])
def test_gradient_against_central_differences(D, branches):
    """Per coefficient: central differences of the longdouble log L, step 1e-6 relative, the perturbed branch's matrix by the
    fixed-point exponential; bar 1e-8 of sum_s f_s |term_s| (truncation about 1e-12, a mistake O(1)).  The forward form
    sum_s f_s g_s V_s^T L(Q, dQ/dx_k) in_s is held to the same bar."""
    cs, T, x, Q = gc.built_case(D, 2, tiny=False)
    outs = [gc.outside(cs)]
    f = _f(cs)
    use = np.isfinite(dc.site_logl(cs, cs["P"]).astype(np.float64))
    cs = dict(cs, pattern_freq=np.where(use, f, 0))       # (patterns impossible at build time take no part on either side)
    for node in branches:
        ref = gc.gradient(cs, outs, node, [Q[node]], T=T)
        terms = gc.forward_terms(cs, outs, node, [Q[node]], T)[0]
        for k in range(len(T)):
            bar = 1e-8 * float(np.sum(_f(cs) * np.abs(terms[k])))
            assert abs(float(np.sum(_f(cs) * terms[k])) - ref["grad"][0][k]) <= bar, (D, node, k, "forward form")
            h = 1e-6 * x[node][k]
            ll = []
            for sign in (1, -1):
                xb = x[node].copy()
                xb[k] += sign * h
                P = np.asarray(cs["P"]).astype(np.longdouble)
                P[node] = gc.expm_fixed(gc.build_q(T, xb))
                ll.append(_logl(cs, P))
            fd = float((ll[0] - ll[1]) / (2 * np.longdouble(h)))
            assert abs(fd - ref["grad"][0][k]) <= bar, (D, node, k, fd, ref["grad"][0][k], bar)


def test_gradient_against_central_differences_three_classes():
    cs, T, x, Q = gc.ladder_template_case()
    w = cs["weights"]
    outs = gc.outs_of(cs)
    f = _f(cs)

    def logl(P):
        ll = np.stack([dc.site_logl(cs, P[c]) for c in range(3)])
        top = ll.max(axis=0)
        return top + np.log(np.sum(w[:, None] * np.exp(ll - top), axis=0))      # (per pattern: the difference is summed)
    for node in cs["branches"][1::2]:
        ref = gc.gradient(cs, outs, node, list(Q[:, node]), weights=w, T=T)
        terms = gc.forward_terms(cs, outs, node, list(Q[:, node]), T, weights=w)
        for c in range(3):
            for k in range(len(T)):
                bar = 1e-8 * float(np.sum(f * np.abs(terms[c, k])))
                h = 1e-6 * x[c, node, k]
                ll = []
                for sign in (1, -1):
                    xb = x[c, node].copy()
                    xb[k] += sign * h
                    P = np.asarray(cs["P"]).astype(np.longdouble)
                    P[c, node] = gc.expm_fixed(gc.build_q(T, xb))
                    ll.append(logl(P))
                fd = float(np.sum(f * (ll[0] - ll[1])) / (2 * np.longdouble(h)))
                assert abs(fd - ref["grad"][c][k]) <= bar, (node, c, k, fd, ref["grad"][c][k], bar)


def test_every_mistake_is_far_outside_the_allowances():
    """Each MISTAKE lies more than 1000 allowances from the reference on at least one case (non-reversible Q, random pi)."""
    single = [gc.built_case(D, 2) for D in (4, 5, 20)]
    lad = gc.ladder_template_case()
    worst = {m: 0.0 for m in gc.MISTAKES}
    for m in gc.MISTAKES:
        for cs, T, x, Q in single:
            good_outs, bad_outs = [gc.outside(cs)], [gc.outside(cs, mistake=m)]
            for node in (5, 17):
                good = gc.gradient(cs, good_outs, node, [Q[node]], T=T)
                bad = gc.gradient(cs, bad_outs, node, [Q[node]], T=T, mistake=m)
                for key, al in (("W", gc.sensitivities(cs, good_outs, node)["allow"]), ("S", good["allow_S"]), ("grad", good["allow_grad"])):
                    dev = np.abs(np.asarray(bad[key] - good[key], dtype=np.float64))
                    worst[m] = max(worst[m], float(np.max(dev / np.asarray(al, dtype=np.float64))))
        cs, T, x, Q = lad
        w = cs["weights"]
        good_outs = gc.outs_of(cs)
        bad_outs = [gc.outside(cs, cs["P"][c], mistake=m) for c in range(3)] if m == "u_for_v" else good_outs
        node = cs["branches"][-1]
        good = gc.sensitivities(cs, good_outs, node, w)
        bad = gc.sensitivities(cs, bad_outs, node, w, mistake=m)
        with np.errstate(invalid="ignore", over="ignore"):
            dev = np.abs(np.asarray(bad["W"] - good["W"], dtype=np.float64))
            worst[m] = max(worst[m], float(np.nanmax(dev / good["allow"].astype(np.float64))))
    print({m: f"{v:.3g}" for m, v in worst.items()})
    assert all(v > 1000 for v in worst.values()), worst


@pytest.mark.parametrize("D", [4, 5, 8])
def test_fixed_point_frechet_against_mpmath(D):
    """frechet_ref equals the upper-right block of mpmath's exp([[Q^T, W], [0, Q^T]]) at 50 digits after rounding to float64, up to
    one unit in the last place of the largest entry."""
    for kind, Q, W in gc.adjoint_cases(D, 1):
        got, want = gc.frechet_ref(Q[0], W[0]), gc.frechet_mpmath(Q[0], W[0])
        assert np.max(np.abs(got - want)) <= 2.0 ** -52 * np.max(np.abs(want)), (D, kind)


def test_frechet_model_against_extended_precision():
    """The float64 model of the device's algorithm against frechet_ref: the largest deviation per entry in units of max |W|, for
    the matrices that need no squaring and for those that do.  What this prints is what grad_cases records; the recorded figures
    must cover it."""
    worst = {False: 0.0, True: 0.0}
    for D in (4, 5, 16, 17, 20):
        for kind, Q, W in gc.adjoint_cases(D):
            for q, w in zip(Q, W):
                dev = float(np.max(np.abs(gc.frechet_model(q, w) - gc.frechet_ref(q, w))) / np.max(np.abs(w)))
                worst[gc.squarings(q) > 0] = max(worst[gc.squarings(q) > 0], dev)
                if kind == "zero":
                    assert np.array_equal(gc.frechet_model(q, w), w)
    print(f"frechet_model - frechet_ref, units of max |W|: no squaring {worst[False]:.3g}, squarings {worst[True]:.3g}")
    assert worst[False] <= gc.MODEL_DEV_PLAIN and worst[True] <= gc.MODEL_DEV_SQUARED, worst


def test_golden_references_match_their_inputs():
    """The stored frechet_ref of adjoint_cases(D) belongs to the matrices the seed gives today; one matrix per state count is
    recomputed."""
    import os
    for D in gc.GOLDEN_D:
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"frechet_adjoint_D{D}.npz"))
        cases = gc.adjoint_cases(D)
        assert np.array_equal(g["check"], np.array([float(np.sum(Q)) + float(np.sum(W)) for _, Q, W in cases])), D
    kind, Q, W = gc.adjoint_cases(48)[5]
    assert np.array_equal(np.load(os.path.join(os.path.dirname(__file__), "golden", "frechet_adjoint_D48.npz"))["S"][5][1], gc.frechet_ref(Q[1], W[1]))
