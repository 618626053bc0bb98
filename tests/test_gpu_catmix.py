"""Rate classes over explicit-form mixtures in one batched evaluation (hyphy_hip_evaluate_categories_mixture and its _built form),
held to the enclosure of tests/catmix_cases.py on every launch form.

Bar.  That of tests/test_gpu_mixture.py::_hold: per pattern and in total lo - t <= got <= hi + t, where [lo, hi] encloses the exact
mixed likelihood of any matrices within the exponential kernels' allowances (catmix_cases.enclosure; narrower than 1e-9 everywhere,
tests/test_catmix_cases_cpu.py) and t = RTOL x |mid| + ATOL of tests/hold.py.  Every test prints the largest
(got - mid) / (half width + t) it saw.  Two device routes to the same value agree to 1e-13 in total and 1e-11 per pattern (SAME,
SITE_ABS of tests/test_gpu_mixture.py).

The sequence (catmix_cases.CatScenario), the reference recomputed at every step: (1) a persisting full batched pass, (2) a lazy one,
(3) a batched partial update of a leaf branch whose count goes 3 -> 16 in every class, (4) the same branch 16 -> 1, (5) a batched
partial update of an internal branch on the re-rooting path, 5 new components per class, (6) a ONE-class evaluate_mixture(cat=1)
partial update of the next branch on that path, class 1's per-pattern values held to class 1's own enclosure, then a batched call
without matrices, (7) the same under new class weights: a re-mix, no exponential kernel runs, (8) download_partials(cat=1),
(9) two last full batched passes.

All tests run under HYPHY_HIP_POISON=1 and HYPHY_HIP_TUNE=0.  The shapes are the smallest at which anything can go wrong: 8 leaves x 40
patterns, and 40 leaves x 24 patterns for the rescale.

Measured on an MI355X (measurements, not tolerances): the 66 tests in 4 s; the largest (got - mid) / (half width + t) per form
0.0001 (0.0003 on cm_deep_D61_40_C3 and cm_poly12_D20_C8).
"""
import numpy as np
import pytest

from tests import catmix_cases as cm
from tests import expm_child as ec
from tests import expm_ref as er
from tests import hmm_ref
from tests import mixture_cases as mc
from tests import test_gpu_mixture as tm
from tests.tuner_child import hold_downloaded

pytestmark = pytest.mark.gpu

SAME, SITE_ABS = tm.SAME, tm.SITE_ABS
CASES = cm.cases_by_name()
NONE = np.zeros(0, dtype=np.int64)
WIDE = ("workgroup", "wave", "team-m2", "rerooted-wave-m2", "levels", "shards3")


def _hip():
    from hyphy_amd import hip
    return hip


def _env(monkeypatch, env):
    tm._env(monkeypatch, env)


def _mk(cs):
    return tm._mk(cs)


def _batched(part, sc, step, branches, entry, w=None, update=None):
    """One batched call on ``branches`` under state[step] (no branch: no matrices) -> (log-L, mixed likelihoods, mixed exponents)."""
    pi = sc.cs["root_freqs"]
    qn = np.asarray(branches, dtype=np.int64)
    un = qn if update is None else update
    w = sc.w if w is None else w
    if entry == "built":
        co, mw = sc.built(step, branches) if len(qn) else ([], [])
        return part.evaluate_categories_mixture_built(un, qn, co, mw, w, pi, per_site=True)
    q, mw = sc.dense(step, branches) if len(qn) else ([], [])
    return part.evaluate_categories_mixture(un, qn, q, mw, w, pi, per_site=True)


def _reduce_form_ok(part, what):
    rf = part.reduce_form()
    assert rf.startswith("site ") and "floor" in rf, (what, rf)


def run_sequence(part, sc, what, form, entry="dense", twin=None, on_full=None):
    """The sequence on ``part`` (module docstring); ``twin``: a second partition on which every step is repeated through the dense
    entry points; ``on_full(part)``: behind the first lazy full pass."""
    hip = _hip()
    cs, C, cus = sc.cs, sc.C, sc.cus
    exps = []

    def call(step, branches, tag, ref=None, w=None):
        got = _batched(part, sc, step, branches, entry, w)
        if len(branches):
            kern = hip.last_expm_kernel()
            assert kern == mc.kernel_for(cs, C * sc.n_tot(step, branches), cus), (what, tag, kern)
        _reduce_form_ok(part, f"{what}: {tag}")
        exps.append(tm._hold(f"{what}: {tag}", form, got, sc.ref(step if ref is None else ref)))
        if twin is not None:
            tm._close(f"{what}: {tag}, built against dense", got, _batched(twin, sc, step, branches, "dense", w))
        return got

    call(1, sc.nodes, "1 persisting full pass")
    call(2, sc.nodes, "2 lazy full pass")
    if on_full:
        on_full(part)
    call(3, [sc.leaf], f"3 branch {sc.leaf} 3 -> 16 components")
    call(4, [sc.leaf], f"4 branch {sc.leaf} 16 -> 1 component")
    call(5, [sc.inner], f"5 inner branch {sc.inner}, 5 components per class")
    got = tm._mix(part, cs, sc.state[6][1], [sc.nxt], entry, cat=1)
    assert hip.last_expm_kernel() == mc.kernel_for(cs, len(sc.single.w), cus), (what, hip.last_expm_kernel())
    tm._hold(f"{what}: 6 one-class update of branch {sc.nxt}, class 1", form, got, sc.ref("cls1"))
    if twin is not None:
        tm._close(f"{what}: 6 one-class update, built against dense", got, tm._mix(twin, cs, sc.state[6][1], [sc.nxt], "dense", cat=1))
    call(6, [], "6 batched call without matrices")
    before = hip.last_expm_kernel()
    call(6, [], "7 re-mix under new class weights", ref=7, w=sc.w_new)
    assert hip.last_expm_kernel() == before
    cache, counts = part.download_partials(1)
    hold_downloaded(f"{what}: 8 download of class 1", cache, counts, sc.ref("cond"))
    call(9, sc.nodes, "9 full pass")
    call(9, sc.nodes, "9 last full pass")
    print(f"{what}: form {form}: largest (got - mid) / (half width + t) so far {tm._worst[form]:.4f}")
    return exps


# ---- the sequence, dense entry point ----------------------------------------------------------------------------------------------------

def _pairs():
    out = []
    for name in cm.names(lambda c: not c["K"] and int(c["D"]) != 4 and "_rep_" not in c["name"]):
        for fid in WIDE:
            if fid.startswith("rerooted") and not name.startswith(("cm_ladder_", "cm_deep_", "cm_classes_")):
                continue          # (a re-rooted schedule needs a re-rooting path)
            out.append(pytest.param(name, fid, id=f"{name}-{fid}"))
    out += [pytest.param("cm_ladder_D4_C3", fid, id=f"cm_ladder_D4_C3-{fid}") for fid in ("interp-fold1-lp1", "generated-small1")]
    return out


@pytest.mark.parametrize("name,fid", _pairs())
def test_sequence_under_every_form(name, fid, monkeypatch):
    _env(monkeypatch, tm.FORMS[fid])
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    with _mk(cs) as part:
        exps = run_sequence(part, sc, f"{name} {fid}", "catmix/" + fid)
    if cs["deep"]:
        assert all(e.max() > 0 for e in exps), (name, fid, [int(e.max()) for e in exps])


def test_sequence_on_the_class_compressed_form(monkeypatch):
    """The ladder with every pattern twice, class-compressed form in use (repeat_stats()[7] == 1 behind a full pass).  The switches
    are those of tests/test_gpu_mixture.py::test_sequence_on_the_class_compressed_form on the same shape: HYPHY_HIP_REPEATS=2 at theta
    0.9.  HYPHY_HIP_REPEATS=1 keeps the size rules (docs/switches.md), and under them 20 distinct patterns get no tables at all
    (measured: available 0, in_use 0), so nothing class-compressed would run."""
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="2", HYPHY_HIP_REP_THETA="0.9"))
    name = "cm_rep_D61_C2"
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())

    def in_use(part):
        assert part.repeat_stats()["in_use"] == 1, (name, part.repeat_stats())

    with _mk(cs) as part:
        run_sequence(part, sc, name, "catmix/compressed", on_full=in_use)


# ---- the sequence, built entry point ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fid", ["wave", "rerooted-wave-m2"])
@pytest.mark.parametrize("name", cm.names(lambda c: c["K"]))
def test_sequence_with_components_built_on_the_device(name, fid, monkeypatch):
    _env(monkeypatch, tm.FORMS[fid])
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    T = mc.templates(int(cs["D"]), cs["K"])
    with _mk(cs) as part, _mk(cs) as twin:
        part.set_q_templates(T)
        run_sequence(part, sc, f"{name} {fid}", "catmix/" + fid + "/built", entry="built", twin=twin)


# ---- relations ----------------------------------------------------------------------------------------------------------------------------

def _host_mix(per, w):
    """The host's class mix of per-class (likelihood, exponent) pairs, in np.longdouble on the smallest exponent -> log per pattern."""
    lik = np.stack([p[1] for p in per]).astype(np.longdouble)
    cnt = np.stack([p[2] for p in per])
    low = cnt.min(axis=0)
    tot = sum(np.longdouble(w[c]) * lik[c] * np.exp2(np.longdouble(-64.0) * (cnt[c] - low)) for c in range(len(per)))
    return (np.log(tot) - low * np.longdouble(tm.LOG_SCALER)).astype(np.float64)


@pytest.mark.parametrize("name", ["cm_ladder_D20_C3", "cm_ladder_D4_C3"])
def test_batched_against_the_host_mix_of_one_class_calls(name, monkeypatch):
    """At 20 and 4 states the exponential kernel does not depend on the batch size: the batched mixed per-pattern values equal the
    host's mix of C one-class evaluate_mixture results on the same components."""
    _env(monkeypatch, {})
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    freq = np.asarray(cs["pattern_freq"], dtype=np.float64)
    with _mk(cs) as part:
        got = _batched(part, sc, 1, sc.nodes, "dense")
    with _mk(cs) as part:
        per = [tm._mix(part, cs, sc.state[1][c], sc.nodes, "dense", cat=c) for c in range(sc.C)]
    host = _host_mix(per, sc.w)
    site = tm._site(got[1], got[2])
    assert np.all(np.abs(site - host) <= SITE_ABS), (name, float(np.abs(site - host).max()))
    total = float(np.sum(host * freq))
    assert abs(got[0] - total) <= SAME * abs(total), (name, got[0], total)


@pytest.mark.parametrize("name", ["ladder_D61", "ladder_D20", "ladder_D4"])
def test_one_class_equals_evaluate_mixture(name, monkeypatch):
    """C == 1: the new entry point with class_weights = [1] against evaluate_mixture."""
    _env(monkeypatch, {})
    cs = mc.cases_by_name()[name]
    sc = mc.scenario(name, 0, ec.cu_count())
    q, w = mc.dense_input(cs, sc.state[1])
    with _mk(cs) as part:
        got = part.evaluate_categories_mixture(sc.nodes, sc.nodes, [q], [w], [1.0], cs["root_freqs"], per_site=True)
        one = np.array([sc.leaf], dtype=np.int64)
        q3, w3 = mc.dense_input(cs, [sc.state[3][sc.leaf]])
        got3 = part.evaluate_categories_mixture(one, one, [q3], [w3], [1.0], cs["root_freqs"], per_site=True)
    with _mk(cs) as part:
        want = tm._mix(part, cs, sc.state[1], sc.nodes, "dense")
        want3 = tm._mix(part, cs, sc.state[3], [sc.leaf], "dense")
    tm._close(f"{name}: C == 1, full pass", got, want)
    tm._close(f"{name}: C == 1, partial update", got3, want3)


def test_resident_values_behind_a_batched_pass(monkeypatch):
    """hmm_set_sites before any pass; behind a batched pass hmm_logl equals hip.hmm_host on the per-class (l, c) read back by
    one-class calls without matrices, at the bar tests/test_gpu_hmm.py holds the device's forward sum to (hmm_ref.bar)."""
    hip = _hip()
    _env(monkeypatch, {})
    name = "cm_ladder_D61_C3"
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    rng = np.random.default_rng(77)
    T, pi0 = hmm_ref.random_chain(rng, 3)
    S = cs["leaf_codes"].shape[1]
    sites = rng.integers(0, S, size=70)
    with _mk(cs) as part:
        part.hmm_set_sites(sites)
        _batched(part, sc, 1, sc.nodes, "dense")
        got = part.hmm_logl(T, pi0)
        per = [part.evaluate_mixture(NONE, NONE, np.zeros((0, 1, 61, 61)), np.zeros((0, 1)), cs["root_freqs"], cat=k, per_site=True) for k in range(3)]
    l, c = np.array([x[1] for x in per]), np.array([x[2] for x in per], dtype=np.int64)
    want = hip.hmm_host(l, c, T, pi0, sites)
    tol = hmm_ref.bar(len(sites), 3, want)
    print(f"hmm behind a batched pass: {got!r} against {want!r}, bar {tol:.3e}")
    assert np.isfinite(want) and abs(got - want) <= tol, (got, want, tol)
    for k in range(3):                             # and the per-class values are the classes' own
        tm._hold(f"{name}: resident values of class {k}", "catmix/resident", per[k], mc.enclosure(cs, sc.state[1][k]))


@pytest.mark.parametrize("tag", sorted(cm.CLASS_WEIGHT_CASES))
@pytest.mark.parametrize("name", ["cm_ladder_D61_C3", "cm_ladder_D20_C3"])
def test_class_weight_cases(name, tag, monkeypatch):
    """A class weight of exactly 0, and a vector far from uniform: inside the enclosure."""
    _env(monkeypatch, {})
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    w = np.array(cm.CLASS_WEIGHT_CASES[tag])
    with _mk(cs) as part:
        got = _batched(part, sc, 1, sc.nodes, "dense", w=w)
    tm._hold(f"{name}: class weights {tag}", "catmix/weights", got, cm.enclosure(cs, sc.state[1], w))


# ---- failure and refusals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cm_ladder_D61_C3", "cm_ladder_D20_C3", "cm_ladder_D4_C3"])
def test_a_bad_component_fails_the_call_whatever_its_weight(name, monkeypatch):
    """A NaN in one component of class 2, at weight 0: < 0 with the "valid transition matrix" text; a full batched pass with good
    matrices then gives the value a fresh partition gives — never a finite value in between."""
    hip = _hip()
    _env(monkeypatch, {})
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    D = int(cs["D"])
    b = 8
    assert len(sc.state[1][2][b].w) == 5
    q, mw = sc.dense(1, sc.nodes)
    q = [[x.copy() for x in qc] for qc in q]
    mw = [[x.copy() for x in wc] for wc in mw]
    bad = np.array(er.cases_by_name()[f"nonrev_D{D}_n0p2"]["Q"])
    bad[D - 1, 0] = np.nan
    q[2][b][2] = bad
    rest = np.delete(mw[2][b], 2)
    mw[2][b] = np.insert(rest / rest.sum(), 2, 0.0)
    pi = cs["root_freqs"]
    with _mk(cs) as part:
        first = _batched(part, sc, 1, sc.nodes, "dense")[0]
    assert np.isfinite(first)
    for partial in (False, True):
        with _mk(cs) as part:
            ok = _batched(part, sc, 1, sc.nodes, "dense")[0]
            assert abs(ok - first) <= SAME * abs(first), (name, ok, first)
            with pytest.raises(hip.HipError, match="valid transition matrix"):
                if partial:
                    one = np.array([b], dtype=np.int64)
                    part.evaluate_categories_mixture(one, one, [[qc[b]] for qc in q], [[wc[b]] for wc in mw], sc.w, pi)
                else:
                    part.evaluate_categories_mixture(sc.nodes, sc.nodes, q, mw, sc.w, pi)
            same = _batched(part, sc, 1, sc.nodes, "dense")[0]
            assert abs(same - first) <= SAME * abs(first), (name, partial, same, first)


def test_refusals(monkeypatch):
    hip = _hip()
    _env(monkeypatch, {})
    name = "cm_built2_D20_C2"
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    pi = cs["root_freqs"]
    lib = hip.load()
    with _mk(cs) as part:
        part.set_q_templates(mc.templates(20, 2))
        q, mw = sc.dense(1, sc.nodes)
        co, _ = sc.built(1, sc.nodes)
        with pytest.raises(hip.HipError, match="first evaluation"):                 # the first call without every branch
            one = sc.nodes[:1]
            part.evaluate_categories_mixture(one, one, [qc[:1] for qc in q], [wc[:1] for wc in mw], sc.w, pi)
        with pytest.raises(hip.HipError, match="class_weights == NULL"):
            part.evaluate_categories_mixture(sc.nodes, sc.nodes, q, mw, None, pi)
        pq, pw, cnt = hip.pack_class_mixture(len(sc.nodes), q, mw, 2)
        for wrong in (0, 17):                                                        # a count of 0 or 17
            c2 = cnt.copy()
            c2[3] = wrong
            out = hip.C.c_double(0.0)
            rc = lib.hyphy_hip_evaluate_categories_mixture(part._h, hip._l(sc.nodes), len(sc.nodes), hip._l(sc.nodes), len(sc.nodes), hip._l(c2),
                                                           hip._d(pq), hip._d(pw), hip._d(sc.w), hip._d(np.ascontiguousarray(pi)), hip.C.byref(out), None, None)
            assert rc < 0 and "1..16 components" in lib.hyphy_hip_last_error().decode(), (wrong, rc)
        pc, _, _ = hip.pack_class_mixture(len(sc.nodes), co, mw, 1)

        def built_call():
            out = hip.C.c_double(0.0)
            rc = lib.hyphy_hip_evaluate_categories_mixture_built(part._h, hip._l(sc.nodes), len(sc.nodes), hip._l(sc.nodes), len(sc.nodes), hip._l(cnt),
                                                                 hip._d(pw), hip._d(sc.w), hip._d(np.ascontiguousarray(pi)), hip.C.byref(out), None, None)
            return rc, lib.hyphy_hip_last_error().decode(), out.value

        part.build_q(pc[:-1])                                                        # rows staged != rows consumed
        rc, msg, _ = built_call()
        assert rc < 0 and "different number of rows" in msg, (rc, msg)
        # rows already claimed as one row per (class, branch): 2 x 14 rows consumed by evaluate_categories_built, then offered again
        part.build_q(np.ascontiguousarray(pc[:2 * len(sc.nodes)]))
        part.evaluate_categories_built_sites(sc.nodes, sc.nodes, sc.w, pi, np.ascontiguousarray(pc[:2 * len(sc.nodes)]))
        ones = np.ones(len(sc.nodes), dtype=np.int64)
        out = hip.C.c_double(0.0)
        w1 = np.ones(2 * len(sc.nodes))
        rc = lib.hyphy_hip_evaluate_categories_mixture_built(part._h, hip._l(sc.nodes), len(sc.nodes), hip._l(sc.nodes), len(sc.nodes), hip._l(ones),
                                                             hip._d(w1), hip._d(sc.w), hip._d(np.ascontiguousarray(pi)), hip.C.byref(out), None, None)
        assert rc < 0 and "(class, branch)" in lib.hyphy_hip_last_error().decode(), lib.hyphy_hip_last_error().decode()
        # rows already claimed as one row per (branch, component) of one class: 58 rows consumed by evaluate_mixture_built(cat=0) under
        # doubled counts ... offered again to the batch, which needs 2 x 29 = 58 too
        twice = [np.concatenate([a, b]) for a, b in zip(co[0], co[1])]
        wtw = [np.concatenate([a, b]) * 0.5 for a, b in zip(mw[0], mw[1])]
        part.evaluate_mixture_built(sc.nodes, sc.nodes, twice, wtw, pi, cat=0)
        rc, msg, _ = built_call()
        assert rc < 0 and "(branch, component)" in msg, (rc, msg)
        # and a good call behind all of them
        good = part.evaluate_categories_mixture_built(sc.nodes, sc.nodes, co, mw, sc.w, pi, per_site=True)
        tm._hold(f"{name}: behind the refusals", "catmix/refusals", good, sc.ref(1))
    cs4 = CASES["cm_ladder_D4_C3"]                                                   # the built form on a 4-state partition
    sc4 = cm.scenario("cm_ladder_D4_C3", ec.cu_count())
    with _mk(cs4) as part:
        part.set_q_templates(np.ones((2, 4, 4)))
        rows = [[np.ones((len(br.w), 2)) for br in st] for st in sc4.state[1]]
        with pytest.raises(hip.HipError, match="MFMA partitions only"):
            part.evaluate_categories_mixture_built(sc4.nodes, sc4.nodes, rows, sc4.dense(1, sc4.nodes)[1], sc4.w, cs4["root_freqs"])


# ---- no existing behaviour moved ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cm_ladder_D61_C3", "cm_ladder_D4_C3"])
def test_one_class_and_plain_category_passes_behind_the_sequence(name, monkeypatch):
    """After the whole sequence on one partition, a one-class evaluate_mixture full pass and a plain evaluate_categories pass each
    give what they give on a fresh partition."""
    _env(monkeypatch, {})
    cs = CASES[name]
    sc = cm.scenario(name, ec.cu_count())
    pi = cs["root_freqs"]
    Q = np.stack([np.stack([tm._matrix(cs, br.names[0]) for br in sc.state[1][c]]) for c in range(sc.C)])

    def both(part):
        a = tm._mix(part, cs, sc.state[1][1], sc.nodes, "dense", cat=1)
        b = part.evaluate_categories(sc.nodes, sc.nodes, Q, sc.w, pi, per_site=True)
        return a, b

    with _mk(cs) as part:
        run_sequence(part, sc, f"{name} before", "catmix/behind")
        got = both(part)
    with _mk(cs) as part:
        want = both(part)
    tm._close(f"{name}: one-class mixture pass behind the sequence", got[0], want[0])
    tm._close(f"{name}: evaluate_categories behind the sequence", got[1], want[1])
