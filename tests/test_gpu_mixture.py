"""Explicit-form mixtures (hyphy_hip_evaluate_mixture, hyphy_hip_evaluate_mixture_built) with a component count of its own on every
branch, held to the enclosure of tests/mixture_cases.py on every launch form.

Bar.  Per pattern and in total lo - t <= got <= hi + t, where [lo, hi] encloses the exact likelihood of any matrices within the
exponential kernels' allowances (mixture_cases.enclosure; narrower than 1e-9 everywhere, tests/test_mixture_cases_cpu.py) and
t = scalefree.GPU_RTOL x |mid| + 1e-9 is tests/hold.py's allowance for the pruning's own rounding.  Exponents are int64 and bounded;
the deep cases show non-zero ones.  Every test prints the largest (got - mid) / (half width + t) it saw.

The sequence (mixture_cases.Scenario), the reference recomputed at every step: (1) a persisting full mixture pass, (2) a lazy one,
(3) a mixture partial update of a leaf branch whose count goes 3 -> 16, (4) the same branch 16 -> 1,
which equals a plain partial update of that matrix to 1e-13, (5) a mixture partial update of the internal branch in the middle of
the re-rooting path, (6) a PLAIN partial update of the next branch on that path, (7) two lazy full mixture passes (their component total is one above that of (1): here the
staging buffers regrow; the single-branch calls of (3) - (5) fit the buffers of the full pass before them), (8) above 4
states the branch cache at a path node, (9) a pinned evaluation at an internal node, un-pinned and a pass behind it, (10)
download_partials, (11) two last full passes.  With templates, the mixture steps go through evaluate_mixture_built and step 6
through build_q + evaluate_built, and every built result is compared with the dense entry point on the same components at 1e-13.

All tests run under HYPHY_HIP_POISON=1 and HYPHY_HIP_TUNE=0; every switch used is read at creation or per call (docs/switches.md).

Measured on an MI355X (measurements, not tolerances; profiles/mixture_tests.md): the 119 tests of the sequences, relations and failure path in 14 s, 1 342 comparisons, the largest
(got - mid) / (half width + t) 0.0003 (the 4-state forms; 0.0001-0.0003 elsewhere): a deviation of 3e-13 where t is 1e-9.  The
slowest ids are deep_D4_120 under the generated kernel, 4.2-4.4 s for the synchronous compilation of a 120-leaf ladder.
"""
import numpy as np
import pytest

from tests import expm_child as ec
from tests import expm_ref as er
from tests import mixture_cases as mc
from tests.hold import ATOL, LOG_SCALER, RTOL
from tests.tuner_child import hold_downloaded

pytestmark = pytest.mark.gpu

SAME = 1e-13       # two device routes to the same value (tests/test_gpu_repeats_states.py, test_explicit_form_mixture_built_*)
SITE_ABS = 1e-11   # ... per pattern, log units
CASES = mc.cases_by_name()

SWITCHES = ("HYPHY_HIP_TUNE", "HYPHY_HIP_TUNE_CACHE", "HYPHY_HIP_KERNEL", "HYPHY_HIP_SLOTS", "HYPHY_HIP_WAVE_VARIANT", "HYPHY_HIP_CHAIN_M", "HYPHY_HIP_CUT",
            "HYPHY_HIP_FRAGMENT", "HYPHY_HIP_REROOT", "HYPHY_HIP_REPEATS", "HYPHY_HIP_REP_THETA", "HYPHY_HIP_POISON", "HYPHY_HIP_FORCE_SHARDS",
            "HYPHY_HIP_FUSED_REDUCE", "HYPHY_HIP_NUCGEN", "HYPHY_HIP_NUCGEN_SMALL", "HYPHY_HIP_NUC_FOLD", "HYPHY_HIP_NUC_LP", "HYPHY_HIP_NUC", "HYPHY_HIP_EXPM",
            "HYPHY_HIP_EXPM_DEGREE", "HYPHY_HIP_COEF_INLINE", "HYPHY_HIP_TRUNK_WALK", "HYPHY_HIP_TRUNK_KERNEL")

WIDE_FORMS = {
    "workgroup": dict(HYPHY_HIP_KERNEL="0"),
    "wave": dict(HYPHY_HIP_KERNEL="1"),
    "team-m2": dict(HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="2"),
    "rerooted-wave-m2": dict(HYPHY_HIP_REROOT="1", HYPHY_HIP_KERNEL="1", HYPHY_HIP_CHAIN_M="2"),
    "rerooted-team-m3": dict(HYPHY_HIP_REROOT="1", HYPHY_HIP_KERNEL="2", HYPHY_HIP_CHAIN_M="3"),
    "shards3": dict(HYPHY_HIP_FORCE_SHARDS="3"),
    "levels": dict(HYPHY_HIP_CUT="levels"),
    "fused0": dict(HYPHY_HIP_FUSED_REDUCE="0"),
    "fused1": dict(HYPHY_HIP_FUSED_REDUCE="1"),
}
NUC_FORMS = {f"interp-fold{f}-lp{lp}": dict(HYPHY_HIP_NUCGEN="0", HYPHY_HIP_NUC_FOLD=f, HYPHY_HIP_NUC_LP=lp) for f in "01" for lp in "01"}
NUC_FORMS.update({f"generated-small{s}": dict(HYPHY_HIP_NUCGEN="2", HYPHY_HIP_NUCGEN_SMALL=s) for s in "01"})
NUC_FORMS.update({k: WIDE_FORMS[k] for k in ("shards3", "fused0", "fused1")})
FORMS = dict(WIDE_FORMS, **NUC_FORMS)

_worst = {}


def _hip():
    from hyphy_amd import hip
    return hip


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _mk(cs):
    return _hip().HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], cs["C"])


def _site(lik, sc):
    with np.errstate(divide="ignore"):
        return np.log(lik) - sc * LOG_SCALER


def _hold(what, form, got, r):
    """got = (log-L, likelihoods, exponents) against an enclosure; returns the exponents."""
    worst = mc.hold_enclosure(what, got, r)
    _worst[form] = max(_worst.get(form, 0.0), worst)
    return got[2]


def _mix(part, cs, state, branches, entry, cat=-1, update=None):
    brs = [state[int(b)] for b in branches]
    qn = np.asarray(branches, dtype=np.int64)
    un = qn if update is None else update
    if entry == "built":
        co, w = mc.built_input(cs, brs)
        return part.evaluate_mixture_built(un, qn, co, w, cs["root_freqs"], cat=cat, per_site=True)
    q, w = mc.dense_input(cs, brs)
    return part.evaluate_mixture(un, qn, q, w, cs["root_freqs"], cat=cat, per_site=True)


def _matrix(cs, name):
    return mc.host_built(int(cs["D"]), cs["K"], name) if cs["K"] else er.cases_by_name()[name]["Q"]


def _close(what, a, b):
    assert abs(a[0] - b[0]) <= SAME * abs(b[0]), (what, a[0], b[0])
    assert np.all(np.abs(_site(a[1], a[2]) - _site(b[1], b[2])) <= SITE_ABS), what


def run_sequence(part, sc, what, form, entry="dense", cat=-1, on_full=None, dense_twin=None):
    """The sequence on ``part`` (module docstring).  ``on_full(part, step)``: behind the last full pass of steps 2, 7 and 11;
    ``dense_twin``: a second partition on which every built mixture step is repeated through the dense entry point."""
    hip = _hip()
    cs, cus = sc.cs, sc.cus
    D, pi = int(cs["D"]), cs["root_freqs"]
    c = max(cat, 0)
    exps = []

    def mix(step, branches, tag):
        st = sc.state[step]
        got = _mix(part, cs, st, branches, entry, cat)
        kern = hip.last_expm_kernel()
        assert kern == mc.kernel_for(cs, sum(len(st[int(b)].w) for b in branches), cus), (what, tag, kern)   # (never "": a mixture does not fold)
        exps.append(_hold(f"{what}: {tag}", form, got, sc.ref(step)))
        if dense_twin is not None:
            _close(f"{what}: {tag}, built against dense", got, _mix(dense_twin, cs, st, branches, "dense", cat))
        return got

    def full(step, tag, check=False):
        got = mix(step, sc.nodes, tag)
        if check and on_full:
            on_full(part, step)
        return got

    full(1, "1 persisting full pass")
    full(2, "2 lazy full pass", check=True)
    mix(3, [sc.leaf], f"3 branch {sc.leaf} 3 -> 16 components")
    got = mix(4, [sc.leaf], f"4 branch {sc.leaf} 16 -> 1 component")
    one = np.array([sc.leaf], dtype=np.int64)
    plain = part.evaluate(one, one, _matrix(cs, sc.single.names[0])[None], pi, cat=cat, per_site=True)
    _close(f"{what}: 4 one component of weight 1 against a plain update", got, plain)
    mix(5, [sc.inner], f"5 inner branch {sc.inner}, 5 components")
    one = np.array([sc.nxt], dtype=np.int64)
    if entry == "built":
        part.build_q(mc.coefficient_row(D, cs["K"], sc.plain.names[0])[None])
        got = part.evaluate_built(one, one, pi, cat=cat, per_site=True)
        if dense_twin is not None:
            dense_twin.evaluate(one, one, _matrix(cs, sc.plain.names[0])[None], pi, cat=cat)
    else:
        got = part.evaluate(one, one, _matrix(cs, sc.plain.names[0])[None], pi, cat=cat, per_site=True)
    exps.append(_hold(f"{what}: 6 plain update of branch {sc.nxt}", form, got, sc.ref(6)))
    full(7, "7 full pass")
    full(7, "7 lazy full pass", check=True)
    if D != 4:
        part.branch_cache_build(sc.bc, cat=c)
        got = part.branch_cache_evaluate(sc.bc, _matrix(cs, sc.bc_branch.names[0]), cat=c, per_site=True)
        _hold(f"{what}: 8 branch cache at {sc.bc}", form, got, sc.ref(8))
    part.set_pinned_states(sc.pin, sc.states)
    try:
        got = _mix(part, cs, sc.state[6], sc.nodes, entry, cat)
    finally:
        part.set_pinned_states(None)
    _hold(f"{what}: 9 pinned at {sc.pin}", form, got, sc.ref("pin"))
    full(7, "9 full pass behind the pin")
    cache, counts = part.download_partials(c)
    hold_downloaded(f"{what}: 10 download", cache, counts, sc.ref("cond"))
    full(11, "11 full pass")
    full(11, "11 last full pass", check=True)
    print(f"{what}: form {form}: largest (got - mid) / (half width + t) so far {_worst[form]:.4f}")
    return exps


# ---- every launch form ---------------------------------------------------------------------------------------------------------------

def _pairs():
    out = []
    for name in mc.names(lambda c: c["C"] == 1 and not c["K"] and not c["name"].startswith("rep_")):
        nuc = int(CASES[name]["D"]) == 4
        for fid in (NUC_FORMS if nuc else WIDE_FORMS):
            if fid.startswith("rerooted") and not name.startswith(("ladder_", "deep_D61")):
                continue          # (a re-rooted schedule needs a re-rooting path: tests/test_mixture_cases_cpu.py)
            out.append(pytest.param(name, fid, id=f"{name}-{fid}"))
    return out


def _on_full(name, fid):
    env = FORMS[fid]
    nuc = int(CASES[name]["D"]) == 4

    def check(part, step):
        info = part.schedule_info()
        if fid.startswith("rerooted") and step in (7, 11):
            assert "re-rooted" in info, (name, fid, step, info)
        if nuc and "HYPHY_HIP_NUCGEN" in env:
            want = "nucgen_kernel" if env["HYPHY_HIP_NUCGEN"] == "2" else "prune_nuc2_kernel"
            assert part.prune_kernel_name() == want, (name, fid, step, part.prune_kernel_name(), info)
        if fid in ("workgroup", "wave", "team-m2") and int(CASES[name]["D"]) > 48:
            want = "prune_wave_kernel" if fid == "wave" else "prune_mfma_kernel"
            assert part.prune_kernel_name() == want, (name, fid, step, part.prune_kernel_name(), info)
    return check


@pytest.mark.parametrize("name,fid", _pairs())
def test_sequence_under_every_form(name, fid, monkeypatch):
    _env(monkeypatch, FORMS[fid])
    cs = CASES[name]
    sc = mc.scenario(name, 0, ec.cu_count())
    with _mk(cs) as part:
        exps = run_sequence(part, sc, f"{name} {fid}", fid, on_full=_on_full(name, fid))
    if cs["deep"]:
        assert all(e.max() > 0 for e in exps), (name, fid, [int(e.max()) for e in exps])


@pytest.mark.parametrize("name", ["rep_D61", "rep_D20"])
def test_sequence_on_the_class_compressed_form(name, monkeypatch):
    """HYPHY_HIP_REPEATS=2 at theta 0.9 on the ladders with every pattern twice; the pinned and branch-cache steps run plain by the
    library's own rule."""
    _env(monkeypatch, dict(HYPHY_HIP_REPEATS="2", HYPHY_HIP_REP_THETA="0.9"))
    cs = CASES[name]
    sc = mc.scenario(name, 0, ec.cu_count())

    def in_use(part, step):
        assert part.repeat_stats()["in_use"] == 1, (name, step, part.repeat_stats())

    with _mk(cs) as part:
        in_use(part, 0)
        run_sequence(part, sc, name, "compressed", on_full=in_use)


@pytest.mark.parametrize("fid", ["workgroup", "wave", "team-m2"])
def test_two_classes(fid, monkeypatch):
    """The sequence on class 1 of a two-class partition, a full pass on class 0 under other components, then class 1 again without
    matrices (n_q = 0 on the dense entry point): still class 1's value."""
    _env(monkeypatch, FORMS[fid])
    name = "classes_D61"
    cs = CASES[name]
    sc0, sc1 = (mc.scenario(name, k, ec.cu_count()) for k in (0, 1))
    none = np.zeros(0, dtype=np.int64)
    with _mk(cs) as part:
        run_sequence(part, sc1, f"{name} {fid} class 1", fid + "/classes", cat=1)
        for k in range(2):
            got = _mix(part, cs, sc0.state[1], sc0.nodes, "dense", 0)
            _hold(f"{name} {fid} class 0, pass {k}", fid + "/classes", got, sc0.ref(1))
        got = part.evaluate_mixture(sc1.nodes, none, np.zeros((0, 1, 61, 61)), np.zeros((0, 1)), cs["root_freqs"], cat=1, per_site=True)
        _hold(f"{name} {fid} class 1 without matrices", fid + "/classes", got, sc1.ref(11))
        got = _mix(part, cs, sc1.state[6], sc1.nodes, "dense", 1)
        _hold(f"{name} {fid} class 1 again", fid + "/classes", got, sc1.ref(11))


def _built_pairs():
    out = []
    for name in mc.names(lambda c: c["K"]):
        D = int(CASES[name]["D"])
        forms = ("interp-fold1-lp1", "generated-small1") if D == 4 else ("wave", "team-m2", "rerooted-wave-m2")
        if "400" in name:
            forms = ("wave", "rerooted-team-m3")
        out += [pytest.param(name, fid, id=f"{name}-{fid}") for fid in forms]
    return out


@pytest.mark.parametrize("name,fid", _built_pairs())
def test_sequence_with_components_built_on_the_device(name, fid, monkeypatch):
    _env(monkeypatch, FORMS[fid])
    cs = CASES[name]
    sc = mc.scenario(name, 0, ec.cu_count())
    T = mc.templates(int(cs["D"]), cs["K"])
    with _mk(cs) as part, _mk(cs) as twin:
        part.set_q_templates(T)
        run_sequence(part, sc, f"{name} {fid}", fid + "/built", entry="built", on_full=_on_full(name, fid), dense_twin=twin)


def test_prepared_step_with_a_count_per_branch(monkeypatch):
    """prepare_mixture_built_step with ``counts``: flat rows and weights, read at call time; equal to evaluate_mixture_built on the
    same rows, and inside the enclosure."""
    hip = _hip()
    _env(monkeypatch, {})
    name = "built3_D61"
    cs = CASES[name]
    sc = mc.scenario(name, 0, ec.cu_count())
    pi = cs["root_freqs"]
    r = sc.ref(7)
    tt = RTOL * abs(r["mid_total"]) + ATOL
    with _mk(cs) as part:
        part.set_q_templates(mc.templates(61, 3))
        co, w, cnt = hip.pack_mixture(len(sc.nodes), *mc.built_input(cs, sc.state[6]), 1)
        assert cnt.tolist() == [len(br.w) for br in sc.state[6]] and len(set(cnt.tolist())) > 2
        split = np.cumsum(cnt)[:-1]
        step = part.prepare_mixture_built_step(sc.nodes, sc.nodes, w, pi, co, counts=cnt)

        def both(tag):
            got = step()
            want = part.evaluate_mixture_built(sc.nodes, sc.nodes, np.split(co, split), np.split(w, split), pi)
            assert np.isfinite(got) and abs(got - want) <= SAME * abs(want), (tag, got, want)
            return got

        got = both("as staged")
        assert r["lo_total"] - tt <= got <= r["hi_total"] + tt, (got, r["lo_total"], r["hi_total"])
        first = got
        co *= 0.5                                    # other values in place under the same counts: half the rates,
        for k, part_w in enumerate(np.split(w, split)):
            part_w[:] = part_w[::-1].copy()          # the weights of every branch reversed (np.split gives views)
        assert both("changed in place") != first


# ---- relations that need no reference ------------------------------------------------------------------------------------------------

def _variants(sc):
    """{label: state} of rewritings of state[1] that leave every P_b what it is."""
    base = sc.state[1]
    out = {}
    b = next(k for k, br in enumerate(base) if np.any(br.w == 0.0))
    keep = base[b].w != 0.0
    st = list(base)
    st[b] = mc.Branch([n for n, k in zip(base[b].names, keep) if k], base[b].w[keep], base[b].kernel)
    out[f"zero-weight component of branch {b} removed"] = st
    b = next(k for k, br in enumerate(base) if len(br.w) == 3)
    st = list(base)
    st[b] = mc.Branch((base[b].names[0],) + base[b].names, np.r_[0.5 * base[b].w[0], 0.5 * base[b].w[0], base[b].w[1:]], base[b].kernel)
    out[f"first component of branch {b} as two halves"] = st
    b = next(k for k, br in enumerate(base) if len(br.w) == 16)
    order = np.random.default_rng(5).permutation(16)
    st = list(base)
    st[b] = mc.Branch([base[b].names[k] for k in order], base[b].w[order], base[b].kernel)
    out[f"components of branch {b} permuted"] = st
    return out, b


@pytest.mark.parametrize("name", ["ladder_D4", "ladder_D20", "ladder_D61"])
def test_rewritings_of_a_mixture_give_the_same_value(name, monkeypatch):
    _env(monkeypatch, {})
    cs = CASES[name]
    sc = mc.scenario(name, 0, ec.cu_count())
    variants, b16 = _variants(sc)
    with _mk(cs) as part:
        base = _mix(part, cs, sc.state[1], sc.nodes, "dense")
        for label, st in variants.items():
            _close(f"{name}: {label}", _mix(part, cs, st, sc.nodes, "dense"), base)
        _close(f"{name}: back", _mix(part, cs, sc.state[1], sc.nodes, "dense"), base)
        st = variants[f"components of branch {b16} permuted"]
        _close(f"{name}: permuted, as a partial update", _mix(part, cs, st, [b16], "dense"), base)
        # one component of weight 1 on every branch: a plain evaluation
        singles = [mc.Branch(br.names[:1], [1.0], br.kernel) for br in sc.state[1]]
        got = _mix(part, cs, singles, sc.nodes, "dense")
        Q = np.stack([_matrix(cs, br.names[0]) for br in singles])
    with _mk(cs) as part:
        plain = part.evaluate(sc.nodes, sc.nodes, Q, cs["root_freqs"], per_site=True)
    _close(f"{name}: count 1, weight 1 against evaluate", got, plain)


# ---- the failure path ---------------------------------------------------------------------------------------------------------------------

def _bad(D, what):
    if what == "5 I":
        return 5.0 * np.eye(D)
    Q = np.array(er.cases_by_name()[f"nonrev_D{D}_n0p2"]["Q"])
    Q[D - 1, 0] = np.nan
    return Q


@pytest.mark.parametrize("weight", [0.3, 0.0])
@pytest.mark.parametrize("what", ["5 I", "NaN"])
@pytest.mark.parametrize("D", [4, 20, 61])
def test_a_bad_component_never_gives_a_finite_value(D, what, weight, monkeypatch):
    """A NaN matrix or 5 I as the third of the five components of branch 8, in the middle of the list, at weight 0.3 and at weight 0,
    in a full pass and in a partial update of a partition already evaluated with good mixtures: HipError("... valid transition
    matrix") or NaN, never a finite value (measured: the error in all 24 combinations; the contract in include/hyphy_hip.h says an
    error whatever the weight); the same partition afterwards, and a fresh one, give the first value under the good mixture."""
    hip = _hip()
    _env(monkeypatch, {})
    name = f"ladder_D{D}"
    cs = CASES[name]
    sc = mc.scenario(name, 0, ec.cu_count())
    b = 8
    good = sc.state[1]
    assert len(good[b].w) == 5
    q, w = mc.dense_input(cs, good)
    q, w = [x.copy() for x in q], [x.copy() for x in w]
    q[b][2] = _bad(D, what)
    rest = np.delete(w[b], 2)
    w[b] = np.insert(rest / rest.sum() * (1.0 - weight), 2, weight)
    pi = cs["root_freqs"]
    with _mk(cs) as part:
        first = _mix(part, cs, good, sc.nodes, "dense")[0]
    assert np.isfinite(first)
    outcome = []
    for partial in (False, True):
        with _mk(cs) as part:
            ok = _mix(part, cs, good, sc.nodes, "dense")[0]
            assert abs(ok - first) <= 1e-12 * abs(first), (name, ok, first)
            try:
                if partial:
                    one = np.array([b], dtype=np.int64)
                    ll = part.evaluate_mixture(one, one, [q[b]], [w[b]], pi)
                else:
                    ll = part.evaluate_mixture(sc.nodes, sc.nodes, q, w, pi)
            except hip.HipError as e:
                assert "valid transition matrix" in str(e), (name, what, weight, partial, str(e))
                outcome.append((partial, "error"))
            else:
                outcome.append((partial, ll))
            same = _mix(part, cs, good, sc.nodes, "dense")[0]          # the same partition recovers with a full pass of good matrices
            assert abs(same - first) <= 1e-12 * abs(first), (name, what, weight, partial, same, first)
        with _mk(cs) as part:
            again = _mix(part, cs, good, sc.nodes, "dense")[0]
        assert abs(again - first) <= 1e-12 * abs(first), (name, what, weight, partial, again, first)
    print(f"D = {D}, {what}, weight {weight}: (partial, outcome) {outcome}")
    assert all(o == "error" or np.isnan(o) for _, o in outcome), (name, what, weight, outcome)
