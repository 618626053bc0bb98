"""Every matrix-exponential kernel and every matrix image against an accurate reference (tests/expm_ref.py): absolute, per entry,
per image, per kernel.  (a) hip.expm_batch on the whole case list, (b) the images the pruning kernels read, entry by entry through
probe partitions (tests/expm_child.py), (c) the variants behind HYPHY_HIP_EXPM, _EXPM_DEGREE, _COEF_INLINE and _EXPM_MASK, each in
a process of its own because the library reads those switches once, (d) the failure path.  Everything under HYPHY_HIP_POISON=1."""
import os

import numpy as np
import pytest

from tests import expm_child as ec
from tests import expm_ref as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY = er.cases_by_name()


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")


@pytest.fixture(scope="module")
def cus():
    return ec.cu_count()


def _hip():
    from hyphy_amd import hip
    return hip


# ---- (a) expm_batch on every case ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", er.STATE_COUNTS)
def test_expm_batch_on_every_case(D, cus):
    """One call per state count (49-64 states: one per batch of tests/expm_ref.batches, so that 4, 2 and 1 workgroups per matrix all
    run, matrices without squarings next to matrices with some): every entry within the allowance of the reference, rows summing to
    1 within 1e-14, nothing below minus the allowance, everything finite, the zero matrix the identity exactly, and the kernel the
    library names is the one the case was written for."""
    worst = {}
    for kernel, names, P in ec.run_batches(D, cus):
        assert kernel == er.kernel_for(D, len(names), cus), (D, len(names), cus, kernel)
        worst[kernel] = max(worst.get(kernel, 0.0), ec.check_batch(kernel, names, P))
    if D >= 49:
        assert set(worst) == {"expm64_kernel<4>", "expm64_kernel<2>", "expm64_kernel<1>"}, worst
    else:
        assert set(worst) == {er.default_kernel(D)}
    print(f"D = {D}: largest deviation / allowance " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))


# ---- (b) the images, entry by entry ----------------------------------------------------------------------------------------------------

PROBE_STATES = (4, 5, 16, 17, 20, 33, 48, 49, 61, 64)
L5 = 5
KINDS = (("leaf", (3, 4), ()), ("ambig", (3,), (3,)), ("internal", (L5 + 1, L5 + 2), ()))   # (leaf 4 and internal 2 hang off the root)


def _expected_kernel(D, n, cus):
    return ("expm_nuc_kernel", "") if D == 4 else (er.kernel_for(D, n, cus, images=True),)


def _case_names(D):
    return [t.format(D=D) for t in ec.PROBE_CASES]


def _allow(name, D, n, cus):
    return er.allowance(name, "expm_nuc_kernel" if D == 4 else er.kernel_for(D, n, cus, images=True))


@pytest.mark.parametrize("kind,branches,amb", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("D", PROBE_STATES)
def test_images_through_plain_evaluate(D, kind, branches, amb, cus):
    """The column-gather image (resolved leaf), the A-operand image (ambiguous leaf, internal branch): a full evaluation, and a
    partial update of the probed branch alone."""
    hip = _hip()
    zero = hip.expm_batch(np.zeros((1, D, D)))[0]
    assert np.array_equal(zero, np.eye(D))           # what the other branches carry
    worst = 0.0
    with ec.Probe(D, L5, branches, amb) as pr:
        for g in range(len(branches)):
            for name in _case_names(D):
                ref = pr.expected(er.case_reference(name))
                got = pr.plain(g, BY[name]["Q"])
                assert hip.last_expm_kernel() in _expected_kernel(D, pr.B, cus), hip.last_expm_kernel()
                worst = max(worst, ec.check_probe(got, ref, _allow(name, D, pr.B, cus), (D, kind, g, name, "full")))
            first = _case_names(D)[0]
            got = pr.partial(g, BY[first]["Q"])
            worst = max(worst, ec.check_probe(got, pr.expected(er.case_reference(first)), _allow(first, D, 1, cus), (D, kind, g, first, "partial")))
    print(f"D = {D}, {kind}: largest deviation / bound {worst:.3f}")


@pytest.mark.parametrize("K", (1, 2, 3, 4, 5, 7))
@pytest.mark.parametrize("D", PROBE_STATES)
def test_images_through_the_built_path(D, K, cus):
    """set_q_templates / build_q / evaluate_built: the rate matrix formed inside the exponential kernel from K templates (the
    accumulation specialised on K <= 4, generic above), every other branch from zero coefficients."""
    hip = _hip()
    worst = 0.0
    for kind, branches, amb in (("leaf", (3,), ()), ("ambig+internal", (3, L5 + 1), (3,))):
        with ec.Probe(D, L5, branches, amb) as pr:
            for g in range(len(branches)):
                for name in _case_names(D):
                    got = pr.built(g, BY[name]["Q"], K)
                    assert hip.last_expm_kernel() in _expected_kernel(D, pr.B, cus), hip.last_expm_kernel()
                    worst = max(worst, ec.check_probe(got, pr.expected(er.case_reference(name)), _allow(name, D, pr.B, cus), (D, K, kind, g, name)))
    print(f"D = {D}, K = {K}: largest deviation / bound {worst:.3f}")


def _some_pairs(D, n, seed):
    rng = np.random.default_rng(seed)
    a, c = rng.integers(0, D, size=n), rng.integers(0, D, size=n)
    corners = [(0, D - 1), (D - 1, 0), (D - 1, D - 1), (0, 0), (D - 1, 47), (48, D - 1), (15, 16), (16, 15), (31, 32), (32, 31)]
    return np.concatenate([np.array(corners), np.stack([a, c], axis=1)])


@pytest.mark.parametrize("L,K,kernel", [(70, 3, "expm64_kernel<1>"), (70, 2, "expm64_kernel<1>"), (40, 3, "expm64_kernel<2>")])
@pytest.mark.parametrize("D", (61, 64))
def test_images_on_ladders_either_side_of_the_inline_coefficient_limit(D, L, K, kernel, cus):
    """138 branches (70 leaves) times K = 3 coefficients exceed the 400 the kernel-argument block takes, times K = 2 they fit; the
    same ladder runs one workgroup per matrix, 40 leaves two (on 256 compute units).  A leaf, an ambiguous leaf, and internal
    branches at both ends and in the middle."""
    hip = _hip()
    assert (2 * L - 2) * 3 > 400 >= (2 * L - 2) * 2 or L != 70
    branches = (0, L - 1, L // 2, L + 0, L + L // 2, 2 * L - 3)
    worst = 0.0
    with ec.Probe(D, L, branches, (L // 2,), pairs=_some_pairs(D, 300, D + L)) as pr:
        if cus == 256:
            assert er.kernel_for(D, pr.B, cus, images=True) == kernel      # (the names in the parametrisation are those of 256 compute units)
        for g in range(len(branches)):
            name = _case_names(D)[g % 2]
            got = pr.built(g, BY[name]["Q"], K)
            assert hip.last_expm_kernel() == er.kernel_for(D, pr.B, cus, images=True)
            worst = max(worst, ec.check_probe(got, pr.expected(er.case_reference(name)), _allow(name, D, pr.B, cus), (D, L, K, g, name)))
        got = pr.plain(2, BY[_case_names(D)[1]]["Q"])
        worst = max(worst, ec.check_probe(got, pr.expected(er.case_reference(_case_names(D)[1])), _allow(_case_names(D)[1], D, pr.B, cus), (D, L, "plain")))
    print(f"D = {D}, L = {L}, K = {K}: {hip.last_expm_kernel()}, largest deviation / bound {worst:.3f}")


@pytest.mark.parametrize("D", (4, 20, 61, 64))
def test_images_of_three_rate_classes(D, cus):
    """evaluate_categories with a different branch probed in each class: the class offsets of the images.  A pattern of group g with
    a != c is impossible in the other classes (their branch b_g is the identity), with a == c every class contributes."""
    hip = _hip()
    branches = (0, L5 + 0, L5 + 1)            # nested: leaf 0, above (0, 1), above (0, 1, 2)
    names = [f"nonrev_D{D}_n0p2", f"nonrev_D{D}_n3", f"rev_D{D}_n0p2"]
    w = np.array([0.5, 0.3, 0.2])
    with ec.Probe(D, L5, branches, C=3) as pr:
        Q = np.zeros((3 * pr.B, D, D))
        for h, (b, name) in enumerate(zip(branches, names)):
            Q[h * pr.B + b] = BY[name]["Q"]
        res = pr.part.evaluate_categories(pr.nodes, pr.nodes, Q, w, pr.pi, per_site=True)
        assert hip.last_expm_kernel() in _expected_kernel(D, 3 * pr.B, cus), hip.last_expm_kernel()
        same = pr.a == pr.c
        for g in range(3):
            ref = np.zeros(len(pr.a))
            allow = np.zeros(len(pr.a))
            for h, name in enumerate(names):
                on = same | (h == g)
                ref += np.where(on, w[h] * pr.expected(er.case_reference(name)), 0.0)
                allow += np.where(on, w[h] * _allow(name, D, 3 * pr.B, cus), 0.0)
            got = pr.read(res, g)
            dev = np.abs(got - ref)
            assert np.all(dev <= allow + 4.0 * np.spacing(ref)), (D, g, float(dev.max()))


@pytest.mark.parametrize("C,cat", [(1, -1), (2, 1)], ids=["one class", "class 1 of 2"])
@pytest.mark.parametrize("D", (4, 20, 61, 64))
def test_images_of_a_branch_site_mixture(D, C, cat, cus):
    """evaluate_mixture with three components against sum_m w_m reference(Q_m): mix_images_kernel writes the images; a resolved
    leaf, an ambiguous leaf and an internal branch; once in class 1 of a two-class partition (the class offset of the images)."""
    hip = _hip()
    names = [f"nonrev_D{D}_n0p2", f"nonrev_D{D}_n3", f"rev_D{D}_n0p2"]
    w = np.array([0.5, 0.3, 0.2])
    ref_P = sum(wm * er.case_reference(n) for wm, n in zip(w, names))
    for branches, amb in (((3, L5 + 1), ()), ((3,), (3,))):
        with ec.Probe(D, L5, branches, amb, C=C) as pr:
            for g, b in enumerate(branches):
                Qc = np.zeros((pr.B, 3, D, D))
                Qc[b] = np.stack([BY[n]["Q"] for n in names])
                W = np.tile(np.array([0.5, 0.25, 0.25]), (pr.B, 1))       # (dyadic: the identity branches mix to exactly 1)
                W[b] = w
                got = pr.read(pr.part.evaluate_mixture(pr.nodes, pr.nodes, Qc, W, pr.pi, cat=cat, per_site=True), g)
                assert hip.last_expm_kernel() == er.kernel_for(D, 3 * pr.B, cus), hip.last_expm_kernel()
                allow = sum(wm * _allow(n, D, 3 * pr.B, cus) for wm, n in zip(w, names))
                ec.check_probe(got, pr.expected(ref_P), allow, (D, branches, amb, g))


def test_images_of_a_rerooted_schedule(monkeypatch, cus):
    """HYPHY_HIP_REROOT=1 on a ladder (its height-minimising node is in the middle): the edges between the given root and that node
    are read through transposed twins, the first of them scaled by pi.  Every branch on that path probed over repeated evaluations
    (the re-rooted form is a steady-state one): the values must not change."""
    hip = _hip()
    for k, v in (("HYPHY_HIP_REROOT", "1"), ("HYPHY_HIP_KERNEL", "1"), ("HYPHY_HIP_CHAIN_M", "3")):
        monkeypatch.setenv(k, v)
    D, L = 61, 12
    path = hip.plan_reroot(ec.ladder(L), L)
    assert len(path) >= 3, path
    branches = tuple(L + int(i) for i in path[1:])
    name = f"nonrev_D{D}_n0p2"
    with ec.Probe(D, L, branches, pairs=_some_pairs(D, 600, 5)) as pr:
        ref = pr.expected(er.case_reference(name))
        seen = False
        for rep in range(4):
            for g in range(len(branches)):
                got = pr.plain(g, BY[name]["Q"])
                ec.check_probe(got, ref, _allow(name, D, pr.B, cus), ("re-rooted", rep, g, pr.part.schedule_info()))
                seen = seen or "re-rooted" in pr.part.schedule_info()
        assert seen, pr.part.schedule_info()


# ---- (c) forced variants, each in a process of its own ------------------------------------------------------------------------------

SETTINGS = [("default", {}), ("EXPM=0", {"HYPHY_HIP_EXPM": "0"}), ("EXPM=1", {"HYPHY_HIP_EXPM": "1"}), ("EXPM=2", {"HYPHY_HIP_EXPM": "2"}),
            ("EXPM=4", {"HYPHY_HIP_EXPM": "4"}), ("EXPM_DEGREE=12", {"HYPHY_HIP_EXPM_DEGREE": "12"}),
            ("COEF_INLINE=0", {"HYPHY_HIP_COEF_INLINE": "0"}), ("EXPM_MASK=0", {"HYPHY_HIP_EXPM_MASK": "0"})]

@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    """{setting: results} of the children, run one after another; the first abnormal exit ends the series."""
    base = tmp_path_factory.mktemp("expm_forced")
    done = {}
    for label, env in SETTINGS:
        out = base / (label.replace("=", "_") + ".npz")
        rc, tail = ec.run_child("forced", out, env, timeout=240)
        if rc != 0:
            done[label] = (rc, tail)
            break
        z = np.load(out)
        done[label] = {k: z[k] for k in z.files}
    return done


def _forced_result(forced, label):
    assert label in forced, f"{label} was not run: an earlier child exited abnormally ({[k for k, v in forced.items() if isinstance(v, tuple)]})"
    assert isinstance(forced[label], dict), forced[label]
    return forced[label]


@pytest.mark.parametrize("label,env", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_forced_variant(label, env, forced):
    """The 49-64-state batches and the 61- and 64-state probes under one setting: the same allowances, and the kernel the setting
    forces.  EXPM_DEGREE=12: also within 2e-15 of the default run where that chose degree 6 or 9.  EXPM_MASK=0: the built-path
    probes equal the default run bit for bit."""
    res = _forced_result(forced, label)
    base = _forced_result(forced, "default")
    cus = int(res["cus"])
    mode = int(env.get("HYPHY_HIP_EXPM", -1))
    fixed = "HYPHY_HIP_EXPM_DEGREE" in env
    worst = 0.0
    for j in range(int(res["n_batches"])):
        kernel, names, P = str(res[f"batch{j}_kernel"]), [str(n) for n in res[f"batch{j}_names"]], res[f"batch{j}_P"]
        D = P.shape[1]
        assert kernel == er.kernel_for(D, len(names), cus, mode), (label, D, len(names), kernel)
        worst = max(worst, ec.check_batch(kernel, names, P, fixed_degree=fixed))
        if fixed:
            assert [str(n) for n in base[f"batch{j}_names"]] == names
            low = [k for k, n in enumerate(names) if er.plan(BY[n]["Q"], kernel)[1] < 12]
            assert low, (label, j)
            d = np.abs(P[low] - base[f"batch{j}_P"][low]).max()
            assert d <= er.BAR_NO_SQUARING, (label, j, float(d))
    kernels = {str(res[f"batch{j}_kernel"]) for j in range(int(res["n_batches"]))}
    want = {0: {"expm_mfma_kernel<4,2>"}, 1: {"expm64_kernel<1>"}, 2: {"expm64_kernel<2>"}, 4: {"expm64_kernel<4>"}}.get(
        mode, {"expm64_kernel<1>", "expm64_kernel<2>", "expm64_kernel<4>"})
    assert kernels == want, (label, kernels)
    for i, lab in enumerate(str(x) for x in res["probe_labels"]):
        D, how, kind, name = lab.split("|")
        kernel, got = str(res[f"probe{i}_kernel"]), res[f"probe{i}_values"]
        assert kernel == er.kernel_for(int(D), 2 * L5 - 2, cus, mode, images=True), (label, lab, kernel)
        ref = er.case_reference(name)
        a, c = np.divmod(np.arange(int(D) ** 2), int(D))
        worst = max(worst, ec.check_probe(got, ref[c, a], er.allowance(name, kernel, fixed), (label, lab)))
        if label == "EXPM_MASK=0" and how == "built":
            assert str(base["probe_labels"][i]) == lab and np.array_equal(got, base[f"probe{i}_values"]), (label, lab)
    for tag in ("few", "more", "many"):        # the failure path in the kernel this setting runs: 5 I is rejected
        n, kernel = int(res[f"reject_{tag}_n"]), str(res[f"reject_{tag}_kernel"])
        assert kernel == er.kernel_for(61, n, cus, mode), (label, tag, kernel)
        assert bool(res[f"reject_{tag}"]), (label, tag, kernel)
    print(f"{label}: kernels {sorted(kernels)}, largest deviation / allowance {worst:.3f}")


@pytest.mark.parametrize("gen,fold", [("0", "0"), ("0", "1"), ("2", "0"), ("2", "1")])
def test_four_state_images_under_interpreter_and_generated_kernel(gen, fold, monkeypatch, cus):
    """4 states: the row-major image and its transposed copy, read by the interpreter (HYPHY_HIP_NUCGEN=0) and by the run-time
    generated kernel (=2, compiled at the first full pass), with the exponentials in a launch of their own (HYPHY_HIP_NUC_FOLD=0) and
    folded into the pruning launch (=1).  Both switches are read at every evaluation.  By the library's own rules every one of these
    partitions takes the variant asked for: five leaves (leaf pairs), at most 512 patterns (a small shard: the generated kernel
    folds too), one program, no pinned state, and no subtree repeats (HYPHY_HIP_REPEATS=0: the class-compressed view has no
    generated kernel) — so nothing falls back, and each evaluation asserts the kernel that pruned and whether the exponentials had a
    launch of their own.  A partial update stays with the interpreter (the generator covers full passes)."""
    hip = _hip()
    monkeypatch.setenv("HYPHY_HIP_NUCGEN", gen)
    monkeypatch.setenv("HYPHY_HIP_NUC_FOLD", fold)
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "0")
    D = 4
    for kind, branches, amb in KINDS:
        with ec.Probe(D, L5, branches, amb) as pr:
            for rep in range(2):
                for g in range(len(branches)):
                    for name in _case_names(D):
                        hip.expm_batch(np.zeros((1, D, D)))       # (so that an empty name afterwards is this evaluation's)
                        assert hip.last_expm_kernel() == "expm_nuc_kernel"
                        got = pr.plain(g, BY[name]["Q"])
                        assert hip.last_expm_kernel() == ("" if fold == "1" else "expm_nuc_kernel"), (gen, fold, kind, rep, g, hip.last_expm_kernel())
                        assert pr.part.prune_kernel_name() == ("nucgen_kernel" if gen == "2" else "prune_nuc2_kernel"), (gen, fold, kind, rep, g)
                        ec.check_probe(got, pr.expected(er.case_reference(name)), er.allowance(name, "expm_nuc_kernel"), (gen, fold, kind, g, name))
            first, second = _case_names(D)
            pr.plain(0, BY[second]["Q"])              # (every other branch the identity again; then branch 0's matrix alone replaced)
            got = pr.partial(0, BY[first]["Q"])
            ec.check_probe(got, pr.expected(er.case_reference(first)), er.allowance(first, "expm_nuc_kernel"), (gen, fold, kind, "partial"))


# ---- (d) the failure path ---------------------------------------------------------------------------------------------------------------

def _bad_matrices(D):
    nan = np.array(BY[f"nonrev_D{D}_n0p2"]["Q"])
    nan[D - 1, 0] = np.nan
    return {"5 I": 5.0 * np.eye(D), "NaN": nan}


@pytest.mark.parametrize("what", ("5 I", "NaN"))
@pytest.mark.parametrize("D", (4, 5, 20, 33, 61))
def test_expm_batch_rejects_what_is_no_rate_matrix(D, what):
    """Q = 5 I and a matrix with a NaN: HipError with the reference's message through the status word, and a later call with a good
    matrix succeeds.  (5 I: the diagonal exp(5 / 2^p) is above 1 at every scale until 5 / 2^p rounds away; restarting as the reference
    does would end at the identity, so a positive diagonal entry fails at the first verification.)"""
    hip = _hip()
    good = f"nonrev_D{D}_n3"
    Q = _bad_matrices(D)[what]
    with pytest.raises(hip.HipError, match="valid transition matrix"):
        hip.expm_batch(np.stack([BY[good]["Q"], Q]))
    P = hip.expm_batch(BY[good]["Q"])
    assert np.abs(P - er.case_reference(good)).max() <= er.allowance(good, er.default_kernel(D)), (D, what)


def test_panel_kernel_rejects_without_squarings():
    """0.2 I at 61 states needs no squaring: the row panels of expm64_kernel<4> report the diagonal above 1 themselves."""
    hip = _hip()
    with pytest.raises(hip.HipError, match="valid transition matrix"):
        hip.expm_batch(0.2 * np.eye(61)[None])
    assert hip.last_expm_kernel() == "expm64_kernel<4>"


@pytest.mark.parametrize("what", ("5 I", "NaN"))
@pytest.mark.parametrize("D", (4, 20, 61))
def test_evaluate_never_uses_a_stale_matrix(D, what):
    """The same matrices on one branch of a partition that has been evaluated with good ones: the evaluation fails or returns NaN,
    never a finite log-likelihood; a fresh partition afterwards gives the first value."""
    hip = _hip()
    rng = np.random.default_rng(40 + D)
    L = 6
    fp = ec.ladder(L)
    B = 2 * L - 2
    codes = rng.integers(0, D, size=(L, 40))
    pi = rng.random(D) + 0.2
    pi /= pi.sum()
    nodes = np.arange(B, dtype=np.int64)
    Q = np.stack([BY[f"nonrev_D{D}_n0p2"]["Q"]] * B)
    bad = _bad_matrices(D)[what]

    def fresh():
        return hip.HipPartition(D, fp, L, codes, None, np.ones(40, dtype=np.int64))

    with fresh() as part:
        first = part.evaluate(nodes, nodes, Q, pi)
    assert np.isfinite(first)
    outcome = []
    for partial in (False, True):
        with fresh() as part:
            good = part.evaluate(nodes, nodes, Q, pi)       # (so that a stale matrix exists)
            assert abs(good - first) <= 1e-12 * abs(first), (D, good, first)
            try:
                if partial:
                    ll = part.evaluate(ec.path_above(fp, L, 2), [2], bad[None], pi)
                else:
                    Qb = Q.copy()
                    Qb[2] = bad
                    ll = part.evaluate(nodes, nodes, Qb, pi)
            except hip.HipError as e:
                assert "valid transition matrix" in str(e), (D, what, partial, str(e))
            else:
                outcome.append((partial, ll))
        with fresh() as part:
            again = part.evaluate(nodes, nodes, Q, pi)
        assert abs(again - first) <= 1e-12 * abs(first), (D, what, partial, again, first)
    print(f"D = {D}, {what}: returned without an error: {outcome}")
    assert all(np.isnan(ll) for _, ll in outcome), (D, what, outcome)
