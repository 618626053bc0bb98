"""Call sequences on the class-compressed form (repeats.hip) with the 2^64 rescale in play, held to tests/scalefree.py.

The cases, the sequences and their replayed references are tests/compressed_cases.py's: partial updates at a leaf and an inner branch
of a table, above a topmost table, on the trunk and at a leaf with ambiguity codes — alone, several at once, the same dirty set
twice, more dirty sets than the item-queue ring has slots — a re-evaluation, new root frequencies, a download between two compressed
passes, full passes, a sequence in which patterns become impossible and possible again, and three rate classes whose exponents lie
far apart.  The per-class exponents (``rep_cnt``) and the walk's hand-over (``hand_cnt``) are non-zero throughout and move at every
partial step.  The download runs a persisting full pass under the partition's own tree — the library never re-expands the class
tables — and the compressed pass behind it is promoted to a full one: that step holds the plain pass between two compressed ones
and the full rebuild of the tables after it, not a partial pass after a view switch (tests/test_compressed_cases_cpu.py shows that, and that a stale table is at
least 1000 allowances away).

Every step goes through tests/hold.py::_hold: per pattern and in total at GPU_RTOL x |reference| + 1e-9, -inf exactly where the
reference has it, exponents integral.  HYPHY_HIP_REPEATS=2, HYPHY_HIP_TUNE=0, HYPHY_HIP_POISON=1; ``repeat_stats()["in_use"] == 1``
before the first step and after the last.  The last two full passes of every sequence equal a fresh partition's bit for bit."""
import numpy as np
import pytest

from tests import compressed_cases as cc
from tests.hold import ATOL, LOG_SCALER, RTOL, _hold

pytestmark = pytest.mark.gpu

THETAS = ("0.05", "0.9")


def _mk(fx, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(fx["D"]), fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], C)


def _forms(D):
    """The trunk forms that exist at ceil(D / 16) row blocks (test_gpu_repeats_states._forms): (label, environment, kernel expected
    on lazy full passes)."""
    nw = (D + 15) // 16
    forms = [("wave", dict(HYPHY_HIP_TRUNK_WALK="0"), "prune_wave_kernel")]
    if nw >= 2:
        forms += [(f"walk/{c}", dict(HYPHY_HIP_TRUNK_WALK="1", HYPHY_HIP_WALK_CHAINS=str(c)), "trunk_walk_kernel") for c in (1, 2)]
    if nw == 4:
        forms += [(f"wg/{k}", dict(HYPHY_HIP_TRUNK_WALK="0", HYPHY_HIP_TRUNK_KERNEL=str(k)), "prune_mfma_kernel") for k in (0, 2)]
    return forms


def _form(D, label):
    return {lab: (env, kernel) for lab, env, kernel in _forms(D)}[label]


def _setenv(monkeypatch, theta=None, **env):
    monkeypatch.setenv("HYPHY_HIP_REPEATS", "2")
    monkeypatch.setenv("HYPHY_HIP_TUNE", "0")
    monkeypatch.setenv("HYPHY_HIP_POISON", "1")
    if theta is not None:
        monkeypatch.setenv("HYPHY_HIP_REP_THETA", theta)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _call(part, step):
    what, un, qn, M, pi, entry = step
    if entry == "categories":
        return part.evaluate_categories(un, qn, M, cc.CLASS_WEIGHTS, pi, q_is_probability=True, per_site=True)
    cat = entry[1] if isinstance(entry, tuple) else -1
    return part.evaluate(un, qn, M, pi, cat=cat, q_is_probability=True, per_site=True)


def _hold_download(what, part, rec):
    """Conditionals divided by their largest element against the reference's, log(largest) - 64 ln2 count against its log-magnitude,
    zero vectors exactly where the reference has them (test_gpu_rescale.py::test_downloaded_conditionals_and_counts)."""
    ref = rec["ref"]
    cache, counts = part.download_partials()
    top = cache.max(axis=2)
    zero = ~(ref["cond"].max(axis=2) > 0)
    assert np.array_equal(top == 0, zero), (what, np.argwhere((top == 0) != zero)[:8])
    assert np.all(cache[zero] == 0), what
    norm = cache / np.where(top > 0, top, 1.0)[:, :, None]
    assert np.allclose(norm, ref["cond"], rtol=1e-9, atol=1e-12), what
    with np.errstate(divide="ignore"):
        mag = np.log(top) - LOG_SCALER * counts
    ok = ~zero
    dev = np.abs(mag[ok] - ref["log_mag"][ok])
    allow = RTOL * np.abs(ref["log_mag"][ok]) + ATOL
    print(f"{what}: largest log-magnitude deviation / allowance = {float(np.max(dev / allow)):.3f}; largest count {int(counts.max())}")
    assert np.all(dev <= allow), (what, float(np.max(dev / allow)))
    return cache, counts


def _play(part, fx, D, which, label, kernel=None, hold=True):
    """Every step of the sequence on ``part``, held to its replayed reference (``hold``); returns the results (of a download: the
    conditionals and counts)."""
    out = []
    for step, rec in zip(cc.sequence(D, which), cc.replay(D, which)):
        what = f"D = {D} {which} {label} '{step[0]}'"
        if step[5] == "download":
            out.append(_hold_download(what, part, rec) if hold else part.download_partials())
            continue
        got = _call(part, step)
        if hold:
            site, total = cc.step_reference(fx, rec)
            _hold(f"{what} [{part.prune_kernel_name()}]", got, site, total)
            if kernel and "(lazy)" in step[0]:
                assert part.prune_kernel_name() == kernel, (what, part.prune_kernel_name(), part.schedule_info())
        out.append(got)
    return out


def _assert_same(x, y, what):
    """Identical bytes: log-L, per-pattern likelihoods and exponents (of a download: conditionals and counts)."""
    if len(x) == 2:
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes(), (what, int(np.sum(x[0] != y[0])), int(np.sum(x[1] != y[1])))
        return
    diff = np.flatnonzero((x[1] != y[1]) | (x[2] != y[2]))
    detail = [(int(s), float(x[1][s]), float(y[1][s]), int(x[2][s]), int(y[2][s])) for s in diff[:4]]
    assert len(diff) == 0 and x[1].tobytes() == y[1].tobytes(), (what, f"{len(diff)} patterns differ", detail)
    assert x[0] == y[0], (what, "the totals differ over identical per-pattern values", x[0], y[0], x[0] - y[0])


def _run(D, which, label, kernel=None, C=1):
    """The sequence, every step held, on a partition that must be compressed from the first step to the last."""
    fx = cc.case(D)
    with _mk(fx, C) as part:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        _play(part, fx, D, which, label, kernel)
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()


def _run_bytes(D, which, label, C=1, whole=False):
    """The sequence on one partition, then its last two (full) passes on a fresh one: identical bytes, nothing of the sequence is left
    behind.  ``whole``: the whole sequence on the fresh one, every step compared."""
    fx = cc.case(D)
    steps = cc.sequence(D, which)
    with _mk(fx, C) as part:
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
        got = _play(part, fx, D, which, label, hold=False)
        assert part.repeat_stats()["in_use"] == 1, part.repeat_stats()
    tail = (len(steps) - 2, len(steps) - 1)
    assert all(len(steps[k][1]) == len(fx["flat_parents"]) - 1 for k in tail)
    with _mk(fx, C) as fresh:
        assert fresh.repeat_stats()["in_use"] == 1, fresh.repeat_stats()
        if whole:
            again = _play(fresh, fx, D, which, label, hold=False)
            for k, (x, y) in enumerate(zip(got, again)):
                _assert_same(x, y, (D, which, label, steps[k][0], "differs on a second partition"))
        else:
            for k in tail:
                _assert_same(got[k], _call(fresh, steps[k]), (D, which, label, steps[k][0], "differs from a fresh partition's"))
        assert fresh.repeat_stats()["in_use"] == 1, fresh.repeat_stats()


_MAIN = [(D, theta, label, rho) for D in cc.WIDE for theta in THETAS for label, _, _ in _forms(D) for rho in ("0", "2")]


@pytest.mark.parametrize("D,theta,form,rho", _MAIN)
def test_main_sequence_under_each_trunk_form(D, theta, form, rho, monkeypatch):
    """rho = 0: a compressed subtree is one path; rho = 2: tables read other tables' exponents (position (b) is a table boundary)."""
    env, kernel = _form(D, form)
    _setenv(monkeypatch, theta, HYPHY_HIP_REP_RHO=rho, **env)
    _run(D, "main", f"{form} theta {theta} rho {rho}", kernel)


@pytest.mark.parametrize("D,theta,form,rho", _MAIN)
def test_main_sequence_leaves_nothing_behind(D, theta, form, rho, monkeypatch):
    """The last two full passes of the main sequence equal a fresh partition's, bit for bit.

    (At D = 17, theta = 0.05 this used to fail on 2 to 6 of the 6 forms per run, with 1 to 8 of the 246 patterns off in the last bit:
    a trunk node with two internal children and leaf children was formed as (a x leaves) x b or (b x leaves) x a, by which child's
    wave arrived last.  The chain schedules now list the deposited children ahead of the leaf groups.)"""
    env, _ = _form(D, form)
    _setenv(monkeypatch, theta, HYPHY_HIP_REP_RHO=rho, **env)
    _run_bytes(D, "main", f"{form} theta {theta} rho {rho}")


@pytest.mark.parametrize("form", ["wave", "walk/2"])
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("D", cc.CLOSED_D)
def test_closed_sequence(D, theta, form, monkeypatch):
    """Every matrix cuts the last state off; a branch is opened, closed, opened with others: -inf appears and leaves exactly."""
    env, kernel = _form(D, form)
    _setenv(monkeypatch, theta, HYPHY_HIP_REP_RHO="2", **env)
    _run(D, "closed", f"{form} theta {theta}", kernel)
    _run_bytes(D, "closed", f"{form} theta {theta}")


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("D", [33, 61])
def test_ticket_protocol(D, theta, monkeypatch):
    """HYPHY_HIP_REP_LEVELS=0 at rho = 2: tables read other tables' exponents inside one launch."""
    _setenv(monkeypatch, theta, HYPHY_HIP_REP_RHO="2", HYPHY_HIP_REP_LEVELS="0")
    _run(D, "main", f"tickets theta {theta}")
    _run_bytes(D, "main", f"tickets theta {theta}")


@pytest.mark.parametrize("rho", ["0", "2"])
@pytest.mark.parametrize("theta", THETAS)
def test_shards(theta, rho, monkeypatch):
    """Three shards at D = 61: every shard plans its own classes."""
    _setenv(monkeypatch, theta, HYPHY_HIP_REP_RHO=rho, HYPHY_HIP_FORCE_SHARDS="3")
    _run(61, "main", f"3 shards theta {theta} rho {rho}")
    _run_bytes(61, "main", f"3 shards theta {theta} rho {rho}")


@pytest.mark.parametrize("theta", [None, "0.05"])
def test_four_states(theta, monkeypatch):
    """The 4-state table kernel (one thread per class walks a whole subtree) below prune_nuc_kernel, set up as
    test_gpu_repeats.py::test_four_states_compressed_equals_plain_and_reference does (and once more at the low threshold)."""
    _setenv(monkeypatch, theta)
    fx = cc.case(4)
    with _mk(fx) as part:
        st = part.repeat_stats()
        assert st["available"] == 1 and st["tables"] > 0, st
        assert part.prune_kernel_name() in ("prune_nuc_kernel", "prune_nuc2_kernel")
    _run(4, "main", f"4 states theta {theta}")
    _run_bytes(4, "main", f"4 states theta {theta}")


@pytest.mark.parametrize("walk", ["0", "1"])
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("D", cc.CLASS_D)
def test_rate_classes(D, theta, walk, monkeypatch):
    """Off-diagonals 1e-2 / 1e-12 / 1e-30: all classes in one call (full, lazy, three partial batches), then a partial update of each
    class alone, held to that class's own values."""
    _setenv(monkeypatch, theta, HYPHY_HIP_TRUNK_WALK=walk)
    _run(D, "classes", f"classes walk {walk} theta {theta}", C=3)
    _run_bytes(D, "classes", f"classes walk {walk} theta {theta}", C=3)


@pytest.mark.parametrize("D,form", [(5, "wave"), (20, "walk/2"), (33, "walk/1"), (61, "wg/0")])
def test_a_second_partition_replays_the_sequence_to_the_same_bytes(D, form, monkeypatch):
    """One case per row-block count: the whole main sequence twice, on two fresh partitions, poisoned buffers and all."""
    env, _ = _form(D, form)
    _setenv(monkeypatch, "0.05", HYPHY_HIP_REP_RHO="2", **env)
    _run_bytes(D, "main", f"{form} twice", whole=True)
