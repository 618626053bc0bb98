"""The two comparisons tests/test_gpu_reduce.py makes of every evaluation, and a child process for the switch that is read once per
process (HYPHY_HIP_REDUCE):

    python -m tests.reduce_child FORM D n        e.g.  block 5 513   /   wave 5 4097

runs the (D, n) cases of tests/reduce_cases.py (a persisting and a lazy full pass each) under the HYPHY_HIP_REDUCE of its environment,
asserts that ``FORM n=<n>`` ran, and ends with a line ``RESULT {json}``.

(a) ``hold_reference``: per pattern and total against the scale-free reference, as tests/hold.py::_hold does, but admitting a NaN
    where the case says so (``_hold`` asserts isfinite(lik)).
(b) ``hold_exact``: the returned log L against an exact sum of the per-pattern (l_s, c_s) the SAME call returned
    (reduce_cases.exact_sum), at 8 x 2^-53 of the summed magnitudes.  The per-pattern values are the operation's inputs here; (a) and
    the other suites hold them."""
import json
import math
import os
import sys

import numpy as np

from tests import reduce_cases as rc
from tests.hold import ATOL, RTOL, _site

WORST = {}          # combiner -> (largest ratio of (b), case) seen in this process


def mk(cs, C=1):
    from hyphy_amd import hip
    return hip.HipPartition(int(cs["D"]), cs["flat_parents"], int(cs["L"]), cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], C)


def nodes_of(cs):
    return np.arange(len(cs["flat_parents"]) - 1, dtype=np.int64)


def full(cs, part, P=None):
    n = nodes_of(cs)
    return part.evaluate(n, n, cs["P"] if P is None else P, cs["root_freqs"], q_is_probability=True, per_site=True)


def hold_reference(what, got, want_site, want_total, freq):
    """(a)  ``want_site``: -inf where the pattern is impossible, NaN where its likelihood is NaN."""
    ll, lik, sc = got
    assert sc.dtype == np.int64 and np.all(np.abs(sc) < 4096), (what, sc)
    nan = np.isnan(want_site)
    assert np.array_equal(np.isnan(lik), nan), (what, "NaN patterns", np.flatnonzero(np.isnan(lik) != nan))
    assert np.all(np.isfinite(lik[~nan])) and np.all(lik[~nan] >= 0), (what, lik)
    site = _site(np.where(nan, 1.0, lik), sc)
    ninf = np.isneginf(want_site)
    assert np.array_equal(np.isneginf(site), ninf), (what, "-inf patterns", np.flatnonzero(np.isneginf(site) != ninf))
    fin = np.isfinite(want_site)
    dev = np.abs(site[fin] - want_site[fin])
    worst = float(np.max(dev / (RTOL * np.abs(want_site[fin]) + ATOL))) if fin.any() else 0.0
    assert worst <= 1.0, (what, worst, int(np.argmax(dev)))
    if math.isnan(want_total):
        assert math.isnan(ll), (what, ll)
    elif want_total == -math.inf:
        assert ll == -math.inf, (what, ll)
    else:
        assert abs(ll - want_total) <= RTOL * abs(want_total) + ATOL, (what, ll, want_total)
    return worst


def hold_exact(what, got, freq, want_total, combiner, extra=0.0, floor_at=()):
    """(b)  ``want_total``: only its kind (NaN, -inf, finite) is used.  ``extra``: added to the allowance (the host's combine of shard
    sums).  ``floor_at``: patterns that category mode floors: they contribute exactly -1e6 f instead of a logarithm."""
    ll, lik, sc = got
    if math.isnan(want_total):
        assert math.isnan(ll), (what, ll)
        return 0.0
    if want_total == -math.inf:
        assert ll == -math.inf, (what, ll)
        return 0.0
    f = np.array(freq, dtype=np.int64)
    floored = 0
    for s in floor_at:
        assert lik[s] == 0.0, (what, "a floored pattern has likelihood 0", s, lik[s])
        floored += -1000000 * int(f[s])
        f[s] = 0
    live = f > 0
    assert np.all(np.isfinite(lik[live])) and np.all(lik[live] > 0), (what, "a live pattern without a finite positive likelihood")
    want, allow, cnt = rc.exact_sum(lik, sc, f)
    want = want + np.longdouble(floored)
    allow += rc.FACTOR * rc.U * abs(floored) + extra
    ratio = abs(float(np.longdouble(ll) - want)) / allow
    print(f"RATIO {combiner}: {ratio:.3f} of the allowance ({what}; log-L {ll!r}, sum f c = {cnt})")
    if ratio > WORST.get(combiner, (-1.0, ""))[0]:
        WORST[combiner] = (ratio, what)
    assert ratio <= 1.0, (what, ratio, ll, float(want), allow)
    return ratio


def check(what, part, got, cs, want, form, combiner=None):
    """The form that ran, then (a) and (b)."""
    assert part.reduce_form() == form, (what, part.reduce_form(), form)
    site, total = want
    hold_reference(what, got, site, total, cs["pattern_freq"])
    return hold_exact(what, got, cs["pattern_freq"], total, combiner or form.split(" n=")[0].split(" S_pad=")[0])


def run_passes(cs, form, passes=2, forms_before=None, expect_kernel=None, combiner=None):
    """``passes`` full passes on a fresh partition (the first persists, the others are lazy), each held both ways.  ``form``: what
    every pass must report — or, with ``forms_before``, what the LAST one must, the earlier ones being allowed those too (forms that
    only steady-state passes take)."""
    want = rc.expected(cs)
    with mk(cs) as part:
        assert part.reduce_form() == ""
        for k in range(passes):
            got = full(cs, part)
            want_form = form
            if forms_before and k < passes - 1 and part.reduce_form() in forms_before:
                want_form = part.reduce_form()
            check(f"{cs['name']} pass {k} [{part.prune_kernel_name()}]", part, got, cs, want, want_form, combiner)
        if expect_kernel:
            assert part.prune_kernel_name() == expect_kernel, (part.prune_kernel_name(), part.schedule_info())
    return got


CHILD_VARIANTS = ("plain", "heavy", "minus_inf@last", "nan@last", "minus_inf@first", "both", "both_r", "freq0")


def main(argv):
    form, D, n = argv[0], int(argv[1]), int(argv[2])
    assert os.environ.get("HYPHY_HIP_REDUCE") == form
    done = []
    for S in rc.sizes_for(D, n):
        for v in CHILD_VARIANTS:
            if v == "heavy" and not 63 <= n <= 4097:       # (outside: the count sum leaves the stated range)
                continue
            if v in ("minus_inf@first", "both", "both_r", "freq0") and S < 8:
                continue
            cs = rc.make(D, S, v)
            assert cs["n"] == n
            run_passes(cs, f"{form} n={n}")
            done.append(cs["name"])
    print("RESULT " + json.dumps({"cases": done, "worst": {k: v[0] for k, v in WORST.items()}}))
    return 0


def run_child(form, D, n, timeout=240):
    """A fresh process for one value of the switch; (exit status, whole output, the RESULT record or None).  Nothing is retried."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HYPHY_HIP_REDUCE=form)
    r = subprocess.run([sys.executable, "-m", "tests.reduce_child", form, str(D), str(n)], env=env, cwd=root, capture_output=True, text=True,
                       timeout=timeout)
    rec = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    return r.returncode, r.stdout + r.stderr, json.loads(rec[-1]) if rec else None


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
