"""The comparison every GPU test against tests/scalefree.py uses (test_gpu_rescale.py, test_gpu_branchcache.py): per pattern
``log(lik) - 64 ln2 sc`` and the total at scalefree.GPU_RTOL x |reference| plus the absolute 1e-9 of tests/test_gpu_parity.py, -inf
exactly where the reference has it, exponents integral and bounded."""
import numpy as np

from tests import scalefree as sf

RTOL = sf.GPU_RTOL
ATOL = 1e-9
LOG_SCALER = sf.LOG_SCALER


def _site(lik, sc):
    with np.errstate(divide="ignore"):
        return np.log(lik) - sc * LOG_SCALER


def miss(site, want_site):
    """Largest per-pattern deviation / allowance of ``_hold`` (inf where -inf sits in other places): the figure ``_hold`` prints."""
    if not np.array_equal(np.isneginf(site), np.isneginf(want_site)):
        return np.inf
    fin = np.isfinite(want_site)
    return float(np.max(np.abs(site[fin] - want_site[fin]) / (RTOL * np.abs(want_site[fin]) + ATOL))) if fin.any() else 0.0


def hold_download(what, cache, counts, want_cond, want_log_mag):
    """``download_partials`` of one class against the reference's ``cond`` and ``log_mag``: conditionals divided by their largest element,
    and the counts consistent with the values: log(largest element) - 64 ln2 count = the reference's log-magnitude."""
    top = cache.max(axis=2)
    zero = ~(want_cond.max(axis=2) > 0)
    assert np.array_equal(top == 0, zero), what
    norm = cache / np.where(top > 0, top, 1.0)[:, :, None]
    assert np.allclose(norm, want_cond, rtol=1e-9, atol=1e-12), what
    with np.errstate(divide="ignore"):
        mag = np.log(top) - LOG_SCALER * counts
    ok = ~zero
    assert np.all(np.abs(mag[ok] - want_log_mag[ok]) <= RTOL * np.abs(want_log_mag[ok]) + ATOL), what


def _hold(what, got, want_site, want_total):
    """got = (log-L, likelihoods, exponents) of an evaluation with per_site=True."""
    ll, lik, sc = got
    assert sc.dtype == np.int64 and np.all(np.abs(sc) < 4096), (what, sc)
    assert np.all(np.isfinite(lik)) and np.all(lik >= 0), (what, lik)
    site = _site(lik, sc)
    assert np.array_equal(np.isneginf(site), np.isneginf(want_site)), (what, np.flatnonzero(np.isneginf(site) != np.isneginf(want_site)))
    fin = np.isfinite(want_site)
    dev = np.abs(site[fin] - want_site[fin])
    worst = float(np.max(dev / (RTOL * np.abs(want_site[fin]) + ATOL))) if fin.any() else 0.0
    print(f"{what}: largest per-pattern deviation / allowance = {worst:.3f}; log-L {ll!r} against {want_total!r}")
    assert worst <= 1.0, (what, worst, int(np.argmax(dev)))
    if np.isneginf(want_total):
        assert ll == -np.inf, (what, ll)
    else:
        assert abs(ll - want_total) <= RTOL * abs(want_total) + ATOL, (what, ll, want_total)
