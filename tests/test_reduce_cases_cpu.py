"""What tests/reduce_cases.py promises, asserted on the scale-free reference alone (no device): the partial counts, the share of
patterns that need an exponent, the range of the heavy count sums, the place of the special patterns, and that a plain float64 model
of the reduction stays within half the allowance the GPU tests give the device.

Pattern order: the special patterns are placed in the caller's order, which is the device's because the wide-state GPU tests run with
HYPHY_HIP_SORT_PATTERNS=0 and 4-state patterns are never sorted (tests/reduce_cases.py says where)."""
import math

import numpy as np
import pytest

from tests import reduce_cases as rc

_LISTS = [(5, rc.WIDE5_N), (61, rc.WIDE61_N), (4, rc.FOUR_N)]
# the sizes whose reference is cheap enough for a CPU test that runs with every pull request (the largest: D = 5, S = 16 * 4097)
_SIZES = [(D, S, v) for D, ns in _LISTS for (S, v) in rc.size_list(D, [n for n in ns if rc.width(D) * n <= 70000])]
_SIZES += [(61, 16 * n, "plain") for n in (500, 540)]      # (around 2 x the compute units of the devices the suite meets)


def test_case_names_carry_their_partial_count():
    for D, ns in _LISTS:
        for n in ns:
            for S in rc.sizes_for(D, n):
                assert rc.n_partials(D, S) == n, (D, n, S)
                assert (S - 1) // rc.width(D) == n - 1, "the last partial holds a real pattern"
    for sp in rc.SITE_S_PAD:
        assert rc.n_partials(5, sp) * 16 == sp
    assert all(n % 2 == 0 for n in rc.FOUR_N), "4 states: the pattern count is padded to 512, two workgroups"
    cs = rc.make(5, 16 * 513 - 9, "plain")
    assert cs["n"] == 513 and cs["name"] == "D5_n513_S8199_plain"


def test_wave_k_is_the_first_entry_of_the_last_non_empty_wave():
    for n in (2048, 2049, 2050, 2561, 4096, 4097):
        chunk = ((n + 7) // 8 + 511) // 512 * 512
        k = rc.wave_k_partial(n)
        assert k % chunk == 0 and k < n <= k + chunk
    assert rc.wave_k_partial(4097) == 4096 and rc.wave_k_partial(4096) == 3584 and rc.wave_k_partial(2049) == 2048


@pytest.mark.parametrize("D,S,variant", _SIZES, ids=lambda x: str(x))
def test_case_keeps_its_promises(D, S, variant):
    cs = rc.make(D, S, variant)
    site, total = rc.expected(cs)
    f, sp, w = cs["pattern_freq"], cs["special"], rc.width(D)
    kind, _, pos = variant.partition("@")
    # the special patterns: where the name says, and what the name says
    ordinary = np.ones(S, dtype=bool)
    for key in ("minus_inf", "nan"):
        if sp[key] is not None:
            ordinary[sp[key]] = False
    assert np.all(np.isfinite(site[ordinary])), "all other patterns are finite"
    if sp["minus_inf"] is not None:
        assert site[sp["minus_inf"]] == -np.inf, "the reference finds the pattern impossible"
    if sp["nan"] is not None:
        assert np.isnan(cs["ambig"][2]).any() and cs["leaf_codes"][0, sp["nan"]] == -3
        assert not np.any(cs["leaf_codes"][:, ordinary] == -3)
    want_partial = {"first": 0, "last": cs["n"] - 1, "wave_k": rc.wave_k_partial(cs["n"])}
    if kind in ("minus_inf", "nan"):
        assert sp[kind] // w == want_partial[pos]
    if kind == "both":
        assert sp["minus_inf"] // w == 0 and sp["nan"] // w == cs["n"] - 1
    if kind in ("both_r", "freq0"):
        assert sp["nan"] // w == 0 and sp["minus_inf"] // w == cs["n"] - 1
    # the expected total
    if kind in ("nan", "both", "both_r"):
        assert math.isnan(total)
    elif kind == "minus_inf":
        assert total == -math.inf
    else:
        assert math.isfinite(total)
    if kind == "freq0":
        assert f[sp["nan"]] == 0 and f[sp["minus_inf"]] == 0 and np.all(f[ordinary] > 0)
    # exponents: at least a quarter of the patterns of a plain / heavy case lie below 2^-64, so their exponent is >= 1
    lik, c = rc.model_inputs(np.where(ordinary, site, 0.0))
    if kind in ("plain", "heavy"):
        assert np.mean(site < -rc.LOG_SCALER) >= 0.25, np.mean(site < -rc.LOG_SCALER)
        assert np.all(c[site < -rc.LOG_SCALER] >= 1) and np.any(c == 0)
    # a float64 model of the reduction against the exact sum of the same inputs: within half the allowance
    live = np.where(ordinary, f, 0)
    want, allow, cnt = rc.exact_sum(lik, c, live)
    got = rc.float64_model(lik, c, live)
    ratio = abs(float(np.longdouble(got) - want)) / allow
    assert ratio <= 0.5, (ratio, got, float(want))
    if kind == "heavy":
        assert 2 ** 33 < cnt < 2 ** 44, math.log2(cnt)
    if kind not in ("nan", "both", "both_r", "minus_inf"):   # the exact sum of the model inputs is the reference's total
        assert abs(float(want) - total) <= 1e-12 * abs(total)


def test_host_exchange_propagates_nan_and_minus_infinity():
    """hyphy_hip_xch_open / _sum / _close (comm.hip, host only): three ranks, one of them carrying NaN -> NaN on every rank; one
    carrying -inf -> -inf; finite shard totals -> their sum to 2 x 2^-53 of the summed magnitudes, the same bits on every rank."""
    import os
    import threading
    from hyphy_amd import hip
    hip.load()
    world = 3
    rounds = [(-1234.5678, float("nan"), -99.25), (-1234.5678, float("-inf"), -99.25), (-1.0e9 - 0.125, -3.0e-7, -4.5e3 + 2.0 ** -20),
              (float("nan"), float("-inf"), -1.0)]
    got = [[None] * len(rounds) for _ in range(world)]
    errors = []
    tag = f"reduce_cases_{os.getpid()}"

    def rank(r):
        try:
            x = hip.HostExchange(tag, r, world)
            for k, vals in enumerate(rounds):
                got[r][k] = x.sum(vals[r])
            x.close()
        except Exception as e:       # noqa: BLE001 (reported below, in the test's own thread)
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for r in range(world):
        assert math.isnan(got[r][0]) and got[r][1] == -math.inf and math.isnan(got[r][3]), got[r]
        want = math.fsum(rounds[2])
        assert abs(got[r][2] - want) <= 2 * rc.U * sum(abs(v) for v in rounds[2]), (got[r][2], want)
        assert got[r][2] == got[0][2]
