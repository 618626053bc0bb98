"""Cases for the last step of every evaluation: per-pattern values (l_s, c_s) -> log L = sum_s f_s log l_s - 64 ln2 sum_s f_s c_s.

Host only and deterministic.  A case is named by the number of partial sums ``n`` it hands the combiner, not by its pattern count:

* wide states (D = 5, 61) with HYPHY_HIP_TILES=1: one partial per tile of 16 patterns, n = ceil(S / 16);
* 4 states: one partial per workgroup of 256 patterns, over a pattern count padded to a multiple of 512 (api.hip: ``S_pad``), so
  n = 2 ceil(S / 512) — always EVEN.  The odd counts 1, 65, 513 and 2049 cannot be reached with 4 states; FOUR_N holds their even
  neighbours 2, 66, 514 and 2050 next to 512 and 2048.

Every case is the 8-leaf balanced binary tree with near-identity matrices whose off-diagonal entries are 1e-30 on every other PAIR of sibling
branches and 1e-3 on the rest, made block-zero (tests/scalefree.py ``_block_zero``: the last state is cut off from the others).  Ordinary
patterns use the other states only, so all of them are possible; conserved ones keep exponent 0 and patterns with several conflicts
need c_s >= 1.  The patterns of a case need not be distinct.

Pattern ORDER: the special patterns are placed by position in the caller's order.  The wide-state GPU tests run with
HYPHY_HIP_SORT_PATTERNS=0 and the library never sorts 4-state patterns (api.hip: ``!p->nuc && sw::sort_patterns()``), so the caller's
order is the device's, and partial k holds patterns [k w, (k + 1) w) with w = 16 or 256.

Variants (``make(D, S, variant)``):
  plain                 frequencies 1..3
  heavy                 frequencies from [2^26, 2^30] (S <= 8208) or [2^26, 2^27] (larger S: the narrower draw keeps the sum below
                        2^44), so that sum f_s c_s lies in (2^33, 2^44): beyond int32, exactly representable in a double
  minus_inf@POS         one impossible pattern (the cut-off state at leaf 0, other states elsewhere)
  nan@POS               one pattern whose leaf 0 refers to an ambiguity vector that contains NaN
  both                  minus_inf@first and nan@last; NaN wins
  both_r                nan@first and minus_inf@last
  freq0                 nan@first and minus_inf@last, both with frequency 0: the total is the finite sum over the others
POS: ``first`` (partial 0), ``last`` (partial n - 1: the last real pattern), ``wave_k`` (n >= 2048: the first entry of the last
non-empty wave's range in multi_wave_reduce_kernel<8>, partial k chunk with chunk = ceil(ceil(n / 8) / 512) 512).
"""
import functools
import math

import numpy as np

from tests import scalefree as sf

LOG_SCALER = sf.LOG_SCALER
U = 2.0 ** -53
FACTOR = 8.0          # the allowance of the exact-sum comparison, in units of u relative to the summed terms (see allowance())

WIDE5_N = (1, 2, 63, 64, 65, 511, 512, 513, 1025, 2047, 2048, 2049, 2561, 4096, 4097)
WIDE61_N = (1, 2, 65, 511, 512, 513)
FOUR_N = (2, 66, 512, 514, 2048, 2050)
SITE_S_PAD = (16, 1008, 1024, 1040, 2048 + 16)


def width(D):
    return 256 if int(D) == 4 else 16


def n_partials(D, S):
    """Partials the pruning launch of a (D, S) partition leaves for the combiner (wide states: under HYPHY_HIP_TILES=1)."""
    return 2 * ((int(S) + 511) // 512) if int(D) == 4 else (int(S) + 15) // 16


def sizes_for(D, n):
    """The pattern counts that give ``n`` partials: all of them real, and a last partial that is mostly padding."""
    if int(D) == 4:
        assert n % 2 == 0
        return (256 * n, 256 * (n - 1) + 7)
    return (16 * n, 16 * n - 9)


def wave_k_partial(n, nwv=8):
    chunk = ((n + nwv - 1) // nwv + 511) // 512 * 512
    return (n - 1) // chunk * chunk


@functools.lru_cache(maxsize=None)
def _base(D, S):
    """Tree, matrices, frequencies of the root and ordinary patterns of the (D, S) cases; shared by the variants, never modified."""
    rng = np.random.default_rng(77000 + 1000 * D + S % 9973)
    fp, L = sf.balanced_tree(2, 3)
    B = len(fp) - 1
    eps = np.where(np.arange(B) // 2 % 2 == 0, 1e-30, 1e-3)           # sibling branches alike: a conflict in a 1e-30 cherry cannot dodge
    P = sf._block_zero(sf.near_identity(rng, B, D, eps), D)
    pi = rng.random(D) + 0.1
    pi /= pi.sum()
    ambig = (rng.random((2, D)) < 0.5).astype(np.float64)
    ambig[:, 0] = 1.0
    ambig[0, :] = 1.0
    ambig[1, D - 1] = 0.0                                  # (the cut-off state stays out of the ordinary patterns)
    m = D - 1                                              # ordinary states
    s = np.arange(S)
    j = np.arange(L)[:, None]
    kind = s % 4
    codes = rng.integers(0, m, size=(L, S))                # kind 3: random
    cons = rng.integers(0, m, size=S)
    codes = np.where(kind == 0, cons[None, :], codes)      # kind 0: conserved
    codes = np.where(kind == 1, (j + j // 2 + s[None, :]) % m, codes)     # kind 1: siblings differ
    k2 = (j * 7 + s[None, :]) % m                          # kind 2: with ambiguity codes
    amb = rng.random((L, S)) < 0.2
    k2 = np.where(amb, -rng.integers(1, 3, size=(L, S)), k2)
    codes = np.where(kind == 2, k2, codes).astype(np.int64)
    for a in (P, pi, ambig, codes):
        a.setflags(write=False)
    return dict(fp=fp, L=L, P=P, pi=pi, ambig=ambig, codes=codes, seed=77000 + 1000 * D + S % 9973)


@functools.lru_cache(maxsize=None)
def _base_site_logl(D, S):
    b = _base(D, S)
    out = sf.prune(D, b["fp"], b["L"], b["codes"], b["ambig"], np.ones(S), b["P"], b["pi"])["site_logl"]
    out.setflags(write=False)
    return out


def _position(D, S, pos):
    n, w = n_partials(D, S), width(D)
    if pos == "first":
        return min(3, S - 1)
    if pos == "last":
        assert (S - 1) // w == n - 1, "the last partial holds no real pattern"
        return S - 1
    if pos == "wave_k":
        assert n >= 2048
        return wave_k_partial(n) * w
    raise ValueError(pos)


def make(D, S, variant, at=None, zero=()):
    """One case: the golden fixtures' keys plus ``P`` (pass with q_is_probability=True), ``n`` and ``special``: a dict with the
    caller's index of the impossible pattern (``minus_inf``) and of the NaN pattern (``nan``), or None.  ``at``: explicit indices of
    the special patterns on top of a ``plain`` or ``heavy`` variant (the shard tests place them per shard); ``zero``: which of them
    get frequency 0."""
    D, S = int(D), int(S)
    b = _base(D, S)
    L = b["L"]
    rng = np.random.default_rng(b["seed"] + 17)
    freq = rng.integers(1, 4, size=S).astype(np.int64)
    codes, ambig = b["codes"], b["ambig"]
    special = dict(minus_inf=None, nan=None)
    kind, _, pos = variant.partition("@")
    if kind == "heavy":
        hi = 2 ** 30 if S <= 8208 else 2 ** 27
        freq = rng.integers(2 ** 26, hi + 1, size=S).astype(np.int64)
    elif kind == "minus_inf":
        special["minus_inf"] = _position(D, S, pos)
    elif kind == "nan":
        special["nan"] = _position(D, S, pos)
    elif kind == "both":
        special["minus_inf"], special["nan"] = _position(D, S, "first"), _position(D, S, "last")
    elif kind in ("both_r", "freq0"):
        special["nan"], special["minus_inf"] = _position(D, S, "first"), _position(D, S, "last")
    elif kind != "plain":
        raise ValueError(variant)
    if at:
        special.update(at)
    if special["minus_inf"] is not None or special["nan"] is not None:
        assert special["minus_inf"] != special["nan"], "one pattern cannot be both (S too small for this variant)"
        codes = codes.copy()
    if special["minus_inf"] is not None:
        s = special["minus_inf"]
        codes[:, s] = (np.arange(L) + s) % (D - 1)
        codes[0, s] = D - 1                                # the cut-off state next to the others: impossible
    if special["nan"] is not None:
        s = special["nan"]
        row = np.ones((1, D))
        row[0, 1] = np.nan
        ambig = np.concatenate([ambig, row])               # ambiguity vector 3 (code -3) carries a NaN
        codes[0, s] = -3
    if kind == "freq0":
        freq[[special["nan"], special["minus_inf"]]] = 0
    for key in zero:
        freq[special[key]] = 0
    if at:
        variant += "+" + ",".join(f"{k}@{v}{'(f=0)' if k in zero else ''}" for k, v in sorted(at.items()))
    return dict(name=f"D{D}_n{n_partials(D, S)}_S{S}_{variant}", D=np.int64(D), L=np.int64(L), flat_parents=b["fp"], leaf_codes=codes,
                ambig=ambig, pattern_freq=freq, root_freqs=b["pi"], P=b["P"], n=n_partials(D, S), special=special, variant=variant)


def expected(cs):
    """(per-pattern log-likelihood by the scale-free reference, expected log L).  The reference is asked about the impossible
    pattern (it must answer -inf) but not about the NaN pattern, which it has no notion of: that entry is NaN because the case says so.
    The total is NaN if a NaN pattern has positive frequency, else -inf if an impossible one has, else the sum over f > 0."""
    D, S = int(cs["D"]), cs["leaf_codes"].shape[1]
    site = np.array(_base_site_logl(D, S))
    sp = cs["special"]
    if sp["minus_inf"] is not None:
        s = sp["minus_inf"]
        site[s] = sf.prune(D, cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"][:2], np.ones(S), cs["P"], cs["root_freqs"],
                           patterns=[s])["site_logl"][0]
    if sp["nan"] is not None:
        site[sp["nan"]] = np.nan
    f = cs["pattern_freq"]
    live = f > 0
    if np.isnan(site[live]).any():
        total = float("nan")
    elif np.isneginf(site[live]).any():
        total = float("-inf")
    else:
        total = math.fsum((site[live] * f[live]).tolist())
    return site, total


# ---- the reduction alone: an exact sum of its own inputs --------------------------------------------------------------------------

def exact_sum(lik, sc, freq):
    """(want, allowance) of log L from the per-pattern (l_s, c_s) of one evaluation, over the patterns with f > 0 (all of which must
    have a finite positive l_s): logarithms and their sum in 80-bit extended precision (64-bit mantissa, asserted), the integer sum
    in Python ints.  allowance = 8 * 2^-53 * (sum |f_s log l_s| + 64 ln2 |sum f_s c_s|).
    Where the 8 comes from, in units of u = 2^-53 relative to the summed terms: a 1-ulp device logarithm 2, its rounded product with
    f 1, the compensated sum 2; on the count term the rounded constant, its product with the count and the final subtraction 1 each:
    about 5 on each part, 8 leaves a margin of 1.6.  Derived, not measured."""
    assert np.finfo(np.longdouble).nmant == 63, "np.longdouble is not the 80-bit extended type here"
    live = np.asarray(freq) > 0
    l = np.asarray(lik, dtype=np.float64)[live]
    assert np.all(np.isfinite(l)) and np.all(l > 0), "exact_sum: a live pattern without a finite positive likelihood"
    f = np.asarray(freq, dtype=np.int64)[live]
    c = np.asarray(sc, dtype=np.int64)[live]
    terms = np.log(l.astype(np.longdouble)) * f.astype(np.longdouble)
    cnt = sum(int(a) * int(b) for a, b in zip(f.tolist(), c.tolist()))
    log_scaler = np.longdouble(64) * np.log(np.longdouble(2))
    want = np.sum(terms) - log_scaler * np.longdouble(cnt)
    allow = FACTOR * U * (float(np.sum(np.abs(terms))) + LOG_SCALER * abs(cnt))
    return want, allow, cnt


def float64_model(lik, sc, freq):
    """The operation in plain float64: np.log in double, rounded products, math.fsum, then the two final operations in double."""
    live = np.asarray(freq) > 0
    l = np.asarray(lik, dtype=np.float64)[live]
    f = np.asarray(freq, dtype=np.int64)[live]
    c = np.asarray(sc, dtype=np.int64)[live]
    total = math.fsum((np.log(l) * f.astype(np.float64)).tolist())
    cnt = sum(int(a) * int(b) for a, b in zip(f.tolist(), c.tolist()))
    return total - LOG_SCALER * float(cnt)


def model_inputs(site_logl):
    """Per-pattern (l_s, c_s) as a kernel with the 2^64 rule could hand them over, from reference log-likelihoods: the smallest
    exponent that brings l_s to 2^-64 or above.  (Stands in for the device's outputs where there is no device.)"""
    site = np.asarray(site_logl, dtype=np.longdouble)
    fin = np.isfinite(site)
    c = np.zeros(len(site), dtype=np.int64)
    c[fin] = np.maximum(0, np.ceil(-np.asarray(site[fin], dtype=np.float64) / LOG_SCALER - 1.0)).astype(np.int64)
    log_scaler = np.longdouble(64) * np.log(np.longdouble(2))
    l = np.zeros(len(site))
    l[fin] = np.exp(site[fin] + log_scaler * c[fin].astype(np.longdouble)).astype(np.float64)
    return l, c


# ---- the lists the GPU tests run --------------------------------------------------------------------------------------------------

def variants_for(D, n):
    """Variants of the (D, n) size with all patterns real: plain everywhere; the specials where the combiner changes its path."""
    out = ["plain"]
    edge = n in (1, 2, 65, 66, 511, 512, 513, 514, 2047, 2048, 2049, 2050, 4096, 4097)
    if edge:
        out += ["minus_inf@last", "nan@last"]
    if n in (2, 65, 66, 513, 514, 2049, 2050, 4097):
        out += ["minus_inf@first", "both", "both_r", "freq0"]
    if n in (63, 65, 66, 513, 514) or (int(D) != 4 and n in (2049, 4097)):
        out += ["heavy"]
    if n >= 2048:
        out += ["minus_inf@wave_k", "nan@wave_k"]
    return out


def size_list(D, ns):
    """[(S, variant)] for the partial counts ``ns``: every variant at S with all patterns real, plain and the last-partial specials at
    the S whose last partial is mostly padding."""
    out = []
    for n in ns:
        full, ragged = sizes_for(D, n)
        out += [(full, v) for v in variants_for(D, n)]
        out += [(ragged, v) for v in variants_for(D, n) if v in ("plain", "minus_inf@last", "nan@last")]
    return out
