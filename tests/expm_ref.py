"""An accurate reference for the matrix-exponential kernels (hyphy_amd/csrc/expm.hip, expm4.h), the cases on which they can go
wrong, and what each case is allowed.

Reference.  ``reference(Q)`` is ``tests/sitefit_ref.transition(Q, extended=True)``: uniformisation with non-negative terms only, in
80-bit arithmetic, pinned entry by entry to mpmath at 50 digits (tests/test_sitefit_ref_cpu.py, tests/test_expm_ref_cpu.py).  It
shares nothing with the kernels' Taylor-and-squaring scheme, which oracle.expm restates.  For mixtures the reference is
sum_m w_m reference(Q_m).

Cases.  ``cases()`` is a fixed, named, seeded list, enumerated in ``_enumerate`` and filtered nowhere else:

  state counts  2, 3, 4, 5, 15, 16, 17, 20, 31, 32, 33, 47, 48, 49, 61, 63, 64 (both sides of every row-block boundary)
  families      rev (S pi, dense), mg94 (MG94xREV, 61 states: the benchmark's matrix), nonrev (random, not reversible), chain
                (tridiagonal), blocks (two dense blocks, exact zeros between them), absorb (the last state has a zero row), stiff
                (one row's rate 1e3 times the others'), zero
  norms         every family at 0.2 (no squarings) and 3 (four squarings), neighbours in the list; at the LADDER state counts the
                rev family (and mg94) at 1e-9, 1e-6, either side of 1/64, 0.11 and 1/4, 0.4, 0.8, 6, 40, 700 (1, 2, 5, 8, 12
                squarings) and 400 (11 squarings: the squaring loop leaves early on a stationary matrix); stiff and chain at 40
                (20 and 61 states); rev at 61 states either side of 1/4 in the norm of expm_mfma_kernel<4,2>

A case is scaled so that the norm THE KERNEL THAT SERVES ITS STATE COUNT uses equals the target: the infinity norm at 49-64 states
(expm64_kernel), sqrt(||.||_1 ||.||_inf) below (expm_mfma_kernel, expm4.h).  ``plan(Q, kernel)`` restates in numpy each kernel's
choice of squaring count and Taylor degree; ``kernel_for`` restates launch_expm's dispatch; ``coverage`` lists the cells
(kernel, degree, squarings or none) the list reaches — tests/test_expm_ref_cpu.py asserts that none is empty.  With squarings the
scaled norm lies in (1/8, 1/4], so the degree is 12: degrees 6 and 9 exist only without squarings.

At 49-64 states the kernel (1, 2 or 4 workgroups per matrix) follows from the batch size and the device's compute units:
``batches(names, cus)`` deals the state count's cases into batches of every kind.  p = 0 and p > 0 cases alternate in the list, so
in the panel kernels panels 1 .. H-1 retire for a matrix and work for its neighbour.

Allowance.  Absolute, per entry: BAR_NO_SQUARING = 2e-15 where the kernel needs no squaring, BAR_SQUARING = 5e-14 where it needs
some (the project's existing bars).  For a case on which oracle.expm (dense path) itself deviates from the reference by more than
half its bar the allowance is ORACLE_FACTOR = 2 times the deviation recorded in ORACLE_DEV: the matrix cores sum in a different
order from the oracle, each of the two may sit on either side of the reference.  ORACLE_DEV is measured by
tests/test_expm_ref_cpu.py::test_oracle_deviation_is_the_recorded_one (which fails when a record is missing, too small, or more than
10 % too large); every case not named there deviates by at most half its bar.  Largest over the list: 2.4e-13 (mg94_D61_n700).
The sparse path (used by the project at 61 states) deviates less than the dense one on every mg94 case (same test).

ORACLE_FAILS names the cases on which the oracle fails outright; they are not built (their seeds stay used up).
"""
import functools
import math

import numpy as np

from tests import sitefit_ref as sr

BAR_NO_SQUARING = 2e-15
BAR_SQUARING = 5e-14
ORACLE_FACTOR = 2.0     # allowance = ORACLE_FACTOR * ORACLE_DEV[name] where the oracle itself is further than half the bar away
ROW_SUM_TOL = 1e-14

STATE_COUNTS = (2, 3, 4, 5, 15, 16, 17, 20, 31, 32, 33, 47, 48, 49, 61, 63, 64)
LADDER_STATE_COUNTS = (4, 5, 20, 33, 49, 61, 64)
EDGE = 1e-6             # "just below / just above" a threshold: a factor 1 -+ EDGE (the norms are sums of <= 64 terms: 1e-14 apart at most)
LADDER = (("1em9", 1e-9), ("1em6", 1e-6), ("b64", (1 - EDGE) / 64), ("a64", (1 + EDGE) / 64), ("b011", 0.11 * (1 - EDGE)),
          ("a011", 0.11 * (1 + EDGE)), ("b025", 0.25 * (1 - EDGE)), ("a025", 0.25 * (1 + EDGE)), ("0p4", 0.4), ("0p8", 0.8), ("6", 6.0),
          ("40", 40.0), ("700", 700.0), ("400", 400.0))
PAIR = (("0p2", 0.2), ("3", 3.0))
FAMILIES = ("rev", "nonrev", "chain", "blocks", "absorb", "stiff")

# name -> largest |oracle.expm(Q, dense) - reference(Q)| where that exceeds half the case's bar (rounded up to two digits)
ORACLE_DEV = {
    "rev_D4_n700": 5.1e-14,   # 5.078e-14 measured
    "rev_D4_n400": 9.8e-14,   # 9.709e-14 measured
    "rev_D5_n400": 7.9e-14,   # 7.860e-14 measured
    "rev_D20_n400": 9.6e-14,   # 9.536e-14 measured
    "rev_D33_n40": 2.8e-14,   # 2.764e-14 measured
    "rev_D33_n400": 6.0e-14,   # 5.926e-14 measured
    "rev_D49_n40": 4.1e-14,   # 4.038e-14 measured
    "rev_D49_n700": 1.3e-13,   # 1.229e-13 measured
    "rev_D49_n400": 4.4e-14,   # 4.344e-14 measured
    "mg94_D61_n40": 4.4e-14,   # 4.369e-14 measured
    "mg94_D61_n700": 2.4e-13,   # 2.388e-13 measured
    "mg94_D61_n400": 7.2e-14,   # 7.118e-14 measured
    "rev_D61_n700": 7.6e-14,   # 7.554e-14 measured
    "rev_D61_n400": 5.1e-14,   # 5.088e-14 measured
    "rev_D64_n700": 9.4e-14,   # 9.352e-14 measured
    "rev_D64_n400": 3.4e-14,   # 3.345e-14 measured
    "chain_D61_n40": 4.8e-14,   # 4.773e-14 measured
}

# cases on which oracle.expm fails outright (FloatingPointError), with the reason; none so far
ORACLE_FAILS = frozenset()

KERNELS = ("expm_nuc_kernel", "expm_mfma_kernel<1,1>", "expm_mfma_kernel<2,2>", "expm_mfma_kernel<3,1>", "expm_mfma_kernel<4,2>",
           "expm64_kernel<1>", "expm64_kernel<2>", "expm64_kernel<4>")


def reference(Q):
    return sr.transition(Q, extended=True)


# ---- what the kernels decide, restated ----------------------------------------------------------------------------------------------

def norm_inf(Q):
    return float(np.abs(Q).sum(axis=1).max())


def norm_geo(Q):
    return math.sqrt(float(np.abs(Q).sum(axis=1).max()) * float(np.abs(Q).sum(axis=0).max()))


def uses_inf_norm(kernel):
    return kernel.startswith("expm64_kernel")


def kernel_norm(Q, kernel):
    return norm_inf(Q) if uses_inf_norm(kernel) else norm_geo(Q)


def plan(Q, kernel, fixed_degree=False):
    """(squarings p, Taylor degree) the kernel takes for Q: p = ilogb(4 norm) + 1 when 4 norm > 1; the degree 6 / 9 / 12 by the
    scaled norm (<= 1/64, <= 0.11, above) in expm64_kernel and expm4.h, always 12 in expm_mfma_kernel."""
    nm = kernel_norm(Q, kernel)
    p = 0
    if 4.0 * nm > 1.0:
        p = math.frexp(4.0 * nm)[1]          # 4 nm = m 2^e, m in [0.5, 1): ilogb = e - 1
    if kernel.startswith("expm_mfma_kernel") or fixed_degree:
        return p, 12
    sn = nm * 2.0 ** -p
    return p, (6 if sn <= 0.015625 else (9 if sn <= 0.11 else 12))


def default_kernel(D):
    """The kernel hip.expm_batch reaches at D states under the default dispatch (49-64 states: one of expm64_kernel<H>)."""
    if D == 4:
        return "expm_nuc_kernel"
    return ("expm_mfma_kernel<1,1>", "expm_mfma_kernel<2,2>", "expm_mfma_kernel<3,1>", "expm64_kernel<4>")[(D + 15) // 16 - 1]


def kernel_for(D, n, cus, mode=-1, images=False):
    """launch_expm's choice for a batch of n rate matrices at D states on a device of ``cus`` compute units; ``mode`` is
    HYPHY_HIP_EXPM; ``images``: the launch writes the pruning kernels' images (a partition above 4 states)."""
    if D == 4 and not images:
        return "expm_nuc_kernel"
    nt = (D + 15) // 16
    if nt < 4:
        return ("expm_mfma_kernel<1,1>", "expm_mfma_kernel<2,2>", "expm_mfma_kernel<3,1>")[nt - 1]
    if mode == 0:
        return "expm_mfma_kernel<4,2>"
    H = 4 if 4 * n <= cus else (2 if 2 * n <= cus else 1)
    if mode in (1, 2, 4):
        H = mode
    return f"expm64_kernel<{H}>"


def kernels_at(D):
    """Every kernel a case at D states is run under by tests/test_gpu_expm.py."""
    if D < 49:
        return (default_kernel(D),)
    return ("expm64_kernel<4>", "expm64_kernel<2>", "expm64_kernel<1>", "expm_mfma_kernel<4,2>")


def _fit(names, lo, hi):
    """Lists of more than lo and at most hi names that cover ``names``, each filled up by going round its own part again."""
    out = []
    for k in range(0, len(names), hi):
        part = list(names[k:k + hi])
        full = list(part)
        while len(full) <= lo:
            full.append(part[(len(full) - len(part)) % len(part)])
        out.append(full)
    return out


def batches(names, cus):
    """[(H, names of one hip.expm_batch call)] at 49-64 states: n <= cus/4 (H = 4), cus/4 < n <= cus/2 (H = 2), n > cus/2 (H = 1);
    8-64, 100 and 140 matrices on 256 compute units."""
    out = [(4, b) for b in _fit(names, 0, max(1, cus // 4))]
    n2 = min(cus // 2, cus // 4 + max(1, (cus * 36) // 256))
    out += [(2, b) for b in _fit(names, n2 - 1, cus // 2)]
    n1 = cus // 2 + max(1, (cus * 12) // 256)
    out += [(1, b) for b in _fit(names, n1 - 1, max(n1, len(names)))]
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def _set_diagonal(Q):
    idx = np.arange(Q.shape[0])
    Q[idx, idx] = 0.0
    Q[idx, idx] = -Q.sum(axis=1)
    return Q


def _family(family, D, rng):
    if family == "rev":
        S = rng.uniform(0.1, 1.0, size=(D, D))
        S = S + S.T
        pi = rng.random(D) + 0.2
        Q = S * (pi / pi.sum())[None, :]
    elif family == "mg94":
        from hyphy_amd import models
        assert D == 61
        Q = models.mg94rev_Q(1.0, 0.7, {k: v for k, v in sr.REV.items() if k != "AG"}, sr.POS_FREQS)
    elif family == "nonrev":
        Q = rng.random((D, D)) * rng.uniform(0.2, 1.0, size=(D, 1))
    elif family == "chain":
        Q = np.zeros((D, D))
        k = np.arange(D - 1)
        Q[k, k + 1] = rng.uniform(0.3, 1.0, size=D - 1)
        Q[k + 1, k] = rng.uniform(0.3, 1.0, size=D - 1)
    elif family == "blocks":
        h = D // 2
        Q = rng.uniform(0.1, 1.0, size=(D, D))
        Q[:h, h:] = 0.0
        Q[h:, :h] = 0.0
    elif family == "absorb":
        Q = rng.random((D, D)) * rng.uniform(0.2, 1.0, size=(D, 1))
        Q[D - 1, :] = 0.0
    elif family == "stiff":
        Q = rng.uniform(0.1, 1.0, size=(D, D))
        Q[D // 2, :] *= 1e3
    else:
        raise ValueError(family)
    return _set_diagonal(np.array(Q, dtype=np.float64))


def _enumerate():
    seed = 0
    for D in STATE_COUNTS:
        kern = default_kernel(D)
        fams = [f for f in FAMILIES if not (f == "blocks" and D < 4)]   # (two blocks of one state: the zero matrix)
        plans = [(f, PAIR) for f in fams]
        if D == 61:
            plans.append(("mg94", PAIR + LADDER))
        if D in LADDER_STATE_COUNTS:
            plans.append(("rev", LADDER))
        for family, norms in plans:
            seed += 1
            base = _family(family, D, np.random.default_rng(7100 + seed))
            n0 = kernel_norm(base, kern)
            for tag, target in norms:
                name = f"{family}_D{D}_n{tag}"
                if name in ORACLE_FAILS:
                    continue
                yield dict(name=name, D=D, family=family, target=target, norm_kernel=kern, Q=_set_diagonal(base * (target / n0)))
        yield dict(name=f"zero_D{D}", D=D, family="zero", target=0.0, norm_kernel=kern, Q=np.zeros((D, D)))
    # -- beyond the grid (seeds of their own, so that the cases above stay what they are)
    # a stiff and a chain matrix at a large norm (eight squarings)
    for k, (D, family) in enumerate(((20, "stiff"), (20, "chain"), (61, "stiff"), (61, "chain"))):
        kern = default_kernel(D)
        base = _family(family, D, np.random.default_rng(7900 + k))
        name = f"{family}_D{D}_n40"
        if name not in ORACLE_FAILS:
            yield dict(name=name, D=D, family=family, target=40.0, norm_kernel=kern, Q=_set_diagonal(base * (40.0 / kernel_norm(base, kern))))
    # either side of 1/4 in the norm of expm_mfma_kernel<4,2> (HYPHY_HIP_EXPM=0), sqrt(||.||_1 ||.||_inf): the 49-64-state cases above
    # are scaled in the infinity norm of expm64_kernel
    base = _family("rev", 61, np.random.default_rng(7950))
    for tag, target in LADDER[6:8]:
        yield dict(name=f"rev_D61_g{tag}", D=61, family="rev", target=target, norm_kernel="expm_mfma_kernel<4,2>",
                   Q=_set_diagonal(base * (target / norm_geo(base))))


@functools.lru_cache(maxsize=None)
def _cases():
    cs = list(_enumerate())
    for c in cs:
        c["Q"].setflags(write=False)
    assert len({c["name"] for c in cs}) == len(cs)
    return tuple(cs)


def cases():
    return list(_cases())


def cases_by_name():
    return {c["name"]: c for c in _cases()}


def cases_at(D):
    return [c for c in _cases() if c["D"] == D]


@functools.lru_cache(maxsize=None)
def _reference_of(name):
    P = reference(cases_by_name()[name]["Q"])
    P.setflags(write=False)
    return P


def case_reference(name):
    """reference(Q) of a case, computed once per process and shared (read-only)."""
    return _reference_of(name)


def bar(p):
    return BAR_NO_SQUARING if p == 0 else BAR_SQUARING


def allowance(name, kernel, fixed_degree=False):
    """Absolute allowance per entry of case ``name`` under ``kernel``: the bar of the squarings that kernel needs, or
    ORACLE_FACTOR times the oracle's own recorded deviation where that exceeds half the bar."""
    p, _ = plan(cases_by_name()[name]["Q"], kernel, fixed_degree)
    b = bar(p)
    dev = ORACLE_DEV.get(name, 0.0)
    return ORACLE_FACTOR * dev if dev > 0.5 * b else b


def coverage():
    """{(kernel, degree, 'none' | 'some'): [case names]} over the list, every kernel a case is run under."""
    cells = {}
    for c in _cases():
        for kern in kernels_at(c["D"]):
            p, deg = plan(c["Q"], kern)
            cells.setdefault((kern, deg, "none" if p == 0 else "some"), []).append(c["name"])
    return cells


def required_cells():
    """Every cell a kernel has: degrees 6 / 9 / 12 without squarings where the kernel chooses a degree, 12 with squarings."""
    out = []
    for kern in KERNELS:
        degrees = (12,) if kern.startswith("expm_mfma_kernel") else (6, 9, 12)
        out += [(kern, d, "none") for d in degrees] + [(kern, 12, "some")]
    return out
