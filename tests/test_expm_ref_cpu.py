"""tests/expm_ref.py checked on the CPU: the reference against 50-digit arithmetic, oracle.expm against the reference on every case
(the recorded deviations the GPU allowances are built from), and that the case list reaches every branch of every kernel."""
import math

import numpy as np
import pytest

from tests import expm_ref as er
from tests import sitefit_ref as sr

CASES = er.cases()
NAMES = [c["name"] for c in CASES]
FRAC = 260      # fractional bits of the fixed-point evaluation (78 digits)


def _mp_expm(Q):
    """Taylor series of exp(Q / 2^s) in mpmath at 50 digits, squared s times."""
    import mpmath as mp
    mp.mp.dps = 50
    D = Q.shape[0]
    A = mp.matrix(D, D)
    for i in range(D):
        for j in range(D):
            A[i, j] = mp.mpf(float(Q[i, j]))
    s = max(0, int(math.ceil(math.log2(max(er.norm_inf(Q), 1e-300)))) + 2)
    A = A / mp.mpf(2) ** s
    E = mp.eye(D)
    term = mp.eye(D)
    for j in range(1, 60):
        term = term * A / j
        E = E + term
    for _ in range(s):
        E = E * E
    return np.array([[E[i, j] for j in range(D)] for i in range(D)], dtype=object)


def _fixed_expm(Q, exact_diagonal=False):
    """The same in integer fixed point with FRAC fractional bits (numpy object arrays of Python integers: a 61 x 61 product at 78
    digits in 15 ms, where mpmath takes a second); held to mpmath at 50 digits by test_fixed_point_evaluation_is_mpmath_to_50_digits.
    Returns Python integers: value * 2^FRAC."""
    D = Q.shape[0]
    one = 1 << FRAC

    def to_fixed(x):
        m, e = math.frexp(float(x))
        return (int(m * (1 << 53)) << (FRAC + e - 53)) if FRAC + e - 53 >= 0 else (int(m * (1 << 53)) >> -(FRAC + e - 53))

    s = max(0, int(math.ceil(math.log2(max(er.norm_inf(Q), 1e-300)))) + 2)
    A = np.array([[to_fixed(Q[i, j]) for j in range(D)] for i in range(D)], dtype=object)
    if exact_diagonal:      # what the reference exponentiates: the diagonal is minus the EXACT sum of the row's other entries
        for i in range(D):
            A[i, i] = 0
            A[i, i] = -sum(A[i, :])
    A = A >> s
    eye = np.array([[one if i == j else 0 for j in range(D)] for i in range(D)], dtype=object)
    E, term = eye.copy(), eye.copy()
    for j in range(1, 60):
        term = (term.dot(A) >> FRAC) // j
        E = E + term
    for _ in range(s):
        E = E.dot(E) >> FRAC
    return E


def _fixed_to_float(E):
    return np.array([[int(v) / (1 << FRAC) for v in row] for row in E], dtype=np.float64)   # (int / int: correctly rounded)


@pytest.mark.parametrize("name", [n for n, c in zip(NAMES, CASES) if c["D"] <= 5 and c["target"] <= 40.0])
def test_fixed_point_evaluation_is_mpmath_to_50_digits(name):
    import mpmath as mp
    mp.mp.dps = 60
    Q = er.cases_by_name()[name]["Q"]
    E, M = _fixed_expm(Q), _mp_expm(Q)
    worst = max(abs(mp.mpf(int(E[i, j])) / mp.mpf(2) ** FRAC - M[i, j]) for i in range(Q.shape[0]) for j in range(Q.shape[0]))
    assert worst < mp.mpf(10) ** -45, (name, worst)


def _mp_expm_exact_diagonal(Q, terms=40):
    """exp(Q) in mpmath numbers at 50 digits (numpy object arrays of mpf), the diagonal minus the exact sum of the row's other
    entries — what the reference exponentiates: Taylor series of the matrix over 2^s (norm <= 1/4), squared s times."""
    import mpmath as mp
    mp.mp.dps = 50
    D = Q.shape[0]
    A = np.array([[mp.mpf(float(Q[i, j])) if i != j else mp.mpf(0) for j in range(D)] for i in range(D)], dtype=object)
    for i in range(D):
        A[i, i] = -sum(A[i, :], mp.mpf(0))
    s = max(0, int(math.ceil(math.log2(max(er.norm_inf(Q), 1e-300)))) + 2)
    A = A / mp.mpf(2) ** s
    eye = np.array([[mp.mpf(1 if i == j else 0) for j in range(D)] for i in range(D)], dtype=object)
    E, term = eye.copy(), eye.copy()
    for j in range(1, terms):
        term = term.dot(A) / mp.mpf(j)
        E = E + term
    for _ in range(s):
        E = E.dot(E)
    return E


@pytest.mark.parametrize("name", ["nonrev_D20_n3", "stiff_D20_n40", "rev_D20_n700", "mg94_D61_n3"])
def test_fixed_point_with_the_exact_diagonal_is_mpmath_at_20_and_61_states(name):
    """The form the pin below uses (exact_diagonal=True), directly against mpmath at the sizes the pin reaches; the 61-state case
    takes ten seconds of mpmath products."""
    import mpmath as mp
    Q = er.cases_by_name()[name]["Q"]
    E, M = _fixed_expm(Q, exact_diagonal=True), _mp_expm_exact_diagonal(Q)
    mp.mp.dps = 60
    D = Q.shape[0]
    worst = max(abs(mp.mpf(int(E[i, j])) / mp.mpf(2) ** FRAC - M[i, j]) for i in range(D) for j in range(D))
    assert worst < mp.mpf(10) ** -40, (name, worst)


PINNED = [n for n, c in zip(NAMES, CASES) if c["D"] <= 20] + ["mg94_D61_n3"]


@pytest.mark.parametrize("name", PINNED)
def test_reference_matches_50_digit_arithmetic_entry_by_entry(name):
    """Every entry, relatively: within the rounding of the float64 result plus the bound sitefit_ref states for the arithmetic
    (transition_bound, with the 80-bit format's rounding unit); exact zeros where the graph has no path."""
    Q = er.cases_by_name()[name]["Q"]
    ref = er.case_reference(name)
    hp = _fixed_to_float(_fixed_expm(Q, exact_diagonal=True))
    D = Q.shape[0]
    mu = float(np.abs(np.diag(Q)).max())
    rel = 2.0 ** -52 + sr.transition_bound(D, mu, terms=60) * (float(np.finfo(np.longdouble).eps) / 2.0) / 2.0 ** -53
    dev = np.abs(ref - hp)
    print(f"{name}: largest absolute deviation {dev.max():.3g}, relative bound {rel:.3g}")
    assert np.all(dev <= rel * np.abs(hp) + 1e-300), (name, float(dev.max()))
    assert np.array_equal(ref == 0.0, hp == 0.0)
    # sharp enough to judge the bars: a tenth of them at the most
    p = min(er.plan(Q, k)[0] for k in er.kernels_at(D))
    assert dev.max() <= 0.1 * er.bar(p) + 2.0 ** -53, (name, float(dev.max()))


def _oracle_dev(name, sparse):
    from oracle import oracle
    return float(np.abs(oracle.expm(er.cases_by_name()[name]["Q"], sparse) - er.case_reference(name)).max())


def test_oracle_deviation_is_the_recorded_one():
    """oracle.expm (dense path) against the reference on every case: at most half the case's smallest bar unless ORACLE_DEV records
    more, and a record is what is measured (not below it, at most 10 % above).  The sparse path, which the project uses at 61
    states, deviates no more than the dense one's allowance on the mg94 cases."""
    worst = ("", 0.0)
    for c in CASES:
        name = c["name"]
        dev = _oracle_dev(name, False)
        if dev > worst[1]:
            worst = (name, dev)
        b = min(er.bar(er.plan(c["Q"], k)[0]) for k in er.kernels_at(c["D"]))
        if name in er.ORACLE_DEV:
            assert dev <= er.ORACLE_DEV[name] <= 1.1 * dev and dev > 0.5 * b, (name, dev, er.ORACLE_DEV[name])
        else:
            assert dev <= 0.5 * b, (name, dev, b)
        if c["family"] == "mg94":
            sp = _oracle_dev(name, True)
            assert sp <= max(er.allowance(name, k) for k in er.kernels_at(61)), (name, sp)
    print(f"largest oracle deviation: {worst[1]:.3g} ({worst[0]})")
    assert set(er.ORACLE_DEV) <= set(NAMES) and not er.ORACLE_FAILS & set(NAMES)


def test_allowance_is_the_bar_or_twice_the_recorded_deviation():
    for c in CASES:
        for kern in er.kernels_at(c["D"]):
            p, _ = er.plan(c["Q"], kern)
            a = er.allowance(c["name"], kern)
            dev = er.ORACLE_DEV.get(c["name"], 0.0)
            assert a == (2.0 * dev if dev > 0.5 * er.bar(p) else er.bar(p))
            assert a <= 10 * er.BAR_SQUARING      # (the largest: mg94_D61_n700, 4.8e-13, a stationary matrix after 12 squarings)


def test_case_list_reaches_every_cell_of_every_kernel():
    """(kernel template) x (degree 6 / 9 / 12 where the kernel chooses) x (no squarings / some), from the numpy restatement of each
    kernel's choice: no cell is empty, with the ORACLE_FAILS cases already taken out."""
    assert len(set(NAMES)) == len(NAMES)
    assert {c["D"] for c in CASES} == set(er.STATE_COUNTS)
    cov = er.coverage()
    for cell in er.required_cells():
        assert cov.get(cell), cell
    assert set(k for k, _, _ in cov) == set(er.KERNELS)
    # degrees 6 and 9 never meet squarings: the scaled norm of a squared case lies in (1/8, 1/4]
    assert all(deg == 12 for (_, deg, sq) in cov if sq == "some")
    # the squaring counts the list asks for, in the norm of the kernel that serves the state count
    for D in er.LADDER_STATE_COUNTS:
        ps = {er.plan(c["Q"], er.default_kernel(D))[0] for c in er.cases_at(D)}
        assert ps >= {0, 1, 2, 4, 5, 8, 11, 12}, (D, ps)
    for c in CASES:
        if c["family"] != "zero":
            nm = er.kernel_norm(c["Q"], c["norm_kernel"])
            assert abs(nm - c["target"]) <= 1e-12 * c["target"], c["name"]
            assert c["Q"][~np.eye(c["D"], dtype=bool)].min() >= 0 and np.abs(c["Q"].sum(axis=1)).max() <= 1e-13 * max(1.0, c["target"])


def test_thresholds_are_straddled():
    for D in er.LADDER_STATE_COUNTS:
        kern = er.default_kernel(D)
        by = {c["name"].rsplit("_n", 1)[1]: er.plan(c["Q"], kern) for c in er.cases_at(D) if c["family"] == "rev" and "_n" in c["name"]}
        deg_kernel = not kern.startswith("expm_mfma_kernel")
        assert by["b64"] == (0, 6 if deg_kernel else 12) and by["a64"] == (0, 9 if deg_kernel else 12)
        assert by["b011"] == (0, 9 if deg_kernel else 12) and by["a011"] == (0, 12)
        assert by["b025"] == (0, 12) and by["a025"] == (1, 12)
    # expm_mfma_kernel<4,2> in its own norm (the infinity norm of these two is not what decides there)
    by = er.cases_by_name()
    assert er.plan(by["rev_D61_gb025"]["Q"], "expm_mfma_kernel<4,2>") == (0, 12)
    assert er.plan(by["rev_D61_ga025"]["Q"], "expm_mfma_kernel<4,2>") == (1, 12)


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_batches_reach_every_panel_count(cus):
    """Every 49-64-state case is in a batch of every kind, the batch sizes give the panel count launch_expm derives from them, and
    matrices without squarings sit next to matrices with some."""
    for D in (49, 61, 63, 64):
        names = [c["name"] for c in er.cases_at(D)]
        seen = {1: set(), 2: set(), 4: set()}
        for H, batch in er.batches(names, cus):
            assert er.kernel_for(D, len(batch), cus) == f"expm64_kernel<{H}>", (D, H, len(batch), cus)
            seen[H] |= set(batch)
            ps = [er.plan(er.cases_by_name()[n]["Q"], f"expm64_kernel<{H}>")[0] for n in batch]
            assert any((a == 0) != (b == 0) for a, b in zip(ps, ps[1:])), (D, H)
        assert all(seen[H] == set(names) for H in seen), (D, cus)


def test_dispatch_restatement():
    assert er.kernel_for(4, 10, 256) == "expm_nuc_kernel" and er.kernel_for(4, 10, 256, images=True) == "expm_mfma_kernel<1,1>"
    assert [er.kernel_for(D, 1, 256) for D in (2, 16, 17, 32, 33, 48, 49, 64)] == [
        "expm_mfma_kernel<1,1>", "expm_mfma_kernel<1,1>", "expm_mfma_kernel<2,2>", "expm_mfma_kernel<2,2>", "expm_mfma_kernel<3,1>",
        "expm_mfma_kernel<3,1>", "expm64_kernel<4>", "expm64_kernel<4>"]
    assert [er.kernel_for(61, n, 256) for n in (64, 65, 128, 129)] == ["expm64_kernel<4>", "expm64_kernel<2>", "expm64_kernel<2>", "expm64_kernel<1>"]
    assert er.kernel_for(61, 8, 256, mode=0) == "expm_mfma_kernel<4,2>" and er.kernel_for(61, 8, 256, mode=1) == "expm64_kernel<1>"
    assert er.kernel_for(61, 200, 256, mode=4) == "expm64_kernel<4>"
