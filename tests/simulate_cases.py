"""Cases shared by tests/test_simulate_cpu.py and tests/test_gpu_simulate.py: rate matrices through the device's exponential, the
reference on P from tests/expm_ref.py.  Everything is seeded, computed once per process and read-only.

A case's rate matrices are Q_b = c_b0 T_0 + c_b1 T_1 (off the diagonal; the diagonal minus the row sum) over two non-negative
templates, so one set of reference exponentials serves the plain form (Q uploaded), the template form (Q built on the device from T
and c: another rounding of Q, 1e-16 relative, nothing next to the near-tie margin) and the mixture (components Q_b and Q_{b-1}).

Near ties.  A column is left out of the comparison when, at some node, |cum_i - u total| <= NEAR_TOL total for some i: there the
device's exponential (allowed 5e-14 per entry, tests/expm_ref.py, D entries per running sum: 3e-12) may land on the other side of u.
Expected share of such columns: about (L + I) D 2 NEAR_TOL, 1e-5 at 61 states on the 40-leaf caterpillar; the cap is 1e-3."""
import functools

import numpy as np

from tests import expm_ref as er
from tests import scalefree as sf
from tests import simulate_ref as mr

MAX_LEFT_OUT = 1e-3
NEAR_TOL = 1e-9
DIST_SEED = 7                   # tests/test_simulate_cpu.py::test_reference_leaf_patterns_follow_the_model notes its statistic
EXPM_CASES = {"cat40_D61": (61, 40), "cat40_D64": (64, 40), "cat120_D4": (4, 120)}
EXPM_R, EXPM_SITES, EXPM_SEED = 2, 700, 31


def reference_P(Q):
    out = np.stack([er.reference(q) for q in np.asarray(Q).reshape((-1,) + Q.shape[-2:])]).reshape(Q.shape)
    out.setflags(write=False)
    return out


def build_Q(T, coeffs):
    Q = np.tensordot(coeffs, T, axes=(1, 0))
    idx = np.arange(Q.shape[-1])
    Q[:, idx, idx] = 0.0
    Q[:, idx, idx] = -Q.sum(axis=2)
    return Q


@functools.lru_cache(maxsize=None)
def expm_case(name):
    D, L = EXPM_CASES[name]
    rng = np.random.default_rng(1000 + D + L)
    fp, L = sf.ladder_tree(L)
    B = len(fp) - 1
    T = rng.random((2, D, D)) * (rng.random((2, D, D)) < 0.6)
    T[:, np.arange(D), np.arange(D)] = 0.0
    coeffs = rng.uniform(0.02, 0.5, size=(B, 2)) / D
    Q = build_Q(T, coeffs)
    pi = rng.random(D) + 0.05
    cs = dict(D=D, L=L, B=B, flat_parents=fp, leaf_codes=rng.integers(0, D, size=(L, 24)), ambig=None,
              pattern_freq=np.ones(24, dtype=np.int64), T=T, coeffs=coeffs, Q=Q, root_freqs=pi / pi.sum(), P=reference_P(Q))
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def reference(cs, P, seed=EXPM_SEED, n_rep=EXPM_R, n_sites=EXPM_SITES):
    """(states [n_rep, L + I, n_sites], near [n_rep, n_sites]) of simulate_ref under Philox."""
    rows = len(cs["flat_parents"])
    return mr.simulate_ref(cs["flat_parents"], cs["L"], P, cs["root_freqs"], mr.uniforms(seed, n_rep, rows, n_sites), near_tol=NEAR_TOL)


@functools.lru_cache(maxsize=None)
def expm_reference(name):
    cs = expm_case(name)
    return reference(cs, cs["P"])


@functools.lru_cache(maxsize=None)
def mixture_of(name):
    """(q_components [B, 2, D, D], weights [B, 2], P = sum_m w_m exp(Q_m)) with the second component the neighbour's matrix."""
    cs = expm_case(name)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.2, 0.8, size=(cs["B"], 1))
    w = np.concatenate([w, 1.0 - w], axis=1)
    comp = np.stack([cs["Q"], np.roll(cs["Q"], 1, axis=0)], axis=1)
    P = w[:, 0, None, None] * cs["P"] + w[:, 1, None, None] * np.roll(cs["P"], 1, axis=0)
    return comp, w, P


def changed(cs, branches, seed):
    """Q and its reference P with new matrices on ``branches`` (other coefficients over the same templates)."""
    rng = np.random.default_rng(seed)
    co = np.array(cs["coeffs"])
    co[branches] = rng.uniform(0.02, 0.5, size=(len(branches), 2)) / cs["D"]
    Q = build_Q(cs["T"], co)
    P = np.array(cs["P"])
    P[branches] = reference_P(Q[branches])
    return Q, P
