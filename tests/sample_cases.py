"""Inputs and checks shared by tests/test_sample_cpu.py and tests/test_gpu_sample.py."""
import functools

import numpy as np

from tests import common
from tests import expm_ref as er
from tests import sample_ref as sr
from tests import scalefree as sf
from tests.test_gpu_joint import BAL8, make_case

# ---- the distribution check: D = 20, BAL8, S = 8, R = 4096, fixed seed --------------------------------------------------------
DIST_R, DIST_SEED = 4096, 20240611


def dist_case():
    return make_case(20, BAL8, 8, 2008)


def distribution_violations(states, post, R):
    """[(node, pattern, state, f, p)] where the sampled frequency f of a state misses |f - p| <= 5 sqrt(p (1 - p) / R) + 2 / R.
    ``states``: [R, I, S] (site = pattern), ``post``: [I, S, D] marginal posteriors."""
    I, S, D = post.shape
    assert states.shape == (R, I, S)
    bad = []
    for i in range(D):
        f = (states == i).mean(axis=0)
        p = post[:, :, i]
        miss = ~(np.abs(f - p) <= 5.0 * np.sqrt(p * (1.0 - p) / R) + 2.0 / R)
        bad += [(int(n), int(s), i, float(f[n, s]), float(p[n, s])) for n, s in np.argwhere(miss)]
    return bad


# ---- the scale-free tier: rate matrices, deep trees --------------------------------------------------------------------------
NEAR_TOL = 1e-9          # a column is left out when some node on it has |cum_i - u total| <= NEAR_TOL total for some i
MAX_LEFT_OUT = 1e-3      # ... and at most this share of the columns may be
SCALEFREE = {"codon61": (61, 40, 24, 64, 611), "nuc4": (4, 120, 40, 40, 41)}   # D, leaves of the caterpillar, S, replicates, seed


@functools.lru_cache(maxsize=None)
def scalefree_case(name):
    """(case with "Q", reference transition matrices, scale-free conditionals [I, S, D]), computed once per process."""
    D, n, S, R, seed = SCALEFREE[name]
    rng = np.random.default_rng(seed)
    fp, L = sf.ladder_tree(n)
    B = len(fp) - 1
    pi = rng.random(D) + 0.05
    cs = sf._case(name, D, fp, L, sf._patterns(rng, L, D, S, 2), None, rng, root_freqs=pi / pi.sum())
    cs["Q"] = common.random_rates(rng, B, D)
    P = np.stack([er.reference(q) for q in cs["Q"]])
    cs["P"] = P
    cond = sf.case_reference(cs, conditionals=True)["cond"]
    for a in (cs["Q"], P, cond):
        a.setflags(write=False)
    return cs, P, cond, R, seed


def scalefree_reference(name):
    """(states, near-tie mask [R, S]) of sample_ref on the scale-free conditionals under the Philox uniforms of the case's seed."""
    cs, P, cond, R, seed = scalefree_case(name)
    I = len(cs["flat_parents"]) - int(cs["L"])
    u = sr.uniforms(seed, R, I, cond.shape[1])
    return sr.sample_ref(cs["flat_parents"], cs["L"], cond, P, cs["root_freqs"], u, near_tol=NEAR_TOL)
