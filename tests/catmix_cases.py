"""Cases, a reference and an enclosure for rate classes over explicit-form mixtures (hyphy_hip_evaluate_categories_mixture and its
_built form): class c evolves on branch b under P_cb = sum_m w_cbm exp(Q_cbm), under the same component counts in every class, and
the classes are mixed by class weights.  Host only.

Everything is built from tests/mixture_cases.py: the cases with ``_mk``, class c's components as ``Scenario(cs, cls=c)`` draws them,
the matrices and their allowances with ``matrices`` (``built_extra`` included for components built on the device).

Reference.  scalefree.prune with P [C, B, D, D] and the class weights.

Enclosure.  The same reference at the lower and upper ends of EVERY class's matrices, the allowance of a component being that of
the exponential kernel ``mixture_cases.kernel_for(cs, n, cus)`` names for the n components of the call that uploaded it: C x n_tot
for a batched call (all classes share one launch), the one-class total for a one-class call.  The mixed likelihood of a pattern is
sum_c w_c L_c with w_c >= 0, and every L_c is non-decreasing in every entry of class c's matrices, so the mixed likelihood is
non-decreasing in every entry of every class's matrices: the argument of mixture_cases.py carries over, and the mixed width is at
most the largest per-class width.  tests/test_catmix_cases_cpu.py holds hi - lo below mixture_cases.WIDTH_BAR for every pattern of
every case and step.

Cases (``cases()``; fixed, named, seeded):

    cm_ladder_D{4,20,33,61,64}_C3   8 leaves, 40 patterns, COUNT_PATTERN (49 components per class): every state count
    cm_classes_D61_C2               98 components: the batched launch runs expm64_kernel<2> where a one-class call runs <4>
    cm_deep_D61_40_C3               40-leaf ladder, short branches, 24 patterns: the 2^64 rescale, exponents that differ between classes
    cm_rep_D61_C2                   every pattern twice: the class-compressed form
    cm_poly12_D20_C8                POLY12, SMALL_PATTERN: many classes
    cm_built2_D20_C2                templates K = 2; 2 x 29 x 2 = 116 coefficients
    cm_built2_D61_C2                100 rows per class: 2 x 100 x 2 = 400 coefficients, ON the inline limit (kCoefInline)
    cm_built3_D61_C3                46 rows per class: 3 x 46 x 3 = 414, above it (the partial updates of the sequence are below)

``CatScenario`` is the one call sequence every form runs (tests/test_gpu_catmix.py):

    1, 2   full batched passes (persisting, lazy)                                   state[1]
    3      batched partial update of leaf branch ``leaf``: 3 -> 16 components in every class        state[3]
    4      the same branch, 16 -> 1                                                 state[4]
    5      batched partial update of the internal branch ``inner`` on the re-rooting path: 5 new components per class   state[5]
    6      a ONE-class evaluate_mixture(cat=1) partial update of ``nxt``, the next branch on that path: ref("cls1") is class 1's own
           enclosure; then a batched call without matrices                          state[6]
    7      a batched call without matrices under NEW class weights                  ref(7)
    8      download_partials(cat=1)                                                 ref("cond")
    9      two last full batched passes                                             state[9]
"""
import functools

import numpy as np

from tests import mixture_cases as mc
from tests import scalefree as sf

WIDTH_BAR = mc.WIDTH_BAR
CLASS_WEIGHT_CASES = {"zero": (0.6, 0.0, 0.4), "skewed": (0.98, 0.015, 0.005)}   # one weight exactly 0; far from uniform


def _enumerate():
    k = 0

    def seed():
        nonlocal k
        k += 1
        return 47000 + k
    for D in (4, 20, 33, 61, 64):
        yield mc._mk(f"cm_ladder_D{D}_C3", seed(), D, sf.ladder_tree(8), C=3)
    yield mc._mk("cm_classes_D61_C2", seed(), 61, sf.ladder_tree(8), C=2)
    yield mc._mk("cm_deep_D61_40_C3", seed(), 61, sf.ladder_tree(40), S=24, deep=True, C=3)
    yield mc._mk("cm_rep_D61_C2", seed(), 61, sf.ladder_tree(8), C=2, twice=True)
    yield mc._mk("cm_poly12_D20_C8", seed(), 20, mc._poly12(), C=8, counts=mc.SMALL_PATTERN)
    yield mc._mk("cm_built2_D20_C2", seed(), 20, sf.ladder_tree(8), K=2, C=2, counts=mc.SMALL_PATTERN)
    yield mc._mk("cm_built2_D61_C2", seed(), 61, sf.ladder_tree(8), K=2, C=2, counts=(3,) + (16,) * 5 + (3,) + (2,) * 7)
    yield mc._mk("cm_built3_D61_C3", seed(), 61, sf.ladder_tree(8), K=3, C=3, counts=(3,) + (16,) * 2 + (1,) * 11)


@functools.lru_cache(maxsize=None)
def _cases():
    cs = list(_enumerate())
    assert len({c["name"] for c in cs}) == len(cs)
    return tuple(cs)


def cases():
    return list(_cases())


def cases_by_name():
    return {c["name"]: c for c in _cases()}


def names(pred=lambda c: True):
    return [c["name"] for c in _cases() if pred(c)]


def class_weights(C):
    """The class weights of steps 1 - 6 and 8, 9: (C, C - 1, ..., 1) / their sum."""
    w = np.arange(C, 0, -1, dtype=np.float64)
    return w / w.sum()


def new_class_weights(C):
    """... and of step 7: the same in reverse."""
    return class_weights(C)[::-1].copy()


def enclosure(cs, states, weights):
    """{"lo", "mid", "hi"} [S] per pattern of the MIXED likelihood, the totals, "width" = hi - lo; ``states``: one state per class."""
    per = [mc.matrices(st) for st in states]
    P = np.stack([p[0] for p in per])
    al = np.stack([p[1] for p in per]).astype(np.longdouble)[:, :, None, None]
    U = mc.U
    ends = {"lo": np.maximum(P - al, 0).astype(np.float64) * (1.0 - 2 * U), "mid": P.astype(np.float64), "hi": (P + al).astype(np.float64) * (1.0 + 2 * U)}
    out = {}
    freq = np.asarray(cs["pattern_freq"], dtype=np.float64)
    for key, M in ends.items():
        r = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], M, cs["root_freqs"], weights=weights)
        out[key] = r["site_logl"]
        out[key + "_total"] = float(np.sum(r["site_logl"] * freq))
        if key == "mid":
            out["class_site_logl"] = r["class_site_logl"]
    out["width"] = out["hi"] - out["lo"]
    return out


class CatScenario:
    """States and nodes of the sequence on one case.  ``state[k][c]``: every branch's components of class c after step k, each marked
    with the kernel of the call that uploaded it; ``ref(k)``: the enclosure under it, computed once."""

    def __init__(self, cs, cus=mc.CUS):
        self.cs, self.cus = cs, cus
        C = self.C = int(cs["C"])
        per = [mc.Scenario(cs, c, cus) for c in range(C)]
        one = per[0]
        self.nodes, self.leaf, self.inner, self.nxt, self.path = one.nodes, one.leaf, one.inner, one.nxt, one.path
        self.w, self.w_new = class_weights(C), new_class_weights(C)
        built = bool(cs["K"])

        def batched(prev, branches, new):
            """``prev`` with ``new[c][k]`` on branch ``branches[k]`` of class c, under the kernel of ONE launch for all classes."""
            kern = mc.kernel_for(cs, C * sum(len(b.w) for b in new[0]), cus)
            out = [list(st) for st in prev]
            for c in range(C):
                assert [len(b.w) for b in new[c]] == [len(b.w) for b in new[0]]
                for b, br in zip(branches, new[c]):
                    out[c][int(b)] = br.under(kern, built)
            return out

        B = len(self.nodes)
        st = {}
        st[1] = batched([[None] * B for _ in range(C)], self.nodes, [[per[c].state[1][b] for b in range(B)] for c in range(C)])
        st[3] = batched(st[1], [self.leaf], [[per[c].state[3][self.leaf]] for c in range(C)])
        st[4] = batched(st[3], [self.leaf], [[per[c].state[4][self.leaf]] for c in range(C)])
        st[5] = batched(st[4], [self.inner], [[per[c].state[5][self.inner]] for c in range(C)])
        # step 6: class 1 alone, new components under the count the branch has in every class (the counts stay shared)
        self.single = mc.draw_branch(cs, np.random.default_rng([int(cs["seed"]), 11]), len(st[5][1][self.nxt].w))
        st[6] = [list(x) for x in st[5]]
        st[6][1][self.nxt] = self.single.under(mc.kernel_for(cs, len(self.single.w), cus), built)
        st[9] = batched(st[6], self.nodes, [[st[6][c][b] for b in range(B)] for c in range(C)])
        st[2] = st[1]
        self.state = st
        self._refs = {}

    def ref(self, step):
        step = {2: 1}.get(step, step)
        if step not in self._refs:
            if step == 7:
                r = enclosure(self.cs, self.state[6], self.w_new)
            elif step == "cls1":
                r = mc.enclosure(self.cs, self.state[6][1])
            elif step == "cond":
                r = mc.enclosure(self.cs, self.state[6][1], conditionals=True)
            else:
                r = enclosure(self.cs, self.state[step], self.w)
            self._refs[step] = r
        return self._refs[step]

    def steps(self):
        return [1, 3, 4, 5, 6, 7, "cls1", 9]

    def dense(self, step, branches):
        """(per-class list of per-branch [M, D, D] rate matrices, per-class list of per-branch weights) of ``branches`` under state[step]."""
        got = [mc.dense_input(self.cs, [self.state[step][c][int(b)] for b in branches]) for c in range(self.C)]
        return [g[0] for g in got], [g[1] for g in got]

    def built(self, step, branches):
        """... with coefficient rows [M, K] in place of the matrices."""
        got = [mc.built_input(self.cs, [self.state[step][c][int(b)] for b in branches]) for c in range(self.C)]
        return [g[0] for g in got], [g[1] for g in got]

    def n_tot(self, step, branches):
        return sum(len(self.state[step][0][int(b)].w) for b in branches)


_scenarios = {}


def scenario(name, cus=mc.CUS):
    key = (name, cus)
    if key not in _scenarios:
        _scenarios[key] = CatScenario(cases_by_name()[name], cus)
    return _scenarios[key]
