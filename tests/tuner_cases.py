"""The cases tests/test_gpu_tuner_forms.py runs every form of the schedule tuner on: five of their own next to the members of
tests/scalefree.py's list that have 49 to 64 states and two to five tiles, and the one call sequence all of those tests share.

Four of the new cases hang from an end of the tree (a caterpillar, on its own or on a small balanced tree), so that a re-rooted
schedule differs from the given one; the fifth is the generator's balanced three-class case, the control.  They are built with the
generator's own helpers but not by ``scalefree._enumerate_cases``, whose seeds run on.  tests/test_tuner_cases_cpu.py holds the CPU
oracle to ``scalefree.case_reference`` on them (within scalefree.ORACLE_MAX_REL, which is not raised for them) and checks that each
has a pattern three steps of 2^64 down, a re-rooting path and chain schedules at the cuts the GPU tests force.

    name                    D   tree                                          matrices                                   S
    cat24_on_k4d2_D61       61  ladder of 24 on balanced (4, 2): 40 taxa      near-identity 1e-15                        70
    cat16_on_k2d3_D64       64  ladder of 16 on balanced (2, 3): 24 taxa      near-identity 1e-10                        53
    cat40_D61_1em6          61  ladder of 40                                  near-identity 1e-6, every third ordinary   70
    cat12_on_k2d3_D61_cls   61  ladder of 12 on balanced (2, 3): 20 taxa      three classes 1e-2 / 1e-12 / 1e-30         40
    classes_D61_k2          61  balanced (2, 6)                               three classes, from the generator          24

(A four-way hang at 1e-30 is beyond the reference's own scheme, as scalefree.py notes: the class case hangs from a binary tree.)
"""
import numpy as np

from tests import scalefree as sf

WEIGHTS = np.array([0.5, 0.3, 0.2])
CLASS_EPS = (1e-2, 1e-12, 1e-30)


def _new_cases():
    out = []

    def add(i, name, D, n, hang, S, make_P, **extra):
        rng = np.random.default_rng(9500 + i)
        fp, L = sf.ladder_tree(n, hang)
        codes = sf._patterns(rng, L, D, S, 4)
        out.append(sf._case(name, D, fp, L, codes, make_P(rng, len(fp) - 1, D), rng, **extra))

    add(0, "cat24_on_k4d2_D61", 61, 24, (4, 2), 70, lambda rng, B, D: sf.near_identity(rng, B, D, 1e-15))
    add(1, "cat16_on_k2d3_D64", 64, 16, (2, 3), 53, lambda rng, B, D: sf.near_identity(rng, B, D, 1e-10))

    def third_ordinary(rng, B, D):
        P = sf.near_identity(rng, B, D, 1e-6)
        P[::3] = sf.ordinary(rng, len(P[::3]), D)
        return P
    add(2, "cat40_D61_1em6", 61, 40, None, 70, third_ordinary)
    add(3, "cat12_on_k2d3_D61_cls", 61, 12, (2, 3), 40,
        lambda rng, B, D: np.stack([sf.near_identity(rng, B, D, e, spread=D * e < 0.3) for e in CLASS_EPS]), weights=WEIGHTS.copy())
    return out


NEW = tuple(c["name"] for c in _new_cases())
UNBALANCED_NEW = NEW                                   # (every new case hangs from an end; the control comes from the generator)
CONTROL = "classes_D61_k2"
CLASS_CASES = ("cat12_on_k2d3_D61_cls", CONTROL)
# the members of the generator's list that run next to them: 49-64 states of scalefree.SUBSET, and the kinds it has none of
EXISTING = tuple(n for n in sf.SUBSET if "_D61_" in n or "_D64_" in n) + (
    "mixed_D64_k3_1em10_S41", "star_D61_n10_1em7", "threshold_D61_below", "threshold_D61_above", "ladder_D61_120_on_k4d3")

_cases = None


def cases_by_name():
    """{name: case} of the new cases, the control and EXISTING (built once)."""
    global _cases
    if _cases is None:
        gen = sf.cases_by_name()
        _cases = {c["name"]: c for c in _new_cases()}
        _cases.update({n: gen[n] for n in (CONTROL,) + EXISTING})
    return _cases


def single_class(cs, c=2):
    """A class case as a one-class case under the matrices of class ``c`` (default: the 1e-30 class); other cases as they are."""
    if cs["P"].ndim == 3:
        return cs
    out = {k: v for k, v in cs.items() if k != "weights"}
    out["P"] = cs["P"][c]
    return out


def other_data(cs, seed):
    """The same tree and pattern count under other leaf data and matrices (what a second partition of an analysis looks like)."""
    rng = np.random.default_rng(seed)
    D, L, S = int(cs["D"]), int(cs["L"]), cs["leaf_codes"].shape[1]
    P = sf.near_identity(rng, len(cs["flat_parents"]) - 1, D, 1e-12)
    return sf._case(cs["name"] + "_other", D, cs["flat_parents"], L, sf._patterns(rng, L, D, S, 4), P, rng)


def reroot_path(cs):
    """Internal indices from the given root to the node the re-rooted schedules hang the tree from (empty: balanced)."""
    from hyphy_amd import hip
    return [int(x) for x in hip.plan_reroot(cs["flat_parents"], int(cs["L"]))]


def inner_nodes(cs):
    """Node codes (update, pin, branch cache) of three internal branches: the middle, the second and the last node of the re-rooting
    path — on a tree without one the first node above internal nodes (the first internal node where that is the root), for all three."""
    L = int(cs["L"])
    path = reroot_path(cs)
    if len(path) >= 3:
        return L + path[len(path) // 2], L + path[1], L + path[-1]
    ch = sf.children_of(cs["flat_parents"], L)
    second = next(i for i in range(len(ch)) if any(c >= L for c in ch[i]))
    return (L + (second if second < len(ch) - 1 else 0),) * 3


class Scenario:
    """The matrices, nodes and references of the one call sequence (test_gpu_tuner_forms.py) on a one-class case; every reference
    is computed once, when first asked for."""

    def __init__(self, cs):
        self.cs = cs
        D = int(cs["D"])
        rng = np.random.default_rng(4242)
        self.leaf = 1
        self.inner, self.pin, self.bc = inner_nodes(cs)
        P0 = cs["P"]
        e = float(P0[self.leaf][0, 1])
        P1 = P0.copy()
        P1[self.leaf] = sf.near_identity(rng, 1, D, min(e * 3.0, 0.1 / D) if e > 0 else 1e-12)[0]
        e = float(P0[self.inner][0, 1])
        P2 = P1.copy()
        P2[self.inner] = sf.near_identity(rng, 1, D, min(e * 3.0, 0.1 / D) if e > 0 else 1e-12)[0]
        P3 = P2.copy()
        P3[self.bc] = sf.near_identity(rng, 1, D, 1e-7)[0]
        self.P = (P0, P1, P2, P3)
        S = cs["leaf_codes"].shape[1]
        self.states = ((np.arange(S) * 5 + 1) % D).astype(np.int64)
        self._refs = {}

    def ref(self, step):
        """step: 0..3 = under P[step]; "pin" = P[2] with the pinned node; "pin0" = P[0] with it; "cond" = P[2] with conditionals."""
        if step not in self._refs:
            k = {"pin": 2, "pin0": 0, "cond": 2}.get(step, step)
            cs = dict(self.cs, P=self.P[k])
            kw = {}
            if step in ("pin", "pin0"):
                kw["pinned"] = (self.pin, self.states)
            if step == "cond":
                kw["conditionals"] = True
            self._refs[step] = sf.case_reference(cs, **kw)
        return self._refs[step]


_scenarios = {}


def scenario(name):
    """The Scenario of a case of cases_by_name() (a class case: under its 1e-30 class), built once per process."""
    if name not in _scenarios:
        _scenarios[name] = Scenario(single_class(cases_by_name()[name]))
    return _scenarios[name]
