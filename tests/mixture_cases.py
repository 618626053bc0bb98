"""Cases, a reference and an enclosure for explicit-form mixtures (hyphy_hip_evaluate_mixture, hyphy_hip_evaluate_mixture_built):
on every branch P_b = sum_m w_bm exp(Q_bm), with a component count of its own per branch.  Host only.

Reference.  P_b = sum_m w_bm expm_ref.case_reference(name_bm), summed in np.longdouble, then scalefree.prune: the construction
tests/expm_ref.py names for mixtures.  It shares nothing with the kernels.

Components.  Every Q_bm is a named case of expm_ref.cases_by_name() at the case's state count, of a family whose exponential is
entrywise positive (rev, nonrev, stiff; mg94 at 61 states) and a norm of 0.2, 0.4, 0.8, 3 or 6.  The deep cases take norms of at most
1/4 only (0.2, and the rev ladder's entries either side of 0.11 and just below 1/4): no squaring, the 2e-15 allowance.  The first
component of a branch is a dense one (rev or nonrev): a stiff matrix has rows whose off-diagonal entries are 1e-6 of the others', and
an absolute allowance on such an entry alone would be a relative one of 1e-9.

Enclosure (in place of a hand-picked tolerance).  a_b = sum_m w_bm expm_ref.allowance(name_bm, kernel), the kernel being what
expm_ref.kernel_for names for the total component count of the call that uploaded the branch.  A site likelihood is a sum of products
of non-negative matrix entries: non-decreasing in every entry of every P_b.  If the device's exponentials are within their
allowances its P_b lies entrywise in [max(P_b - a_b, 0), P_b + a_b], and the exact likelihood of the device's matrices lies between
the scale-free reference evaluated at the two ends (each end moved outwards by one more ulp for the rounding to float64).
``enclosure`` returns lo, mid, hi per pattern and in total.  tests/test_mixture_cases_cpu.py holds hi - lo below 1e-9 for every
pattern of every case and step, so the enclosure cannot hide more than the bar the suite already carries.

Components built on the device (``K`` > 0): the templates are the off-diagonal parts of K of the named cases, a component is
x T_k, and x is chosen so that x T_k is the named case's matrix to the last bit or the one before.  The device's matrix then
differs from the named one by at most 3 ulp per off-diagonal entry and, in the diagonal it derives itself, by those plus two
recursive sums of D - 1 terms: ||dQ||_inf <= (D + 2) 2^-53 ||Q||_inf, and since exp of a rate matrix has infinity norm 1,
|dP| <= ||dQ||_inf entrywise.  ``built_extra`` adds that to the allowance of such a component (2.1e-14 at 61 states and norm 3).

Cases (``cases()``; fixed, named, seeded).  Component counts per branch cycle through COUNT_PATTERN, which puts 1, 2, 3, 5 and 16
side by side; one component of the first 5-component branch has weight exactly 0; the 2-component branches 5 and 9 carry one
matrix twice at weight 1/2.

    ladder_D{4,20,33,61,64}      8 leaves, 40 patterns (conserved, conflicting, ambiguous, random: scalefree._patterns)
    balanced_D61                 balanced (2, 3), HEAVY_PATTERN: 89 components
    poly12_D20                   POLY12 of tests/test_gpu_joint.py (3- and 5-way nodes)
    deep_D61_40, deep_D4_120     ladders of 40 and 120 leaves, short branches: the 2^64 rescale fires
    classes_D61                  the D = 61 ladder as a two-class partition: ``scenario(name, cls)`` has other components per class
    rep_D61, rep_D20             the ladders with every pattern twice (different weights): the class-compressed form
    built{2,3}_D{4,20,61}        templates K = 2, 3; counts 1 to 3 (rows x K <= 400, the kernel-argument block)
    built2_D61_at400, _over400   200 and 201 rows at K = 2: on and above the limit; built3_D61_over400: 136 rows at K = 3

``Scenario`` is the one call sequence every form runs (tests/test_gpu_mixture.py); its ``ref(step)`` recomputes the enclosure
from the state of every branch after that step.
"""
import functools

import numpy as np

from tests import expm_ref as er
from tests import scalefree as sf

CUS = 256                                     # compute units assumed where no device is there to ask (an MI355X has 256)
COUNTS = (1, 2, 3, 5, 16)
COUNT_PATTERN = (1, 2, 3, 5, 16, 2, 1, 3, 5, 2, 3, 1, 2, 3)
HEAVY_PATTERN = (16, 1, 3, 5, 16, 2, 1, 16, 5, 2, 16, 1, 2, 3)    # 89 components: two workgroups per matrix at 49-64 states
SMALL_PATTERN = (1, 2, 3, 3, 2, 2, 1, 3, 1, 2, 3, 1, 2, 3)
HALVES = (5, 9)                               # 2-component branches that carry one matrix twice at weight 1/2
WIDTH_BAR = 1e-9
INLINE_LIMIT = 400                            # kCoefInline (csrc/common.h): coefficients that travel in the kernel-argument block
U = 2.0 ** -53


def _pool(D, deep, K=0):
    """(dense names, all names) a case at D states draws its components from."""
    if K:
        names = _template_names(D, K)
        dense = [n for n in _multiples(D, names) if not n.endswith("n6")]
        return dense, dense
    if deep:
        dense = [f"rev_D{D}_n0p2", f"rev_D{D}_nb011", f"rev_D{D}_na011", f"rev_D{D}_nb025", f"nonrev_D{D}_n0p2"]
        return dense, dense + [f"stiff_D{D}_n0p2"] + ([f"mg94_D61_n0p2", "mg94_D61_nb025"] if D == 61 else [])
    dense = [f"rev_D{D}_n{t}" for t in ("0p2", "0p4", "0p8", "3", "6")] + [f"nonrev_D{D}_n0p2", f"nonrev_D{D}_n3"]
    rest = [f"stiff_D{D}_n0p2", f"stiff_D{D}_n3"]
    if D == 61:
        rest += [f"mg94_D61_n{t}" for t in ("0p2", "0p4", "0p8", "3", "6")]
    return dense, dense + rest


def _template_names(D, K):
    return [f"rev_D{D}_n0p2", f"rev_D{D}_n0p4", f"nonrev_D{D}_n0p2"][:K]


def _multiples(D, template_names):
    """Names of the cases that are a multiple of one of the templates (the same seeded base matrix at another norm)."""
    out = []
    for t in template_names:
        fam = t.split("_")[0]
        tags = ("0p2", "3") if t.endswith("n0p2") else ("0p4", "0p8", "6")
        out += [f"{fam}_D{D}_n{x}" for x in tags]
    return out


def _offdiag(Q):
    T = np.array(Q, dtype=np.float64)
    T[np.arange(len(T)), np.arange(len(T))] = 0.0
    return T


@functools.lru_cache(maxsize=None)
def templates(D, K):
    """[K, D, D] templates (zero diagonals) of the built cases at D states."""
    by = er.cases_by_name()
    return np.stack([_offdiag(by[n]["Q"]) for n in _template_names(D, K)])


@functools.lru_cache(maxsize=None)
def coefficient_row(D, K, name):
    """The row x [K] with x T = the off-diagonal part of case ``name`` (to an ulp per entry): one non-zero entry."""
    by = er.cases_by_name()
    Q = by[name]["Q"]
    for k, t in enumerate(_template_names(D, K)):
        if t.split("_")[0] != name.split("_")[0]:
            continue
        T = templates(D, K)[k]
        x = float(Q[0, 1] / T[0, 1])
        if np.abs(x * T - _offdiag(Q)).max() <= 4 * U * np.abs(Q).max():
            row = np.zeros(K)
            row[k] = x
            return row
    raise KeyError(name)


def host_built(D, K, name):
    """What the dense entry point is given for a built component: sum_k x_k T_k with the diagonal set on the host."""
    Q = np.tensordot(coefficient_row(D, K, name), templates(D, K), axes=1)
    return er._set_diagonal(Q)


def built_extra(name):
    """The device forms x T and its diagonal itself: |dP| <= ||dQ||_inf <= (D + 2) 2^-53 ||Q||_inf (module docstring)."""
    Q = er.cases_by_name()[name]["Q"]
    return (len(Q) + 2) * U * er.norm_inf(Q)


# ---- cases --------------------------------------------------------------------------------------------------------------------------

def _poly12():
    from tests.test_gpu_joint import POLY12
    return POLY12


def _mk(name, seed, D, tree, S=40, deep=False, K=0, counts=COUNT_PATTERN, C=1, twice=False):
    fp, L = tree
    rng = np.random.default_rng(seed)
    if twice:
        half = sf._patterns(rng, L, D, S // 2, 2)
        codes = np.concatenate([half, half], axis=1)
    else:
        codes = sf._patterns(rng, L, D, S, 2)
    pi = rng.random(D) + 0.2
    cs = sf._case(name, D, fp, L, codes, None, rng, root_freqs=pi / pi.sum())
    del cs["P"]
    B = len(fp) - 1
    cs.update(seed=seed, deep=deep, K=K, C=C, counts=tuple(counts[b % len(counts)] for b in range(B)))
    return cs


def _enumerate():
    k = 0

    def seed():
        nonlocal k
        k += 1
        return 31000 + k
    for D in (4, 20, 33, 61, 64):
        yield _mk(f"ladder_D{D}", seed(), D, sf.ladder_tree(8))
    yield _mk("balanced_D61", seed(), 61, sf.balanced_tree(2, 3), counts=HEAVY_PATTERN)
    yield _mk("poly12_D20", seed(), 20, _poly12())
    yield _mk("deep_D61_40", seed(), 61, sf.ladder_tree(40), S=24, deep=True)
    yield _mk("deep_D4_120", seed(), 4, sf.ladder_tree(120), S=24, deep=True)
    yield _mk("classes_D61", seed(), 61, sf.ladder_tree(8), C=2)
    for D in (61, 20):
        yield _mk(f"rep_D{D}", seed(), D, sf.ladder_tree(8), twice=True)
    for K in (2, 3):
        for D in (4, 20, 61):
            yield _mk(f"built{K}_D{D}", seed(), D, sf.ladder_tree(8), K=K, counts=SMALL_PATTERN)
    yield _mk("built2_D61_at400", seed(), 61, sf.ladder_tree(8), K=2, counts=(3,) + (16,) * 12 + (5,))
    yield _mk("built2_D61_over400", seed(), 61, sf.ladder_tree(8), K=2, counts=(3,) + (16,) * 12 + (6,))
    yield _mk("built3_D61_over400", seed(), 61, sf.ladder_tree(8), K=3, counts=(3,) + (16,) * 8 + (1,) * 5)


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


def reroot_path(cs):
    """Internal indices from the given root to the node the re-rooted schedules hang the tree from (empty: none)."""
    from hyphy_amd import hip
    return [int(x) for x in hip.plan_reroot(cs["flat_parents"], int(cs["L"]))]


# ---- a branch's components, the state of a partition, its matrices -----------------------------------------------------------------

class Branch:
    """The components of one branch as uploaded: case names, weights, and the exponential kernel of the call that uploaded them."""

    def __init__(self, names, weights, kernel=None, built=False):
        self.names = tuple(names)
        self.w = np.asarray(weights, dtype=np.float64)
        self.kernel = kernel
        self.built = built
        assert len(self.names) == len(self.w) and 1 <= len(self.w) <= 16

    def under(self, kernel, built=False):
        return Branch(self.names, self.w, kernel, built)


def draw_branch(cs, rng, count, halves=False, zero=False):
    D = int(cs["D"])
    dense, everything = _pool(D, cs["deep"], cs["K"])
    if halves:
        return Branch([str(rng.choice(dense))] * 2, [0.5, 0.5])
    nm = [str(rng.choice(dense))] + [str(x) for x in rng.choice(everything, size=count - 1)]
    w = rng.random(count) + 0.1
    if zero:
        w[count // 2] = 0.0
    return Branch(nm, w / w.sum())


def kernel_for(cs, n_tot, cus=CUS):
    D = int(cs["D"])
    return er.kernel_for(D, n_tot, cus, images=D != 4)


def uploaded(cs, state, branches, new, built=None, cus=CUS):
    """``state`` with ``new[k]`` on branch ``branches[k]``, marked with the kernel one call for all of them runs."""
    built = bool(cs["K"]) if built is None else built
    kern = kernel_for(cs, sum(len(b.w) for b in new), cus)
    out = list(state)
    for b, br in zip(branches, new):
        out[int(b)] = br.under(kern, built)
    return out


def dense_input(cs, branches_of_state):
    """(per-branch [M_k, D, D] rate matrices, per-branch weights [M_k]) for hip.evaluate_mixture."""
    D, K = int(cs["D"]), cs["K"]
    by = er.cases_by_name()
    q = [np.stack([host_built(D, K, n) if K else by[n]["Q"] for n in br.names]) for br in branches_of_state]
    return q, [br.w for br in branches_of_state]


def built_input(cs, branches_of_state):
    """(per-branch [M_k, K] coefficient rows, per-branch weights) for hip.evaluate_mixture_built."""
    D, K = int(cs["D"]), cs["K"]
    return [np.stack([coefficient_row(D, K, n) for n in br.names]) for br in branches_of_state], [br.w for br in branches_of_state]


def matrices(state):
    """(P [B, D, D] in np.longdouble, allowance a [B]) of a state."""
    P, a = [], []
    for br in state:
        assert br.kernel is not None
        acc = 0
        tol = 0.0
        for n, w in zip(br.names, br.w):
            acc = acc + np.longdouble(w) * er.case_reference(n).astype(np.longdouble)
            tol += float(w) * (er.allowance(n, br.kernel) + (built_extra(n) if br.built else 0.0))
        P.append(acc)
        a.append(tol)
    return np.stack(P), np.array(a)


def enclosure(cs, state, pinned=None, conditionals=False):
    """{"lo", "mid", "hi"} [S] per pattern, {"lo_total", "mid_total", "hi_total"}, "width" [S] = hi - lo, and with ``conditionals``
    the mid reference's "cond" and "log_mag"."""
    P, a = matrices(state)
    al = a.astype(np.longdouble)[:, None, None]
    ends = {"lo": np.maximum(P - al, 0).astype(np.float64) * (1.0 - 2 * U), "mid": P.astype(np.float64), "hi": (P + al).astype(np.float64) * (1.0 + 2 * U)}
    out = {}
    freq = np.asarray(cs["pattern_freq"], dtype=np.float64)
    for key, M in ends.items():
        r = sf.prune(cs["D"], cs["flat_parents"], cs["L"], cs["leaf_codes"], cs["ambig"], cs["pattern_freq"], M, cs["root_freqs"], pinned=pinned,
                     conditionals=conditionals and key == "mid")
        out[key] = r["site_logl"]
        out[key + "_total"] = float(np.sum(r["site_logl"] * freq))
        if key == "mid" and conditionals:
            out["cond"], out["log_mag"] = r["cond"], r["log_mag"]
    out["width"] = out["hi"] - out["lo"]
    return out


def hold_enclosure(what, got, r):
    """got = (log-L, likelihoods, exponents) of an evaluation with per_site=True against an enclosure ``r``: every pattern and the total
    inside [lo, hi] widened by the allowance of tests/hold.py; returns the largest (got - mid) / (half width + that allowance)."""
    from tests.hold import ATOL, RTOL, _site
    ll, lik, sc = got
    assert sc.dtype == np.int64 and np.all(np.abs(sc) < 4096), (what, sc)
    assert np.all(np.isfinite(lik)) and np.all(lik > 0), (what, lik)
    site = _site(lik, sc)
    t = RTOL * np.abs(r["mid"]) + ATOL
    ratio = np.abs(site - r["mid"]) / (0.5 * r["width"] + t)
    tt = RTOL * abs(r["mid_total"]) + ATOL
    rtot = abs(ll - r["mid_total"]) / (0.5 * (r["hi_total"] - r["lo_total"]) + tt)
    worst = max(float(ratio.max()), rtot)
    print(f"{what}: largest (got - mid) / (half width + t) = {worst:.4f}; log-L {ll!r} in [{r['lo_total']!r}, {r['hi_total']!r}]")
    assert np.all(site >= r["lo"] - t) and np.all(site <= r["hi"] + t), (what, int(np.argmax(ratio)), float(ratio.max()))
    assert r["lo_total"] - tt <= ll <= r["hi_total"] + tt, (what, ll, r["lo_total"], r["hi_total"])
    return worst


# ---- the one call sequence -----------------------------------------------------------------------------------------------------------

class Scenario:
    """States and nodes of the sequence on one case (``cls``: the rate class, whose components differ).  ``state[k]``: every
    branch's components after step k; ``ref(k)``: the enclosure under it, computed once.

       1, 2   full mixture passes                        state[1]
       3      leaf branch ``leaf``: 3 -> 16 components   state[3]
       4      the same branch: 16 -> 1                   state[4]   (= a plain update of that matrix)
       5      internal branch ``inner`` (the middle of the re-rooting path): new components, 5 of them          state[5]
       6      a PLAIN update of ``nxt``, the next branch on that path                                           state[6]
       7, 11  full mixture passes under state[6]
       8      the branch cache at ``bc`` with one matrix  state[8]   (nothing is stored)
       9      pinned at ``pin`` under state[6]            ref("pin")
       10     download_partials                           ref("cond")
    """

    def __init__(self, cs, cls=0, cus=CUS):
        self.cs, self.cus = cs, cus
        L, fp = int(cs["L"]), cs["flat_parents"]
        I = len(fp) - L
        B = L + I - 1
        rng = np.random.default_rng([int(cs["seed"]), 7, cls])
        counts = cs["counts"]
        zero_at = counts.index(5) if 5 in counts else -1
        first = [draw_branch(cs, rng, counts[b], halves=(b in HALVES and counts[b] == 2), zero=(b == zero_at)) for b in range(B)]
        self.nodes = np.arange(B, dtype=np.int64)
        self.leaf = next(b for b in range(L) if counts[b] == 3)
        path = reroot_path(cs)
        self.path = path
        if len(path) >= 3:
            self.inner, self.nxt = L + path[len(path) // 2], L + path[len(path) // 2 + 1]
            self.pin, self.bc = L + path[1], L + path[-1]
        else:
            self.inner = L
            up = int(fp[L])
            self.nxt = L + up if up != I - 1 else L + 1
            self.pin = self.bc = self.inner
        S = cs["leaf_codes"].shape[1]
        self.states = ((np.arange(S) * 5 + 1) % int(cs["D"])).astype(np.int64)
        dense = _pool(int(cs["D"]), cs["deep"], cs["K"])[0]
        st = {}
        st[1] = uploaded(cs, [None] * B, self.nodes, first, cus=cus)
        st[3] = uploaded(cs, st[1], [self.leaf], [draw_branch(cs, rng, 16)], cus=cus)
        self.single = Branch([str(rng.choice(dense))], [1.0])
        st[4] = uploaded(cs, st[3], [self.leaf], [self.single], cus=cus)
        st[5] = uploaded(cs, st[4], [self.inner], [draw_branch(cs, rng, 5)], cus=cus)
        self.plain = Branch([str(rng.choice(dense))], [1.0])
        st[6] = uploaded(cs, st[5], [self.nxt], [self.plain], cus=cus)
        self.bc_branch = Branch([str(rng.choice(dense))], [1.0])
        st[8] = uploaded(cs, st[6], [self.bc], [self.bc_branch], cus=cus)
        st[2], st[7], st[11] = st[1], st[6], st[6]
        self.state = st
        self._refs = {}

    def ref(self, step):
        step = {2: 1, 7: 6, 11: 6}.get(step, step)
        if step not in self._refs:
            if step == "pin":
                self._refs[step] = enclosure(self.cs, self.state[6], pinned=(self.pin, self.states))
            elif step == "cond":
                self._refs[step] = enclosure(self.cs, self.state[6], conditionals=True)
            else:
                self._refs[step] = enclosure(self.cs, self.state[step])
        return self._refs[step]

    def steps(self):
        """Every reference of the sequence (the CPU tests go through all of them)."""
        return [1, 3, 4, 5, 6, 8, "pin"] if int(self.cs["D"]) != 4 else [1, 3, 4, 5, 6, "pin"]


_scenarios = {}


def scenario(name, cls=0, cus=CUS):
    key = (name, cls, cus)
    if key not in _scenarios:
        _scenarios[key] = Scenario(cases_by_name()[name], cls, cus)
    return _scenarios[key]
