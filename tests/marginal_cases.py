"""Cases, references and the comparison for marginal ancestral reconstruction (hyphy_hip_marginal_ancestral), shared by
tests/test_gpu_marginal.py and tests/test_marginal_cases_cpu.py.

The reference is ``scalefree.prune(..., posteriors=True)``: ``post`` for the internal rows, ``leaf_post`` for the leaf rows (pinned on
the CPU to the pinned-state evaluation and to brute force by tests/test_scalefree_cpu.py).  ``hold_support`` compares COMPONENTWISE:
every operation of the walk is a product or a sum of non-negative numbers, so a correct kernel computes a support of 1e-60 to the same
relative accuracy as one of 0.5, and an absolute tolerance would hide a dropped factor in it.

``model_support`` is the device's scheme in plain float64 numpy — conditionals and outside vectors rescaled by powers of 2^64 on
their sums (threshold 2^-64, up to 15 steps, both directions), classes accumulated the way MargSink::add accumulates them — and
serves the CPU test alone: a correct implementation of the scheme passes ``hold_support`` on every case of this module, and the
class accumulation with the min-exponent rule applied to a zero contribution does not.

Largest componentwise deviation of that model from the reference over every case of this module, supports of at least FLOOR,
measured by test_marginal_cases_cpu.py::test_model_of_the_scheme_passes_the_bar:

    MODEL_MAX_REL = 1.4e-14

(1.38e-14 measured, classes_D20_k2; the constant is that rounded up.)  That is more than 100 x below the 1e-9 bar, so FLOOR stays
at 1e-100.  The device keeps vector sums inside [2^-64, 2^64]: an entry of relative size r of such a vector is a normal number down
to r ~ 2^-958, and entries around 1e-100 lose nothing unless the scheme itself is wrong.
"""
import numpy as np

from tests import branchcache_cases as bc, scalefree as sf

RTOL = 1e-9            # the project's rtol for supports (test_oracle_golden.py's), here per component
FLOOR = 1e-100
MODEL_MAX_REL = 1.4e-14
MAP_MARGIN = 1e-6      # MAP states are compared with the reference where its two largest supports differ by more (relative)
MAP_LEFT_OUT = 1e-3    # and the margin may leave out at most this share of the (row, pattern) entries


def pin_update_list(fp, L, code):
    """The update list of an evaluation with node ``code`` pinned, and of the one that puts the path back after the pin is removed:
    the node's own path, and the children of an internal node (the node itself is recomputed when one of its children is listed)."""
    from hyphy_amd import tree
    flat = tree.flat_from_parents(fp, L)
    out = set()
    if int(flat.flat_parents[code]) >= 0:
        out.update(int(x) for x in flat.path_update_nodes(int(code)))
    if code >= L:
        out.update(int(c) for c in flat.children_of(code - L))
    return np.array(sorted(out), dtype=np.int64)


def hold_support(what, got, ref, sums_to_one=False):
    """``got`` [rows, S', D] against the reference's ``ref``: finite wherever the reference is; |got - ref| <= RTOL x ref for every
    entry with ref >= FLOOR and <= RTOL x FLOOR below it; rows summing to 1 within 1e-12 (internal rows).  Returns the largest
    relative deviation above the floor."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    bad = np.argwhere(fin & ~np.isfinite(got))
    assert not len(bad), f"{what}: row {bad[0][0]} pattern {bad[0][1]} state {bad[0][2]}: {got[tuple(bad[0])]!r}, reference {ref[tuple(bad[0])]!r}"
    r = np.where(fin, ref, 0.0)
    dev = np.where(fin, np.abs(np.where(fin, got, 0.0) - r), 0.0)
    over = dev / (RTOL * np.maximum(r, FLOOR))
    w = np.unravel_index(int(np.argmax(over)), over.shape)
    big = fin & (r >= FLOOR)
    rel = float(np.max(dev[big] / r[big])) if big.any() else 0.0
    print(f"{what}: largest deviation / allowance = {over[w]:.3e}; largest relative deviation above the floor {rel:.3e}")
    assert over[w] <= 1.0, f"{what}: row {w[0]} pattern {w[1]} state {w[2]}: {got[w]!r}, reference {ref[w]!r}"
    if sums_to_one:
        rows = fin.all(axis=2)
        tot = np.where(rows, np.where(fin, got, 0.0).sum(axis=2), 1.0)
        w = np.unravel_index(int(np.argmax(np.abs(tot - 1.0))), tot.shape)
        assert abs(tot[w] - 1.0) <= 1e-12, f"{what}: row {w[0]} pattern {w[1]} sums to {tot[w]!r}"
    return rel


def map_agreement(ref):
    """(rows, patterns) where the reference's MAP state is decided by more than MAP_MARGIN: that mask [rows, S'], the mask of the
    possible patterns, the reference's argmax."""
    r = np.where(np.isfinite(ref), ref, -1.0)
    if r.shape[2] == 1:
        r = np.concatenate([r, np.full_like(r, -1.0)], axis=2)
    top2 = np.sort(r, axis=2)[:, :, -2:]
    fin = np.isfinite(ref).all(axis=2)
    decided = fin & (top2[:, :, 1] - top2[:, :, 0] > MAP_MARGIN * top2[:, :, 1])
    return decided, fin, r.argmax(axis=2)


def has_uniform_matrix(cs):
    """Whether some branch's off-diagonal entries are all equal (near_identity with spread=False: the stars, the threshold cases,
    the 1e-2 class at 61 states).  States that such a tree treats alike have EQUAL supports, exactly: ties that no margin decides."""
    D = int(cs["D"])
    P = cs["P"].reshape(-1, D, D)
    off = P[:, ~np.eye(D, dtype=bool)]
    return D > 2 and bool(np.any(off.max(axis=1) == off.min(axis=1)))


def hold_map(what, ms, mv, sup, ref):
    """MAP state and support [rows, S'] of a call against its own support ``sup`` (first argmax and maximum, exactly) and against
    the reference: equal to its argmax wherever that is decided by more than MAP_MARGIN, and everywhere, ties included, a state
    whose reference support lies within MAP_MARGIN of the largest; -1 / NaN exactly where the pattern is impossible.  Returns the
    number of entries the margin leaves to the second check alone."""
    decided, fin, arg = map_agreement(ref)
    assert ms.dtype == np.int64 and np.array_equal(ms[fin], sup.argmax(axis=2)[fin]), what
    assert np.array_equal(mv[fin], sup.max(axis=2)[fin]), what
    assert np.all(ms[~fin] == -1) and np.all(np.isnan(mv[~fin])), (what, ms[~fin], mv[~fin])
    r = np.where(fin[:, :, None], ref, 0.0)
    at = np.take_along_axis(r, np.maximum(ms, 0)[:, :, None], axis=2)[:, :, 0]
    assert np.all(at[fin] >= (1.0 - MAP_MARGIN) * r.max(axis=2)[fin]), (what, np.argwhere(fin & (at < (1.0 - MAP_MARGIN) * r.max(axis=2)))[:4])
    assert np.array_equal(ms[decided], arg[decided]), (what, np.argwhere(decided & (ms != arg))[:4])
    return int((fin & ~decided).sum())


# ---- the device's scheme in float64 -------------------------------------------------------------------------------------------

_T, _U = 2.0 ** -64, 2.0 ** 64


def _rescale(v, cnt):
    """rescale_vec / rescale_decision: powers of 2^64 on the sum, at most 15 steps either way; a zero vector stays as it is."""
    tot = v.sum(axis=1)
    for _ in range(15):
        low, high = (tot < _T) & (tot > 0), (tot > _U) & np.isfinite(tot)
        if not (low.any() or high.any()):
            break
        v[low] *= _U; tot[low] *= _U; cnt[low] += 1
        v[high] *= _T; tot[high] *= _T; cnt[high] -= 1
    return v, cnt


def _model_class(cs, P, which):
    """One class: numerators [rows, S, D], denominators [rows, S] and 2^64 exponents [rows, S] as the walk hands them to its sink."""
    D, L = int(cs["D"]), int(cs["L"])
    fp, codes, amb = cs["flat_parents"], cs["leaf_codes"], cs["ambig"]
    I, S = len(fp) - L, codes.shape[1]
    ch, sel = sf.children_of(fp, L), np.arange(S)
    cond, cnt = [None] * I, np.zeros((I, S), dtype=np.int64)
    for n in range(I):                                   # the pruning pass: every node tested on its sum
        v = np.ones((S, D))
        for c in ch[n]:
            v = v * sf._edge(P[c], c, L, codes, amb, cond, None, sel)
            cnt[n] += cnt[c - L] if c >= L else 0
        cond[n], cnt[n] = _rescale(v, cnt[n])
    rows = I if which == 0 else L
    num, dn, ex = np.zeros((rows, S, D)), np.zeros((rows, S)), np.zeros((rows, S), dtype=np.int64)
    U, Ucnt = {I - 1: np.broadcast_to(cs["root_freqs"], (S, D)).copy()}, {I - 1: np.zeros(S, dtype=np.int64)}
    for n in range(I - 1, -1, -1):                       # (children are numbered before parents: this is a pre-order)
        pre, pcnt, slots = U[n], Ucnt[n], []
        for c in ch[n]:                                  # prefix pass
            E, ecnt = sf._edge(P[c], c, L, codes, amb, cond, None, sel), (cnt[c - L] if c >= L else np.zeros(S, dtype=np.int64))
            slots.append((pre, pcnt, E, ecnt))
            pre, pcnt = _rescale(pre * E, pcnt + ecnt)
        if which == 0:
            num[n], dn[n], ex[n] = pre, pre.sum(axis=1), pcnt
        suf, scnt = np.ones((S, D)), np.zeros(S, dtype=np.int64)
        for i in range(len(ch[n]) - 1, -1, -1):          # suffix pass
            c = ch[n][i]
            if c >= L or which == 1:
                V, vcnt = _rescale(slots[i][0] * suf, slots[i][1] + scnt)
                Uc = V @ P[c]
                if c >= L:
                    U[c - L], Ucnt[c - L] = _rescale(Uc, vcnt)
                else:                                    # a leaf: U is NOT rescaled
                    k = codes[c]
                    lv = np.where((k >= 0)[:, None], np.eye(D)[np.maximum(k, 0)], amb[np.maximum(-k - 1, 0)])
                    num[c], dn[c], ex[c] = Uc, (Uc * lv).sum(axis=1), vcnt
            if i > 0:
                suf, scnt = _rescale(suf * slots[i][2], scnt + slots[i][3])
    return num, dn, ex


def model_support(cs, which, add="skip"):
    """Support [rows, S, D] under the model.  ``add``: how a class is added to the ones before it — "min": the smaller exponent
    always wins (MargSink::add before the fix); "skip": a contribution whose weighted denominator is exactly 0 is passed over and a
    stored denominator of 0 is overwritten (the fix).  Also returns the per-class exponents [C, rows, S]."""
    Ps = cs["P"] if cs["P"].ndim == 4 else cs["P"][None]
    ws = cs["weights"] if cs["P"].ndim == 4 else np.ones(1)
    acc = den = aexp = None
    exps = []
    for c in range(len(Ps)):
        num, dn, e = _model_class(cs, Ps[c], which)
        exps.append(e)
        wd = ws[c] * dn
        if c == 0:
            keep = (wd > 0) | (add == "min")
            acc, den, aexp = np.where(keep[:, :, None], ws[c] * num, 0.0), wd, e
            continue
        e_new = np.minimum(aexp, e)
        with np.errstate(over="ignore", invalid="ignore"):
            f_old, f_new = np.ldexp(1.0, -64 * (aexp - e_new)), ws[c] * np.ldexp(1.0, -64 * (e - e_new))
            a2, d2 = acc * f_old[:, :, None] + num * f_new[:, :, None], den * f_old + dn * f_new
        if add == "skip":
            store, skip = (den == 0) & (wd > 0), ~(wd > 0)
            a2 = np.where(store[:, :, None], ws[c] * num, np.where(skip[:, :, None], acc, a2))
            d2 = np.where(store, wd, np.where(skip, den, d2))
            e_new = np.where(store, e, np.where(skip, aexp, e_new))
        acc, den, aexp = a2, d2, e_new
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((den > 0)[:, :, None], acc / den[:, :, None], np.nan), np.stack(exps)


# ---- cases --------------------------------------------------------------------------------------------------------------------

STATE_COUNTS = (2, 4, 5, 16, 17, 20, 32, 33, 48, 49, 61, 64)
SCALEFREE = tuple(sf.SUBSET) + ("ladder_D4_300", "ladder_D20_600", "ladder_D61_120_on_k4d3", "ladder_D4_200_on_k4d3", "star_D61_n9_2em8",
                                "star_D4_n8_1em9", "threshold_D4_below", "threshold_D61_above", "mixed_D4_k2_1em6_S300")
CLASSES = ("classes_D61_k2", "classes_D4_k3", "classes_D20_k2")
CLASS_ORDERS = {"given": (0, 1, 2), "reversed": (2, 1, 0), "1em30_first": (2, 0, 1)}
ALL_IMPOSSIBLE = ("mixed_D4_k4_1em20_S37", "mixed_D61_k4_1em15_S53")
FORMS = ALL_IMPOSSIBLE


def _states_case(D, seed):
    rng = np.random.default_rng(seed)
    fp, L = sf.balanced_tree(2, 3)
    codes = sf._patterns(rng, L, D, 17, 2)
    codes[1, 2], codes[5, 6] = -1, -2                    # two ambiguity codes for certain
    B = len(fp) - 1
    P = sf.ordinary(rng, B, D)
    P[:L] = sf.near_identity(rng, L, D, 1e-12)
    pi = rng.random(D) + 0.1
    return sf._case(f"states_D{D}", D, fp, L, codes, P, rng, root_freqs=pi / pi.sum())


def _wide_case(D, seed):
    rng = np.random.default_rng(seed)
    fp, L = bc.star_tree(40)
    codes = sf._patterns(rng, L, D, 20, 40)
    pi = rng.random(D) + 0.1
    return sf._case(f"wide_D{D}_n40", D, fp, L, codes, sf.near_identity(rng, len(fp) - 1, D, 1e-6), rng, root_freqs=pi / pi.sum())


def _impossible_case(D, seed, order):
    """Two classes on the 64-taxon four-way tree: A near-identity at 1e-30 (dense), B ordinary with the last state cut off.  The last
    four patterns put state D - 1 at one leaf and other states, all in conflict, elsewhere: impossible under B, possible under A."""
    rng = np.random.default_rng(seed)
    fp, L = sf.balanced_tree(4, 3)
    codes = np.concatenate([sf._patterns(rng, L, D, 20, 4), np.zeros((L, 4), dtype=np.int64)], axis=1)
    j = np.arange(L)
    for t in range(4):
        codes[:, 20 + t] = (j + j // 4 + j // 16 + t) % (D - 1)
        codes[(0, 21, 42, 63)[t], 20 + t] = D - 1
    B = len(fp) - 1
    P = np.stack([sf.near_identity(rng, B, D, 1e-30), sf._block_zero(sf.ordinary(rng, B, D), D)])
    w = np.array([0.6, 0.4])
    pi = rng.random(D) + 0.1
    cs = sf._case(f"one_class_impossible_D{D}_{'AB' if order == (0, 1) else 'BA'}", D, fp, L, codes, P[list(order)], rng,
                  root_freqs=pi / pi.sum(), weights=w[list(order)])
    cs["class_A"] = order.index(0)
    cs["special"] = np.arange(20, 24)
    return cs


def _reordered(name, tag, order=(0, 1, 2), weights=None):
    base = sf.cases_by_name()[name]
    cs = dict(base, name=f"{name}_{tag}", P=base["P"][list(order)])
    cs["weights"] = np.asarray(weights, dtype=np.float64) if weights is not None else base["weights"][list(order)]
    return cs


_cases = {}


def cases():
    """name -> case, in the groups of GROUPS; built once per process."""
    if not _cases:
        for j, D in enumerate(STATE_COUNTS):
            cs = _states_case(D, 8100 + j)
            _cases[cs["name"]] = cs
        by = sf.cases_by_name()
        for n in SCALEFREE:
            _cases[n] = by[n]
        for j, D in enumerate((4, 20)):
            cs = _wide_case(D, 8200 + j)
            _cases[cs["name"]] = cs
        for n in CLASSES:
            for tag, order in CLASS_ORDERS.items():
                _cases[f"{n}_{tag}"] = _reordered(n, tag, order)
            _cases[f"{n}_w0"] = _reordered(n, "w0", weights=(0.0, 0.6, 0.4))
        for j, D in enumerate((61, 4)):
            for order in ((0, 1), (1, 0)):
                cs = _impossible_case(D, 8300 + j, order)
                _cases[cs["name"]] = cs
        for n in ALL_IMPOSSIBLE:
            _cases[n] = by[n]
    return _cases


def group(prefix):
    if prefix == "scalefree":
        return list(SCALEFREE)
    if prefix == "all_impossible":
        return list(ALL_IMPOSSIBLE)
    return [n for n in cases() if n.startswith(prefix)]


_refs = {}


def reference(name):
    """scalefree's posteriors of the case (``post``, ``leaf_post``, ``site_logl`` ...), computed once per process and not to be written to."""
    if name not in _refs:
        with np.errstate(invalid="ignore"):
            _refs[name] = sf.case_reference(cases()[name], posteriors=True)
    return _refs[name]
