"""Host-side decisions of hyphy_hip_create that need no device (C-ABI: hyphy_hip_plan_reroot, hyphy_hip_plan_pattern_order,
hyphy_hip_plan_schedule): the node steady-state passes may be re-rooted at, the device-side pattern order, and the join
table of chain schedules as the kernels decode it."""
import collections

import numpy as np
import pytest

from hyphy_amd import hip, tree


def _eccentricities(flat):
    fp, L = np.asarray(flat.flat_parents), flat.L
    N = len(fp)
    adj = [[] for _ in range(N)]
    for c, p in enumerate(fp):
        if p >= 0:
            adj[c].append(L + p)
            adj[L + p].append(c)
    ecc = {}
    for r in range(L, N):
        dist = {r: 0}
        q = collections.deque([r])
        while q:
            u = q.popleft()
            for v in adj[u]:
                if v not in dist:
                    dist[v] = dist[u] + 1
                    q.append(v)
        ecc[r - L] = max(dist[leaf] for leaf in range(L))
    return ecc


def test_reroot_plan_finds_the_centre_of_the_tree():
    rng = np.random.default_rng(11)
    n_rerooted = 0
    for trial in range(120):
        n = int(rng.integers(5, 90))
        root = (tree.caterpillar_tree(max(5, n)) if trial % 5 == 0
                else tree.random_tree(n, rng, trifurcating_root=bool(rng.integers(0, 2))))
        flat = tree.flatten(root)
        ecc = _eccentricities(flat)
        best = min(ecc.values())
        I = flat.I
        centres = sorted(k for k, e in ecc.items() if e == best)
        assert len(centres) in (1, 2)            # the centre of a tree: one node or two adjacent ones
        cands = [hip.plan_reroot(flat.flat_parents, flat.L, c) for c in (0, 1)]
        cands = [c for c in cands if len(c)]
        offered = sorted(int(c[-1]) for c in cands)
        def depth(k):                                # edges between internal node k and the given root
            d = 0
            while k != I - 1:
                k, d = int(flat.flat_parents[flat.L + k]), d + 1
            return d
        # every centre node other than the given root is offered (if it is within the 32 twin images), nothing else
        # (trees with fewer than four internal nodes are left alone)
        assert offered == [k for k in centres if k != I - 1 and depth(k) <= 32 and I >= 4], (trial, offered, centres)
        for path in cands:
            assert int(path[0]) == I - 1 and len(path) - 1 <= 32
            for a, b in zip(path[:-1], path[1:]):  # each step goes from a node to one of its children
                assert int(flat.flat_parents[flat.L + int(b)]) == int(a)
        n_rerooted += bool(cands) and ecc[I - 1] > best
    assert n_rerooted > 20                         # most random trees are not hung from their centre


def test_pattern_order_is_a_permutation_grouped_by_majority_state():
    rng = np.random.default_rng(3)
    L, S, D = 12, 500, 61
    base = rng.integers(0, D, size=S)
    codes = np.where(rng.random((L, S)) < 0.25, rng.integers(0, D, size=(L, S)), base[None, :]).astype(np.int64)
    codes[3, 17] = -2                              # an ambiguity code sorts like any other value
    order = hip.plan_pattern_order(D, codes)
    assert sorted(order.tolist()) == list(range(S))
    major = np.array([np.bincount(codes[:, s][codes[:, s] >= 0], minlength=D).argmax() for s in range(S)])
    assert np.all(np.diff(major[order]) >= 0)      # primary key: the pattern's most frequent state
    # inside a group: lexicographic by leaf
    for m in np.unique(major):
        cols = [tuple(codes[:, s]) for s in order if major[s] == m]
        assert cols == sorted(cols)
    # short alignments keep the caller's order
    assert hip.plan_pattern_order(D, codes[:, :20]).tolist() == list(range(20))


def _flat_caterpillar(L):
    """Post-order parents of a caterpillar with L leaves and a trifurcating root (L - 2 internal nodes)."""
    I = L - 2
    fp = np.empty(L + I, dtype=np.int64)
    fp[0] = fp[1] = 0                      # the cherry at the far end
    for k in range(1, I):
        fp[L + k - 1] = k                  # internal node k - 1 hangs below internal node k
        fp[k + 1] = k                      # ... together with leaf k + 1
    fp[L - 1] = I - 1                      # the root's third child
    fp[L + I - 1] = -1
    return fp


def test_chain_schedule_join_table_decodes_for_every_kernel_and_cut():
    """prune.hip decodes jn[n].x as parent | image slot << 16 (negative: root) and jn[n].y & 0xff as the arrivals a node waits
    for: every record of every cut must decode to the topology the schedule was built on — random trees, both chain kernels,
    re-rooted and not."""
    rng = np.random.default_rng(5)
    seen_chain = seen_rr = 0
    for trial in range(60):
        n = int(rng.integers(6, 200))
        flat = tree.flatten(tree.caterpillar_tree(n) if trial % 6 == 0 else tree.random_tree(n, rng, trifurcating_root=bool(rng.integers(0, 2))))
        for kernel in (1, 2):
            for m in (1, 3, 8):
                for rr in (False, True):
                    info = hip.plan_schedule(flat.flat_parents, flat.L, kernel=kernel, chain_m=m, ntiles=int(rng.integers(1, 700)), reroot=rr)
                    assert info["decode_errors"] == 0, (trial, kernel, m, rr, info)
                    if info["chain"]:
                        seen_chain += 1
                        assert info["max_slot"] < 32768 and info["max_need"] <= 255
                    seen_rr += info["rerooted"]
    assert seen_chain > 300 and seen_rr > 20


def test_trees_beyond_the_packed_join_table_get_no_chain_schedule():
    """r02 ADVICE: parent | slot << 16 in one signed int goes negative (= "root") once an image slot reaches 2^15, i.e. for
    trees of roughly 10 000 taxa and more (twin slots of re-rooted schedules first), and arrivals are an 8-bit field.  Such trees
    must fall back to a cut that needs no join table instead of silently truncating the pass."""
    ok = hip.plan_schedule(_flat_caterpillar(9000), 9000, kernel=1, chain_m=12, ntiles=4)
    assert ok["chain"] == 1 and ok["decode_errors"] == 0 and ok["max_slot"] < 32768
    big = hip.plan_schedule(_flat_caterpillar(12000), 12000, kernel=1, chain_m=12, ntiles=4)
    assert big["chain"] == 0 and big["programs"] >= 1
    big_rr = hip.plan_schedule(_flat_caterpillar(11000), 11000, kernel=2, chain_m=5, ntiles=4, reroot=True)
    assert big_rr["chain"] == 0
    # a star of 300 cherries below the root: 300 internal children of one node
    L, I = 600, 301
    fp = np.empty(L + I, dtype=np.int64)
    for k in range(300):
        fp[2 * k] = fp[2 * k + 1] = k
        fp[L + k] = 300
    fp[L + 300] = -1
    star = hip.plan_schedule(fp, L, kernel=1, chain_m=1, ntiles=16)
    assert star["chain"] == 0
    fp2 = fp[: 2 * 200 + 201].copy()       # 200 cherries: fits
    L2 = 400
    fp2 = np.empty(L2 + 201, dtype=np.int64)
    for k in range(200):
        fp2[2 * k] = fp2[2 * k + 1] = k
        fp2[L2 + k] = 200
    fp2[L2 + 200] = -1
    star2 = hip.plan_schedule(fp2, L2, kernel=1, chain_m=1, ntiles=16)
    assert star2["chain"] == 1 and star2["max_need"] == 200 and star2["decode_errors"] == 0


def test_subtree_repeat_classes_and_compressed_set():
    """Subtree repeats (repeats.hip; the reference's tcc masks, src/core/tree.cpp:2801-2858): the classes hyphy_hip_create counts per
    internal node are the distinct leaf sub-patterns below it, the compressed set is closed downwards and never contains the root, and
    the reference's run-length form (a site whose subtree leaves equal the PREVIOUS site's is skipped) can never skip more than the
    class form does."""
    from hyphy_amd import data
    rng = np.random.default_rng(5)
    for trial in range(6):
        taxa = int(rng.integers(6, 40))
        syn = data.evolve(taxa, 400, 3, seed=100 + trial, p_change=0.06)
        pd = data.from_states(syn.states, 61, compress_patterns=True)
        flat = syn.flat
        L, I = flat.L, flat.I
        codes = np.asarray(pd.leaf_codes)
        if trial % 2:   # ambiguity codes are characters like any other
            mask = rng.random(codes.shape) < 0.04
            codes = codes.copy()
            codes[mask] = -1 - rng.integers(0, 3, size=int(mask.sum()))
        S = codes.shape[1]
        theta = [0.2, 0.35, 0.6][trial % 3]
        classes, comp, work = hip.plan_repeats(flat.flat_parents, L, codes, theta)
        # independent count: leaves below every internal node, distinct columns of the leaf table restricted to them
        parents = np.asarray(flat.flat_parents)
        below = [set() for _ in range(I)]
        for n in range(L + I - 1):
            below[parents[n]] |= ({n} if n < L else below[n - L])
        for n in range(I):
            rows = sorted(below[n])
            want = len({tuple(codes[rows, s]) for s in range(S)})
            assert classes[n] == want, (trial, n, classes[n], want)
        assert not comp[I - 1]
        for n in range(I - 1):
            kids_ok = all(comp[c - L] for c in range(L, L + I - 1) if parents[c] == n)
            assert comp[n] == (classes[n] <= theta * S and classes[n] <= 32000 and kids_ok), (trial, n)
        assert work == sum(int(classes[n]) if comp[n] else S for n in range(I - 1))
        # the reference's masks: node n is skipped at site position s > 0 when its leaves equal those of position s - 1; at best
        # (sites sorted so that equal sub-patterns are neighbours) that leaves one evaluation per class
        for n in range(I - 1):
            rows = sorted(below[n])
            runs = 1 + sum(1 for s in range(1, S) if tuple(codes[rows, s]) != tuple(codes[rows, s - 1]))
            assert runs >= classes[n]


def test_nucgen_source_covers_every_node_and_compiles_for_gfx950():
    """hyphy_hip_plan_nucgen (no device; hiprtc cross-compiles): the straight-line kernel the library generates for a 4-state
    partition's steady-state full pass names every internal node once, reads every leaf's code once, takes the lookup path for
    plain leaves and the guarded general path for leaves with ambiguity codes, and compiles for gfx950."""
    import re
    rng = np.random.default_rng(5)
    for trial in range(6):
        n = int(rng.integers(4, 70))
        root = tree.random_tree(n, rng, trifurcating_root=bool(trial % 2))
        flat = tree.flatten(root)
        amb = np.zeros(flat.L, dtype=np.int64)
        if trial >= 3:
            amb[rng.integers(0, flat.L, size=2)] = 1
        small = bool(trial % 3 == 0)   # (the small-shard form: matrices in LDS, exponentials and combine inside the launch)
        src, ok = hip.plan_nucgen(flat.flat_parents, flat.L, amb, compile_it=True, small=small)
        assert src, "the generator must cover a plain full pass"
        assert ok, "hiprtc must compile the generated source for gfx950"
        finals = re.findall(r"double n(\d+)_0 = ", src)
        assert sorted(int(x) for x in finals) == list(range(flat.I))              # every internal node finalised exactly once
        codes = re.findall(r"const int k(\d+) = codes\[", src)
        assert sorted(int(x) for x in codes) == list(range(flat.L))               # every leaf code fetched once, up front
        assert src.count("leaf_general_(L_") == int(amb.sum())                    # guarded general path only where codes can be < 0
        assert len(re.findall(r"const double \*P\d+ = (?:L_|PT) \+ ", src)) == flat.I - 1   # one matrix per internal edge
        assert ("hyhip::expm4_one(" in src) == small and ("hyhip::combine_partials(" in src) == small
        assert "a.partials[" not in src                                           # lazy steady state: nothing persisted, nothing re-read
    # a tree beyond the LDS leaf table (L > 256): not covered, the interpreter stays
    big = tree.flatten(tree.caterpillar_tree(300))
    src, ok = hip.plan_nucgen(big.flat_parents, big.L, None, compile_it=False)
    assert src == "" and not ok


def _random_trunk(rng, n_internal):
    """A random tree over generalised leaves in the layout of a trunk view: leaves 0 .. L - 1, internal nodes L + i with children
    before parents, the root last, every internal node with at least two children."""
    kids = []                       # per internal node: children as ("leaf",) placeholders or internal indices
    roots = []                      # internal nodes without a parent yet
    for i in range(n_internal):
        k = []
        n_int = int(rng.integers(0, min(3, len(roots)) + 1)) if i + 1 < n_internal else len(roots)
        for _ in range(n_int):
            k.append(roots.pop(int(rng.integers(len(roots)))))
        n_leaf = max(0, 2 - len(k)) + int(rng.integers(0, 3))
        k += [None] * n_leaf
        kids.append(k)
        roots.append(i)
    L = sum(c is None for k in kids for c in k)
    parents = np.full(L + n_internal - 1, -1, dtype=np.int64)
    leaf = 0
    children = [[] for _ in range(n_internal)]
    for i, k in enumerate(kids):
        for c in k:
            if c is None:
                parents[leaf] = L + i
                children[i].append(leaf)
                leaf += 1
            else:
                parents[L + c] = L + i
                children[i].append(L + c)
    return L, parents, children


@pytest.mark.parametrize("seed", range(12))
def test_trunk_walk_program_computes_the_root_conditionals(seed):
    """hyphy_hip_plan_trunk_walk (repeats.hip: plan_trunk_walk, what trunk_walk_kernel interprets): random trunks, the program run by
    a small stack machine in numpy — inputs multiplied in, the edge product, a push in front of every second internal child's chain
    and its pop behind that child's product — against the plain recursion; one chain, and two chains whose products meet at the root."""
    from hyphy_amd import hip
    rng = np.random.default_rng(100 + seed)
    n_int = int(rng.integers(1, 14))
    L, parents, children = _random_trunk(rng, n_int)
    D = 3
    P = rng.uniform(0.1, 1.0, (n_int, D, D))          # one matrix per internal node's branch
    E_leaf = rng.uniform(0.1, 1.0, (L, D))            # what a generalised leaf contributes to its parent

    def cond(i):
        v = np.ones(D)
        for c in children[i]:
            v = v * (E_leaf[c] if c < L else P[c - L] @ cond(c - L))
        return v

    want = cond(n_int - 1)
    plan = hip.plan_trunk_walk(parents, L)
    assert plan["depth"] <= max(1, n_int)

    def run(first, end):
        acc, stack, seen = np.ones(D), [], 0
        for k in range(first, end):
            node, n_in, in0, flags = plan["nodes"][k]
            if flags & 1:
                stack.append(acc)
                acc = np.ones(D)
            for j in range(n_in):
                acc = acc * E_leaf[plan["inputs"][in0 + j]]
            if node < 0:
                assert k == end - 1 and not stack
                return acc
            seen += 1
            acc = P[node] @ acc
            if flags & 2:
                acc = acc * stack.pop()
        raise AssertionError("a chain must end at the root")

    one = run(*plan["one"])
    assert np.allclose(one, want, rtol=1e-12)
    if plan["two"] is not None:
        a, b = run(*plan["two"][0]), run(*plan["two"][1])
        assert np.allclose(a * b, want, rtol=1e-12)
        n0, n1 = (e - f - 1 for f, e in plan["two"])          # real nodes per chain
        assert n0 + n1 == n_int - 1 and min(n0, n1) >= 2 and 4 * min(n0, n1) >= max(n0, n1)
    # every internal node but the root is walked exactly once per form; the stack never goes deeper than reported
    first, end = plan["one"]
    walked = sorted(n for n, _, _, _ in plan["nodes"][first:end] if n >= 0)
    assert walked == list(range(n_int - 1))
    depth = d = 0
    for _, _, _, flags in plan["nodes"][first:end]:
        d += 1 if flags & 1 else 0
        depth = max(depth, d)
        d -= 1 if flags & 2 else 0
    assert depth <= plan["depth"]


def test_trunk_walk_program_of_a_balanced_trunk_nests_its_waiting_products():
    """A complete binary trunk of 15 internal nodes: the walk keeps the heavier (here: first) child's chain running and parks it
    while the sibling subtree is walked — three levels deep at the bottom; the two-chain form splits the root's two subtrees 7 + 7."""
    from hyphy_amd import hip
    depth_levels = 4
    n_int = 2 ** depth_levels - 1
    L = 2 ** depth_levels
    # internal nodes in post-order: build recursively
    parents = {}
    counter = {"leaf": 0, "int": 0}

    def build(level):
        if level == depth_levels:
            c = counter["leaf"]
            counter["leaf"] += 1
            return c
        a, b = build(level + 1), build(level + 1)
        me = L + counter["int"]
        counter["int"] += 1
        parents[a] = me
        parents[b] = me
        return me

    root = build(0)
    assert root == L + n_int - 1
    par = np.array([parents[c] for c in range(L + n_int - 1)], dtype=np.int64)
    plan = hip.plan_trunk_walk(par, L)
    assert plan["depth"] == 3 and plan["two"] is not None
    assert [e - f - 1 for f, e in plan["two"]] == [7, 7]
    first, end = plan["one"]
    assert sum(1 for _, _, _, fl in plan["nodes"][first:end] if fl & 1) == sum(1 for _, _, _, fl in plan["nodes"][first:end] if fl & 2) == 7


# ---- the class-compressed form below the trunk: hyphy_hip_plan_repeat_layout run by a numpy interpreter --------------------------

def _node(name, *kids):
    n = tree.Node(name=name, children=list(kids))
    for c in kids:
        c.parent = n
    return n


def _leaves(prefix, k):
    return [tree.Node(name=f"{prefix}{j}") for j in range(k)]


def _pad(codes, D):
    """Patterns padded as hyphy_hip_create pads a shard: state 0, to whole tiles of 16 (4 states: to 512)."""
    q = 512 if D == 4 else 16
    out = np.zeros((codes.shape[0], (codes.shape[1] + q - 1) // q * q), dtype=np.int64)
    out[:, :codes.shape[1]] = codes
    return out


def _layout_case(root, D, sites, seed, cuts=(), ambig_leaves=(), p_change=0.03, **opts):
    """(flat tree, padded leaf codes per shard, resolution vectors, layout): an alignment evolved down ``root`` with few changes,
    ambiguity codes sprinkled over ``ambig_leaves`` (names), the patterns cut into shards at ``cuts``, admission forced."""
    from hyphy_amd import data
    syn = data.evolve(0, sites, 3 if D > 5 else 1, seed=seed, p_change=p_change, tree=root)
    flat, codes = syn.flat, np.array(syn.states, dtype=np.int64) % D
    rng = np.random.default_rng(seed + 1000)
    for name in ambig_leaves:
        leaf = flat.leaf_names.index(name)
        codes[leaf, rng.choice(sites, size=max(3, sites // 10), replace=False)] = -rng.integers(1, 3, size=max(3, sites // 10))
    shards = [_pad(c, D) for c in np.split(codes, list(cuts), axis=1)]
    ambig = (rng.random((2, D)) < 0.5).astype(np.float64)
    ambig[:, 0] = 1.0
    opts.setdefault("mode", 2)
    opts.setdefault("theta", 0.9)
    return flat, shards, ambig, hip.plan_repeat_layout(flat.flat_parents, flat.L, shards, D, **opts)


def _leaf_vectors(code, ambig, D):
    """[n, D]: the unit vector of a state, the resolution vector of an ambiguity code (< 0)."""
    code = np.asarray(code)
    out = np.zeros((len(code), D))
    ok = code >= 0
    assert np.all(code[ok] < D) and np.all(-code[~ok] - 1 < len(ambig))
    out[np.nonzero(ok)[0], code[ok]] = 1.0
    out[~ok] = ambig[-code[~ok] - 1]
    return out


def _run_tables_mfma(lay, sh, P, ambig, D, L):
    """The lower phase as class_table_kernel walks it: every descriptor in order, per table row the path bottom-up."""
    desc, maps = sh["desc"], sh["maps"]
    tab = np.full((sh["rows"], D), np.nan)
    rows_of = [t[1] for t in sh["tables"]]
    for d, rn in enumerate(lay["descriptors"]):
        (row0, U, z, node0), (map0, tiles, level, w) = desc[2 * d], desc[2 * d + 1]
        n_path, kind, rows = z & 0xffff, z >> 16, tiles * 16
        assert (U, rows, row0) == sh["tables"][d][:3] and level == rn["level"] and n_path == len(rn["path"])
        if kind == 1:                                   # a leaf with ambiguity codes: one row per distinct code
            assert w == rn["node"] < L and n_path == 0
            code = maps[map0:map0 + rows]
            assert np.all(code[U:] == code[0])          # padding rows repeat class 0
            tab[row0:row0 + rows] = _leaf_vectors(code, ambig, D) @ P[w].T
            continue
        acc, parked, e = np.ones((rows, D)), None, 0
        for k in range(n_path):
            slot, n_in, in0, flags = desc[node0 + k]
            assert slot == rn["path"][k] and flags == rn["flags"][k] and n_in == len(rn["kids"][k])
            if flags & 1:
                assert parked is None
                acc, parked = np.ones((rows, D)), acc
            for j in range(n_in):
                x, y, m0, wd = desc[in0 + j]
                assert m0 == map0 + e * rows and y == rn["kids"][k][j]
                idx = maps[m0:m0 + rows]
                assert np.all(idx[U:] == idx[0])
                if x >= 0:                               # a table: its descriptor comes earlier, on a lower level
                    cd = wd & 0xffff
                    assert cd == rn["kid_desc"][k][j] < d and lay["descriptors"][cd]["level"] < level
                    assert (wd >> 16) * 16 == rows_of[cd] and x == sh["tables"][cd][2]
                    assert np.all((0 <= idx) & (idx < rows_of[cd]))
                    acc = acc * tab[x + idx]
                else:                                    # an ordinary leaf: the column of its matrix
                    assert wd == -1 and rn["kid_desc"][k][j] == -1 and y < L and np.all((0 <= idx) & (idx < D))
                    acc = acc * P[y].T[idx]
                e += 1
            acc = acc @ P[slot].T
            if flags & 2:
                acc, parked = acc * parked, None
        assert parked is None and e == w
        tab[row0:row0 + rows] = acc
    return tab


def _run_tables_nuc(lay, sh, P, ambig, D, L):
    """... as class_table_nuc_kernel walks it: a post-order over the whole subtree, finished children on a stack."""
    desc, maps = sh["desc"], sh["maps"]
    tab = np.full((sh["rows"], D), np.nan)
    for d, rn in enumerate(lay["descriptors"]):
        (row0, U, n_path, node0), (map0, rows, _, n_in_all) = desc[2 * d], desc[2 * d + 1]
        assert (U, rows, row0) == sh["tables"][d][:3] and rn["level"] == 0
        stack, e, E = [], 0, None
        for k in range(n_path):
            slot, n_in, in0, pops = desc[node0 + k]
            acc = np.ones((rows, D))
            for j in range(n_in):
                x, leaf, _, wd = desc[in0 + j]
                code = maps[map0 + e * rows: map0 + (e + 1) * rows]
                assert x == -1 and wd == -1 and leaf < L and np.all(code[U:] == code[0])
                acc = acc * (_leaf_vectors(code, ambig, D) @ P[leaf].T)
                e += 1
            for _j in range(pops):
                acc = acc * stack.pop()
            E = acc @ P[slot].T
            if k + 1 < n_path:
                stack.append(E)
        assert not stack and e == n_in_all and len(stack) <= 8
        tab[row0:row0 + rows] = E
    return tab


def _run_trunk(lay, sh, tab, P, ambig, D, SP, nuc):
    """The root's conditionals per pattern over the view, generalised leaves read through ``ct`` / ``lt``; and the same through the
    encoded walk program where there is one."""
    v, ct, lt = lay["view"], sh["ct"], sh["lt"]
    vL, vI = v["L"], v["I"]
    j = np.arange(SP)

    def leaf(vl, x, y):
        c = ct[vl * SP + j] if nuc else ct[((j >> 4) * vL + vl) * 16 + (j & 15)]
        if x >= 0:
            d = int(lay["rep_desc_of"][v["leaf_nodes"][vl]])
            assert x == sh["tables"][d][2] and np.all((0 <= c) & (c < sh["tables"][d][0]))
            return tab[x + c]
        assert y == v["leaf_nodes"][vl]
        return _leaf_vectors(c, ambig, D) @ P[y].T

    cond = [None] * vI
    for i in range(vI):
        acc = np.ones((SP, D))
        assert list(v["children"][i]) == sorted(v["children"][i])
        for c in v["children"][i]:
            acc = acc * (leaf(c, *lt[c]) if c < vL else cond[c - vL] @ P[v["slot"][c]].T)
        cond[i] = acc
    walk = sh["walk"]
    if len(walk):
        form1, form2, depth, words = walk[0]
        assert words == len(walk) and depth <= 3

        def chain(first, n):
            acc, stack = np.ones((SP, D)), []
            for slot, n_in, in0, flags in walk[first:first + n]:
                if flags & 1:
                    stack.append(acc)
                    acc = np.ones((SP, D))
                for vl, x, y, _ in walk[in0:in0 + n_in]:
                    assert (x, y) == tuple(lt[vl])
                    acc = acc * leaf(vl, x, y)
                if slot < 0:
                    assert not stack
                    return acc
                acc = acc @ P[slot].T
                if flags & 2:
                    acc = acc * stack.pop()
            raise AssertionError("a chain must end at the root")

        assert walk[form1][0] == 1
        assert np.allclose(chain(*walk[form1 + 1][:2]), cond[vI - 1], rtol=1e-12, atol=0)
        if form2:
            assert walk[form2][0] == 2
            assert np.allclose(chain(*walk[form2 + 1][:2]) * chain(*walk[form2 + 2][:2]), cond[vI - 1], rtol=1e-12, atol=0)
    return cond[vI - 1]


def _check_layout(flat, shards, ambig, lay, D, seed=0):
    """Runs the layout of every shard and compares the root's conditionals per pattern with the plain recursion; returns the layout."""
    assert "declined" not in lay, lay
    L, fp = flat.L, np.asarray(flat.flat_parents)
    I = len(fp) - L
    nuc = D == 4
    rng = np.random.default_rng(seed)
    P = 0.9 * np.eye(D) + 0.1 * rng.random((L + I - 1, D, D))       # one matrix per branch: short branches, nothing underflows
    comp, v = lay["compressed"], lay["view"]
    assert comp.any() and not comp[I - 1]
    # the view: its slots are exactly the trunk nodes and the generalised leaves (ordinary leaves below the trunk, compressed roots)
    trunk = [L + n for n in range(I) if not comp[n]]
    gen = [c for c in range(L + I - 1) if not comp[fp[c]] and (c < L or comp[c - L])]
    assert sorted(v["slot"]) == sorted(trunk + gen) and len(set(v["slot"])) == len(v["slot"])
    assert list(v["slot"][:v["L"]]) == list(v["leaf_nodes"]) and v["I"] == len(trunk)
    children = [[] for _ in range(I)]
    for c, p in enumerate(fp[:-1]):
        children[p].append(c)
    for k, (codes, sh) in enumerate(zip(shards, lay["shards"])):
        SP = codes.shape[1]
        cond = [None] * I
        for n in range(I):
            acc = np.ones((SP, D))
            for c in children[n]:
                acc = acc * ((_leaf_vectors(codes[c], ambig, D) if c < L else cond[c - L]) @ P[c].T)
            cond[n] = acc
        tab = (_run_tables_nuc if nuc else _run_tables_mfma)(lay, sh, P, ambig, D, L)
        assert not np.isnan(tab).any()
        got = _run_trunk(lay, sh, tab, P, ambig, D, SP, nuc)
        assert np.allclose(got, cond[I - 1], rtol=1e-12, atol=0), (k, np.max(np.abs(got / cond[I - 1] - 1)))
    return lay


def _paths(lay):
    return [d for d in lay["descriptors"] if len(d["path"])]


@pytest.mark.parametrize("D,taxa,sites", [(5, 12, 64), (61, 24, 200), (20, 40, 400)])
def test_repeat_layout_inlines_side_chains_at_rho_0(D, taxa, sites):
    """rho = 0: paths run to the bottom, side chains of leaves are walked inline (flags 1 and 2)."""
    root = tree.random_tree(taxa, np.random.default_rng(taxa))
    lay = _check_layout(*_layout_case(root, D, sites, seed=taxa, rho=0.0), D)
    flags = np.concatenate([d["flags"] for d in _paths(lay)])
    assert (flags & 1).any() and (flags & 2).any()
    assert (len(lay["shards"][0]["walk"]) > 0) == (D > 16)             # (the trunk walk: two row blocks and more)


@pytest.mark.parametrize("D,taxa,sites", [(5, 16, 96), (61, 32, 256)])
def test_repeat_layout_tables_read_tables_at_rho_half(D, taxa, sites):
    root = tree.random_tree(taxa, np.random.default_rng(taxa + 1))
    lay = _check_layout(*_layout_case(root, D, sites, seed=taxa, rho=0.5), D)
    assert max(d["level"] for d in lay["descriptors"]) >= 1
    assert not any(f for d in _paths(lay) for f in d["flags"])          # (nothing is inlined unless rho is 0)


@pytest.mark.parametrize("D", [5, 61])
def test_repeat_layout_leaves_with_ambiguity_codes_get_tables_of_their_own(D):
    a = _leaves("a", 2)
    c = _leaves("c", 3)
    t = _leaves("t", 3)
    root = _node("root", _node("n3", _node("n2", _node("n1", a[0], a[1]), c[0]), c[1]), _node("n4", t[0], t[1]), t[2], c[2])
    flat, shards, ambig, lay = _layout_case(root, D, 128, seed=7, ambig_leaves=("a0", "t2"), rho=0.0)
    _check_layout(flat, shards, ambig, lay, D)
    fp, names = flat.flat_parents, flat.leaf_names
    la, lt = names.index("a0"), names.index("t2")
    assert lay["compressed"][fp[la]] and not lay["compressed"][fp[lt]]      # one below a compressed node, one below the trunk
    for leaf in (la, lt):
        d = lay["descriptors"][lay["rep_desc_of"][leaf]]
        assert d["node"] == leaf and len(d["path"]) == 0 and d["level"] == 0
    assert lt in lay["view"]["leaf_nodes"] and not lay["view"]["leaf_has_ambig"].any()


def test_repeat_layout_compresses_a_multifurcation_but_not_a_star_beyond_the_input_list():
    wide = _node("wide", *_leaves("w", 57))                                 # more children than kRepMaxInputs - 8 = 56
    four = _node("four", *_leaves("f", 4))
    root = _node("root", _node("up", wide, _node("pair", *_leaves("p", 2))), four, *_leaves("r", 2))
    flat, shards, ambig, lay = _layout_case(root, 5, 64, seed=3, p_change=0.002, rho=0.0)
    _check_layout(flat, shards, ambig, lay, 5)
    fp, names = flat.flat_parents, flat.leaf_names
    n_wide, n_four = fp[names.index("w0")], fp[names.index("f0")]
    classes, _, _ = hip.plan_repeats(fp, flat.L, shards[0], 0.9)
    assert classes[n_wide] <= 0.9 * shards[0].shape[1] and not lay["compressed"][n_wide]
    assert lay["compressed"][n_four] and sum(1 for p in fp[:flat.L] if p == n_four) == 4


def test_repeat_layout_cuts_a_caterpillar_longer_than_32_nodes():
    root = tree.caterpillar_tree(40)
    flat, shards, ambig, lay = _layout_case(root, 5, 128, seed=5, p_change=0.005, rho=0.0)
    _check_layout(flat, shards, ambig, lay, 5)
    assert lay["compressed"].sum() > 32
    assert len(_paths(lay)) >= 2 and max(len(d["path"]) for d in _paths(lay)) == 32
    assert max(d["level"] for d in lay["descriptors"]) >= 1                 # (the upper path reads the lower one's table)


def test_repeat_layout_of_two_shards_with_different_class_counts():
    root = tree.random_tree(20, np.random.default_rng(21))
    flat, shards, ambig, lay = _layout_case(root, 61, 240, seed=9, cuts=(176,), rho=0.0)
    _check_layout(flat, shards, ambig, lay, 61)
    assert [s.shape[1] for s in shards] == [176, 64] and len(lay["shards"]) == 2
    U = [[t[0] for t in sh["tables"]] for sh in lay["shards"]]
    assert U[0] != U[1] and lay["shards"][0]["rows"] != lay["shards"][1]["rows"]


def test_repeat_layout_4_states_hands_the_root_role_down_where_the_stack_is_too_small():
    """4 states: one walk per compressed subtree root on a stack of 8.  A node over five nodes over five cherries needs 4 + (4 + 1) = 9
    slots: it stays with the trunk and its children become the roots.  Ambiguity codes stay with the kernels' resolution vectors."""
    mids = [_node(f"m{i}", *[_node(f"c{i}_{j}", *_leaves(f"l{i}_{j}_", 2)) for j in range(5)]) for i in range(5)]
    deep = _node("deep", *mids)
    root = _node("root", deep, _node("pair", *_leaves("p", 2)), *_leaves("r", 2))
    flat, shards, ambig, lay = _layout_case(root, 4, 300, seed=11, ambig_leaves=("r0", "l0_0_0"))
    _check_layout(flat, shards, ambig, lay, 4)
    fp, names = flat.flat_parents, flat.leaf_names
    n_c = fp[names.index("l0_0_0")]
    n_m = fp[flat.L + n_c]
    n_deep = fp[flat.L + n_m]
    assert not lay["compressed"][n_deep] and lay["compressed"][n_m] and lay["compressed"][n_c]
    assert lay["rep_desc_of"][flat.L + n_m] >= 0 and lay["rep_desc_of"][flat.L + n_c] < 0
    d = lay["descriptors"][lay["rep_desc_of"][flat.L + n_m]]
    assert len(d["path"]) == 6 and list(d["flags"]) == [0, 0, 0, 0, 0, 5]
    assert lay["view"]["leaf_has_ambig"].sum() == 1 and len(lay["shards"][0]["walk"]) == 0


def test_repeat_layout_names_why_it_declines():
    root = tree.random_tree(12, np.random.default_rng(2))
    for D, opts, word in ((4, dict(mode=-1), "4 states"), (61, dict(mode=0), "switched off"), (61, dict(mode=1, variant=0), "workgroup-per-tile"),
                          (61, dict(mode=1), "too few patterns"), (61, dict(mode=2, theta=1e-9), "no node repeats")):
        res = _layout_case(root, D, 64, seed=1, **opts)[3]
        assert list(res) == ["declined"] and word in res["declined"], (D, opts, res)
