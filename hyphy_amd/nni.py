"""Nearest-neighbour interchanges on rooted trees in the library's numbering (``flat_parents[c]`` = internal index of c's parent,
leaves 0 .. L-1, internal node i has code L + i, children before parents, the root last with -1).

A move (x, y): c = parent(x) is an internal node other than the root and y a sibling of c; x and y exchange parents
(``hip.plan_nni`` lists every move of a tree, ``HipPartition.nni_scores`` gives the log-likelihood of every neighbour from one outside
pass).  ``apply_nni`` writes the neighbour tree down in the same numbering; ``search`` is a hill-climb over topologies on top of
both — the counterpart of the reference's doNNISwap.bf loop, with one device call per round where that loop evaluates per swap.
"""
from __future__ import annotations

import numpy as np


def apply_nni(flat_parents, L: int, x: int, y: int):
    """The tree in which ``x`` and ``y`` have exchanged parents: ``(new_flat_parents, perm)`` with ``perm[new code] = old code``.
    Leaves keep their codes and internal nodes their order, except that c = parent(x) moves to just behind y when y is an internal
    node numbered above c (c becomes y's parent, and children come before parents).  Whatever belongs to a branch follows as
    ``P_new = P_old[perm[:-1]]``."""
    fp = np.asarray(flat_parents, dtype=np.int64)
    L, x, y = int(L), int(x), int(y)
    n = len(fp)
    root = n - 1
    if not (0 <= x < root and 0 <= y < root):
        raise ValueError(f"({x}, {y}): not the codes of two branches")
    c = L + int(fp[x])
    if c == root:
        raise ValueError(f"({x}, {y}): the parent of x is the root")
    if y == c or fp[y] != fp[c]:
        raise ValueError(f"({x}, {y}): y is not a sibling of the parent of x")
    parent = [L + int(q) if q >= 0 else -1 for q in fp]          # old node code of every node's parent
    parent[x], parent[y] = parent[y], parent[x]
    internal = list(range(L, n))
    if y > c:
        internal.remove(c)
        internal.insert(internal.index(y) + 1, c)
    perm = np.array(list(range(L)) + internal, dtype=np.int64)
    new_of = np.empty(n, dtype=np.int64)
    new_of[perm] = np.arange(n)
    new_fp = np.array([new_of[parent[old]] - L if parent[old] >= 0 else -1 for old in perm], dtype=np.int64)
    return new_fp, perm


def search(make_partition, fit, flat_parents, L: int, lengths, weights=None, n_candidates: int = 3, max_rounds: int = 50,
           restart_floor: float = 0.0):
    """Hill-climb over rooted topologies by nearest-neighbour interchanges.

    ``make_partition(flat_parents) -> HipPartition`` builds a partition on a tree; ``fit(part, lengths) -> (lengths, logL)`` fits the
    branch lengths on it from a starting point and must leave the partition evaluated at the lengths it returns
    (``brlen.fit_branch_lengths`` over ``brlen.partition_callables(part, ...)``, then one more ``evaluate`` at the result, is the
    intended one).  ``lengths``: [B] starting lengths of ``flat_parents``' branches; ``weights``: class weights when C > 1.

    Each round scores every move of the current tree in one ``nni_scores`` call, rebuilds the partition on each of the
    ``n_candidates`` best-scoring neighbours with a finite score, re-fits the lengths there from the current ones, carried along
    with their branches, and moves to the best of them if its log L is above the current one; otherwise it stops.
    ``restart_floor`` (default 0: off, ``fit`` gets the current lengths as they are): lengths below it are raised to it before a
    re-fit.  On a wrong topology the central branch tends to collapse; all neighbours around a collapsed branch are one tree, and a
    fit in the logarithm of the lengths (``brlen.fit_branch_lengths``) does not leave a collapsed branch, so with such a fit a small
    positive floor (1e-2, say) is what lets a candidate show its gain.
    Returns a dict: ``flat_parents``, ``lengths``, ``logl``, ``history`` (log L at the start and after every accepted move) and
    ``moves`` (the accepted (x, y), each in the numbering of the tree it was applied to)."""
    from . import hip
    L = int(L)
    fp = np.asarray(flat_parents, dtype=np.int64).copy()
    part = make_partition(fp)
    best = None                                            # (partition, tree, lengths, log L, move) of the round's best candidate
    accepted = []
    try:
        t, ll = fit(part, np.asarray(lengths, dtype=np.float64))
        history = [float(ll)]
        for _ in range(max_rounds):
            moves = hip.plan_nni(fp, L)
            if not len(moves):
                break
            scores = part.nni_scores(moves, weights)
            order = [int(k) for k in np.argsort(-scores, kind="stable")[:n_candidates] if np.isfinite(scores[k])]
            for k in order:                                # (a move that makes a pattern impossible, or a NaN, is not rebuilt)
                fp2, perm = apply_nni(fp, L, *moves[k])
                part2 = make_partition(fp2)
                try:
                    t2, ll2 = fit(part2, np.maximum(np.asarray(t)[perm[:-1]], restart_floor))
                except BaseException:
                    part2.close()
                    raise
                if ll2 > ll and (best is None or ll2 > best[3]):
                    if best is not None:
                        best[0].close()
                    best = (part2, fp2, t2, float(ll2), k)
                else:
                    part2.close()
            if best is None:
                break
            part.close()
            part, fp, t, ll = best[:4]
            accepted.append((int(moves[best[4]][0]), int(moves[best[4]][1])))
            history.append(ll)
            best = None
        return dict(flat_parents=fp, lengths=np.asarray(t), logl=float(ll), history=history, moves=accepted)
    finally:
        if best is not None:                               # (a fit raised while an earlier candidate of the round was held)
            best[0].close()
        part.close()
