"""The compressed-form cases and sequences (tests/compressed_cases.py) are what the GPU tests need them to be.  CPU only.

1  The CPU oracle (oracle/hyphy_oracle.c), given the current matrices of every step of every sequence the way
   test_scalefree_cpu.py::_oracle_site_logl does, stays within scalefree.ORACLE_MAX_REL of the replayed ``scalefree.prune``, with -inf
   in the same places: the allowance of the GPU tests (GPU_RTOL = 100 x that) holds on these cases as it stands.  Largest relative
   per-pattern deviation over all steps, printed by test_oracle_stays_within_the_allowance_at_every_step:

       8.561e-16 (D = 61, rate classes); compressed_cases.COMPRESSED_ORACLE_MAX_REL = 8.6e-16 is that rounded up

2  Exponents are in play: at the starting matrices the reference's log-magnitude at the root exceeds 64 ln 2 for at least a quarter of
   the patterns and twice that for some.
3  Every partial step of every sequence moves exponents: the log-magnitude of the parent of every changed branch moves by more than
   64 ln 2 on some pattern (possible before and after the step; where all classes go in one call, under one of them); over the main
   sequence, where each position is visited on its own, in both directions at each of the positions (a) - (f).
4  A stale table shows: with the previous matrix left on any one changed branch the reference is at least 1000 allowances of
   hold._hold away on some pattern.
5  The closed sequence opens and closes: the count of impossible patterns is positive at the start, drops at the opening step and
   rises at each closing one.
"""
import numpy as np
import pytest

from tests import compressed_cases as cc, scalefree as sf

RTOL, ATOL = sf.GPU_RTOL, 1e-9
ALL = [(D, "main") for D in cc.STATE_COUNTS] + [(D, "closed") for D in cc.CLOSED_D] + [(D, "classes") for D in cc.CLASS_D]


def _oracle_site_logl(fx, P, pi):
    from oracle import oracle
    nodes = np.arange(len(fx["flat_parents"]) - 1, dtype=np.int64)
    op = oracle.OraclePartition(int(fx["D"]), fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"])
    op.set_P(nodes, P)
    with np.errstate(divide="ignore"):
        return op.site_log_likelihoods(nodes, pi)


def _rel(got, want, what):
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


_worst = {}


def test_allowance_rests_on_the_measured_deviation():
    assert cc.COMPRESSED_ORACLE_MAX_REL <= sf.ORACLE_MAX_REL and RTOL == 100 * sf.ORACLE_MAX_REL


@pytest.mark.parametrize("D,which", ALL)
def test_oracle_stays_within_the_allowance_at_every_step(D, which):
    """1; prints the largest deviation of the sequence (the largest over all of them is the case module's figure)."""
    fx = cc.case(D)
    worst, at = 0.0, ""
    for rec in cc.replay(D, which):
        if rec["entry"] == "download":
            continue
        P, ref = rec["P"], rec["ref"]
        if P.ndim == 4:
            rel = max(_rel(_oracle_site_logl(fx, P[c], rec["pi"]), ref["class_site_logl"][c], (D, which, rec["what"], c)) for c in range(len(P)))
        else:
            rel = _rel(_oracle_site_logl(fx, P, rec["pi"]), ref["site_logl"], (D, which, rec["what"]))
        if rel > worst:
            worst, at = rel, rec["what"]
    _worst[(D, which)] = worst
    print(f"D = {D} {which}: oracle against scale-free over {len(cc.replay(D, which))} steps, largest relative deviation {worst:.3e} "
          f"at '{at}' (largest so far {max(_worst.values()):.3e})")
    assert worst <= sf.ORACLE_MAX_REL, (D, which, at, worst)
    assert worst <= cc.COMPRESSED_ORACLE_MAX_REL, (D, which, worst, "COMPRESSED_ORACLE_MAX_REL is out of date")


@pytest.mark.parametrize("D", cc.STATE_COUNTS)
def test_case_is_what_the_issue_asks_for(D):
    """The shape of the case, the positions under both thresholds, and 2."""
    fx = cc.case(D)
    L, S = int(fx["L"]), fx["leaf_codes"].shape[1]
    assert "Q" not in fx and 12 <= L <= 28 and 200 <= S <= 320
    kinds = cc.kinds_at(fx, cc.THETA_PLAN)
    for k in cc.POSITIONS:
        assert fx["pos"][k] in kinds[k], (D, k)
    assert len(set(fx["pos"].values())) == 6
    assert (fx["leaf_codes"][fx["pos"]["f"]] < 0).any()
    high = cc.kinds_at(fx, 0.9)
    at_high = {k: [h for h in cc.POSITIONS if fx["pos"][k] in high[h]] for k in cc.POSITIONS}
    assert not high["d"], (D, high["d"])                       # at 0.9 every node but the root is compressed: no trunk branch
    for rec in cc.replay(D, "main"):
        P = rec["P"]
        assert P.min() >= 0.0 and np.allclose(P.sum(axis=-1), 1.0, rtol=0, atol=1e-14), (D, rec["what"])
    root = cc.replay(D, "main")[0]["ref"]["log_mag"][-1]
    n1, n2 = int(np.sum(root < -sf.LOG_SCALER)), int(np.sum(root < -2 * sf.LOG_SCALER))
    print(f"D = {D}: seed {fx['seed']}, {L} taxa, {S} patterns, positions {fx['pos']} (at theta 0.9: {at_high}); root magnitude beyond one "
          f"step of 64 ln 2 at {n1} patterns, beyond two at {n2}, at most {-root.min() / sf.LOG_SCALER:.1f} steps")
    assert 4 * n1 >= S and n2 > 0, (D, n1, n2, S)


def _movement(fx, rec, before):
    """Per changed branch: (patterns whose parent's log-magnitude fell by more than one step, patterns where it rose)."""
    out = {}
    for code in rec["changed"]:
        x = cc.parent_log_mag(fx, before["ref"], code, rec["cls"])
        y = cc.parent_log_mag(fx, rec["ref"], code, rec["cls"])
        if x.ndim == 2:                                        # all classes in one call: any class counts
            mv = [cc.moved(x[c], y[c]) for c in range(len(x))]
            out[code] = (sum(m[0] for m in mv), sum(m[1] for m in mv))
        else:
            out[code] = cc.moved(x, y)
    return out


@pytest.mark.parametrize("D,which", ALL)
def test_every_partial_step_moves_exponents(D, which):
    """3; prints the movement per step and, for the main sequence, per position."""
    fx = cc.case(D)
    recs = cc.replay(D, which)
    by_code = {}
    for before, rec in zip(recs, recs[1:]):
        if not rec["partial"]:
            continue
        mv = _movement(fx, rec, before)
        print(f"D = {D} {which} '{rec['what']}': patterns whose parent magnitude (fell, rose) by more than 64 ln 2: {mv}")
        # every changed branch (all classes in one call: under one of the classes; the closed sequence: over the patterns possible
        # before and after the step)
        assert all(down + up > 0 for down, up in mv.values()), (D, which, rec["what"], mv)
        for code, (down, up) in mv.items():
            t = by_code.setdefault(code, [0, 0])
            t[0] += down
            t[1] += up
    if which == "main":
        for k in cc.POSITIONS:
            down, up = by_code[fx["pos"][k]]
            print(f"D = {D} position ({k}) = branch {fx['pos'][k]}: exponents raised at {down} pattern-steps, lowered at {up}")
            assert down > 0 and up > 0, (D, k, down, up)


@pytest.mark.parametrize("D,which", ALL)
def test_a_stale_table_shows(D, which):
    """4."""
    fx = cc.case(D)
    least = np.inf
    for rec in cc.replay(D, which):
        if not rec["partial"]:
            continue
        cls = rec["cls"]
        want = rec["ref"]["site_logl"] if cls is None else rec["ref"]["class_site_logl"][cls]
        for code in rec["changed"]:
            P = rec["P"].copy()
            if P.ndim == 4 and cls is None:
                P[:, code] = rec["prev"][:, code]
                stale = cc._prune(fx, P, rec["pi"], weights=cc.CLASS_WEIGHTS)["site_logl"]
            elif P.ndim == 4:
                P[cls][code] = rec["prev"][cls][code]
                stale = cc._prune(fx, P[cls], rec["pi"])["site_logl"]
            else:
                P[code] = rec["prev"][code]
                stale = cc._prune(fx, P, rec["pi"])["site_logl"]
            if (np.isneginf(stale) != np.isneginf(want)).any():
                continue                                        # a pattern possible on one side only: as far away as can be
            fin = np.isfinite(want)
            ratio = float(np.max(np.abs(stale[fin] - want[fin]) / (RTOL * np.abs(want[fin]) + ATOL)))
            least = min(least, ratio)
            assert ratio >= 1000.0, (D, which, rec["what"], code, ratio)
    print(f"D = {D} {which}: a stale branch is at least {least:.3g} allowances away")


@pytest.mark.parametrize("D", cc.CLOSED_D)
def test_closed_sequence_opens_and_closes(D):
    """5."""
    recs = cc.replay(D, "closed")
    dead = [int(np.sum(np.isneginf(r["ref"]["site_logl"]))) for r in recs]
    print(f"D = {D} closed: impossible patterns per step {dead}; branches (x, z, y) {cc.closed_branches(D)[:3]}")
    names = [r["what"].split(" [")[0] for r in recs]
    assert dead[0] > 0 and dead[1] > 0
    assert dead[names.index("3 open x")] < dead[1]
    assert dead[names.index("5 close x")] > dead[names.index("4 y stays closed")]
    assert dead[names.index("7 open x, y, z")] < dead[names.index("6 again")]
    assert dead[names.index("8 close z")] > dead[names.index("7 open x, y, z")]
    assert all(d < len(recs[0]["ref"]["site_logl"]) for d in dead)
