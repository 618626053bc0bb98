"""Randomised GPU stress test of the class-compressed form under the row-split walks (repeats.hip: class_table_team_kernel +
trunk_walk_kernel, one or two workgroups per tile): random trees and alignment sizes, random thresholds (the trunk from one node to most
of the tree), random state counts (codons, or a synthetic compressible partition at 2-64 states: common.compressible_case), the walk
forced or the schedule tuner left to choose the trunk's form, random sequences of full passes with new matrices, partial updates and
per-pattern evaluations — every result held to a second partition of the same data that runs the plain form.
Usage (GPU box): python tests/stress_repeats.py [n_cases] [seed0]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
from hyphy_amd import data, hip, models   # noqa: E402
from tests import common   # noqa: E402

PF = np.array([[0.3, 0.2, 0.25, 0.25], [0.2, 0.3, 0.3, 0.2], [0.25, 0.25, 0.2, 0.3]])
REV = dict(AC=0.5, AT=0.4, CG=0.4, CT=1.2, GT=0.4, AG=1.0)
LOG_SCALER = 64.0 * np.log(2.0)
t0 = time.time()
checks = walks = 0
for case in range(n_cases):
    rng = np.random.default_rng(seed0 + case)
    taxa, codons = int(rng.integers(6, 56)), int(rng.integers(300, 4000))
    theta, chains = float(rng.choice([0.05, 0.15, 0.3, 0.6, 0.9])), str(int(rng.choice([1, 2])))
    D = int(rng.choice(common.REPEAT_STATE_COUNTS + (61,)))
    tuner = bool(rng.random() < 0.3)   # (no forced form: the tuner times the trunk's candidates, the walk among them at NW >= 2)
    os.environ.update(HYPHY_HIP_REPEATS="2", HYPHY_HIP_REP_THETA=str(theta), HYPHY_HIP_TRUNK_WALK="1", HYPHY_HIP_WALK_CHAINS=chains,
                      HYPHY_HIP_POISON="1", HYPHY_HIP_REP_RHO=str(float(rng.choice([0.0, 0.0, 0.5]))))
    if tuner:
        for k in ("HYPHY_HIP_TRUNK_WALK", "HYPHY_HIP_WALK_CHAINS", "HYPHY_HIP_TUNE"):
            os.environ.pop(k, None)
    if D == 61:
        syn = data.evolve(taxa, codons, 3, seed=seed0 + case, p_change=float(rng.choice([0.02, 0.05, 0.15])))
        pd = data.from_states(syn.states, 61)
        parents, L, codes, ambig, freq = syn.flat.flat_parents, syn.flat.L, pd.leaf_codes, None, pd.pattern_freq
        pi = models.f3x4_codon_freqs(PF)
    else:
        fx = common.compressible_case(D, seed0 + case, taxa=min(taxa, 40), S=2 * (codons // 8))
        parents, L, codes, ambig, freq, pi = fx["flat_parents"], int(fx["L"]), fx["leaf_codes"], fx["ambig"], fx["pattern_freq"], fx["root_freqs"]
        rates = fx["Q"] / np.abs(fx["Q"][:, 0, 0])[:, None, None]   # (one random generator per branch, scaled by its length below)
    B = len(parents) - 1
    tmpl = models.mg94rev_template(PF)

    def Q_for(tb, omega, at=slice(None)):
        if D != 61:
            return rates[at] * (tb * omega)[:, None, None]
        Q = np.zeros((len(tb), 61, 61))
        for (i, j, name, ns, f) in tmpl:
            Q[:, i, j] = tb * REV[name] * f * (omega if ns else 1.0)
        Q[:, np.arange(61), np.arange(61)] = -Q.sum(axis=2)
        return Q

    nodes = np.arange(B, dtype=np.int64)
    tb = rng.uniform(0.01, 0.4, B)
    with hip.HipPartition(D, parents, L, codes, ambig, freq) as part, hip.HipPartition(D, parents, L, codes, ambig, freq) as plain:
        plain.set_repeats(False)
        on = part.repeat_stats()["in_use"] == 1
        Q = Q_for(tb, 0.5)
        for op in range(10):
            kind = "full" if op < 2 else str(rng.choice(["full", "full", "partial", "again"]))
            if kind == "full":
                tb = tb * rng.uniform(0.8, 1.25, B)
                Q = Q_for(tb, float(rng.uniform(0.2, 1.5)))
                un = qn = nodes
                Qs = Q
            elif kind == "partial":
                ch = np.sort(rng.choice(B, size=int(rng.integers(1, 4)), replace=False)).astype(np.int64)
                tb[ch] *= rng.uniform(0.5, 1.8)
                Q[ch] = Q_for(tb[ch], 0.7, ch)
                un = qn = ch
                Qs = Q[ch]
            else:
                un = qn = nodes
                Qs = Q
            a, la, sa = part.evaluate(un, qn, Qs, pi, per_site=True)
            b, lb, sb = plain.evaluate(un, qn, Qs, pi, per_site=True)
            assert abs(a - b) <= 1e-12 * abs(b), (case, op, kind, a, b, D, taxa, codons, theta, chains, tuner, part.schedule_info())
            d = np.max(np.abs((np.log(la) - sa * LOG_SCALER) - (np.log(lb) - sb * LOG_SCALER)))
            assert d < 1e-10, (case, op, kind, d)
            checks += 1
            walks += part.prune_kernel_name() == "trunk_walk_kernel"
        assert on or D == 61, (case, D, "nothing compressed")   # (a synthetic case compresses at any threshold)
    print(f"case {case}: {D} states, {L} taxa x {len(freq)} patterns, theta {theta}, " + ("tuner" if tuner else f"walk, chains {chains}") +
          f", compressed {on}: ok", flush=True)
print(f"{n_cases} cases, {checks} evaluations checked ({walks} of them ended in trunk_walk_kernel) in {time.time() - t0:.0f} s: all checks passed")
