"""How the seed and the site count of tests/nni_cases.py::search_case were chosen, on the CPU (``python -m tests.nni_search_check``):
with scalefree.prune as the likelihood and a coordinate-wise Newton fit of the branch lengths,
  1. the generating tree's fitted log L is above the fitted log L of each of its neighbours,
  2. hence above each neighbour's score at the generating tree's fitted lengths (printed beside it),
  3. nni.search itself, run over a CPU stand-in for the partition (scores = scalefree.prune on the neighbour tree), goes from the
     starting tree to the generating tree with a rising history.
Not a test: it takes a minute.  tests/test_gpu_nni.py::test_search_finds_the_generating_tree asserts 3 and 2 on the device."""
import numpy as np

from tests import nni_cases as nc
from tests import scalefree as sf


def logl(cs, fp, t):
    P = nc.expm_np(np.asarray(t)[:, None, None] * cs["Q"][None])
    return sf.prune(4, fp, cs["L"], cs["leaf_codes"], None, cs["pattern_freq"], P, cs["root_freqs"])["logl"]


def fit(cs, fp, t0, sweeps=40, h=1e-3):
    th = np.log(np.asarray(t0, dtype=np.float64))
    f = logl(cs, fp, np.exp(th))
    for _ in range(sweeps):
        f0 = f
        for b in range(len(th)):
            e = np.zeros_like(th)
            e[b] = h
            fp_, fm = logl(cs, fp, np.exp(th + e)), logl(cs, fp, np.exp(th - e))
            d1, d2 = (fp_ - fm) / (2 * h), (fp_ - 2 * f + fm) / h ** 2
            step = float(np.clip(-d1 / d2 if d2 < 0 else np.sign(d1), -1.0, 1.0))
            for _ in range(12):
                e[b] = step
                g = logl(cs, fp, np.exp(th + e))
                if g >= f:
                    th, f = th + e, g
                    break
                step /= 2
        if f - f0 < 1e-8:
            break
    return np.exp(th), f


class CpuPart:
    def __init__(self, cs, fp):
        self.cs, self.fp, self.t = cs, fp, None

    def nni_scores(self, moves, weights=None):
        from hyphy_amd import nni
        out = []
        for x, y in moves:
            fp2, perm = nni.apply_nni(self.fp, self.cs["L"], x, y)
            out.append(logl(self.cs, fp2, self.t[perm[:-1]]))
        return np.array(out)

    def close(self):
        pass


def main():
    from hyphy_amd import nni
    cs = nc.search_case()
    L, fp = cs["L"], cs["flat_parents"]
    B = len(fp) - 1
    t, ll = fit(cs, fp, np.full(B, 0.1))
    print(f"generating tree: fitted log L {ll:.6f} ({len(cs['pattern_freq'])} patterns)")
    worst = -np.inf
    for x, y in nc.enumerate_moves(fp, L):
        fp2, perm = nni.apply_nni(fp, L, x, y)
        score = logl(cs, fp2, t[perm[:-1]])
        _, ll2 = fit(cs, fp2, t[perm[:-1]])
        print(f"  neighbour ({x}, {y}): score {score:.6f}, fitted {ll2:.6f}, below by {ll - ll2:.4f}")
        assert score <= ll2 + 1e-9 and ll2 < ll, (x, y)
        worst = max(worst, ll2)
    print(f"the best neighbour is {ll - worst:.4f} below")

    def fit_part(part, t0):
        part.t, f = fit(cs, part.fp, t0)
        return part.t, f
    res = nni.search(lambda f: CpuPart(cs, f), fit_part, cs["start"], L, np.full(B, 0.1), restart_floor=1e-2)
    print("search history", res["history"], "moves", res["moves"])
    assert nc.splits(res["flat_parents"], L) == nc.splits(fp, L)
    assert all(b >= a for a, b in zip(res["history"], res["history"][1:])) and len(res["history"]) >= 3
    assert abs(res["logl"] - ll) < 1e-4


if __name__ == "__main__":
    main()
