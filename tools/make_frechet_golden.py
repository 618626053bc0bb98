#!/usr/bin/env python3
"""Writes tests/golden/frechet_adjoint_D{D}.npz for the state counts at which tests/grad_cases.frechet_ref (192-bit fixed point on
Python integers) takes seconds per matrix: S [kinds, n, D, D] = L(Q^T, W) of grad_cases.adjoint_cases(D), rounded to float64.
The inputs are not stored: the test regenerates them from the seed and checks them against the stored checksum."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import grad_cases as gc  # noqa: E402


def main(sizes):
    for D in sizes:
        cases = gc.adjoint_cases(D)
        S = np.stack([np.stack([gc.frechet_ref(q, w) for q, w in zip(Q, W)]) for _, Q, W in cases])
        check = np.array([float(np.sum(Q)) + float(np.sum(W)) for _, Q, W in cases])
        path = os.path.join(os.path.dirname(os.path.abspath(gc.__file__)), "golden", f"frechet_adjoint_D{D}.npz")
        np.savez(path, S=S, check=check)
        print(path, S.shape)


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or gc.GOLDEN_D)
