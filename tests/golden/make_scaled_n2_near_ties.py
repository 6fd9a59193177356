"""Writes tests/golden/scaled_n2_near_ties.npy: 256 corners (0,0), (0,1), (1,0), (1,1) (int16 [256, 4]) of
blocks whose 1/4-size pixel, by the definition of tools/scaled_ref.py with Q = 1, is as near to k + 0.5 as
fp64 gets without being it -- 128 from below, 128 from above.  The 2-point matrix is the literal
r = 0x1.6a09e667f3bcdp-1, r * r != 0.5, so a corner whose sum is 8 k - 1020 (an exact tie in real numbers)
lands a few ulp off the half, on the side its roundings take it.

    python tests/golden/make_scaled_n2_near_ties.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tools"))
import scaled_ref  # noqa: E402


def search(seed=5, n=200000):
    rng = np.random.default_rng(seed)
    abc = rng.integers(-300, 301, (n, 3))
    k = rng.integers(1, 254, n)
    corner = np.concatenate([(8 * k - 1020 - abc.sum(axis=1))[:, None], abc], axis=1)  # pixel (0, 0): the sum
    coef = np.zeros((n, 64), np.int16)
    coef[:, [0, 1, 8, 9]] = corner
    R = scaled_ref.unrounded(coef, np.ones((8, 8)), 4, False)[:, 0, 0]
    d = R - np.floor(R) - 0.5
    ok = (R > 0.0) & (R < 255.0) & (d != 0.0)
    below = np.flatnonzero(ok & (d < 0))
    above = np.flatnonzero(ok & (d > 0))
    pick = np.concatenate([below[np.argsort(-d[below], kind="stable")[:128]],
                           above[np.argsort(d[above], kind="stable")[:128]]])
    return corner[pick].astype(np.int16), d[pick]


if __name__ == "__main__":
    corner, d = search()
    print(f"{len(corner)} corners, |R - (k + 0.5)| from {np.abs(d).min():.3e} to {np.abs(d).max():.3e}")
    np.save(os.path.join(HERE, "scaled_n2_near_ties.npy"), corner)
