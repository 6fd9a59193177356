"""Rigorous error bound of the fp32 inverse DCT of the fused round trip
(roundtrip.hip, inverse_block_f32): generates dct_amd/csrc/idct8_bound.h.

The kernel computes, per block, x_uv = fl32(q_uv * s_uv) with s_uv =
fl32(dequant_uv * S_u * S_v) (the plan's fp32 inverse scale; dequant = 1/Q,
the reference's bug-compatible non-adaptive dequantisation,
src/quantization.c:139,144), the transposed AAN graph over each column u, then
over each row (tools/aan_model.py aan8t), and recon = fl32(y + 128).

Every value is tracked as a linear form L over the 64 exact inputs x_k plus an
error bound that is itself LINEAR in the per-input magnitude bounds B_k
(|x_k| <= B_k): e = g . B.  Each fp32 add/sub/mul/fma charges one rounding
u * (|L| . B + e) (u = 2^-24; a fused op has one rounding fewer, so charging
every op also covers contraction); a constant charges its fp32 representation
error; each input starts with 2u + 4u^2 of B_k (the two roundings of the scale
and of the product).  Hence, per output pixel ij,

    |y_ij computed - y_ij exact| <= G[ij] . B          (kInvErrG)
    |y_ij exact|                 <= A[ij] . B          (kInvAbsL: |L|)

and the host (plan_tables.hip) admits a non-adaptive plan to the fp32 inverse iff,
with B_k = max|q_k| * dequant_k * S_u S_v from the plan's Q table,

    max_ij (G[ij].B (1 + u) + u (128 + A[ij].B)) + 1e-9  <=  kInvTol

(the last rounding is the +128; 1e-9 covers the reference's own fp64 error,
~1e-12).  kInvTol = 5e-5 leaves half of north_star's 1e-4 as margin.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
from aan_model import aan8t, scales  # noqa: E402

U = 2.0 ** -24
F32 = lambda k: float(np.float32(k))  # noqa: E731


class Val:
    __slots__ = ("L", "g")

    def __init__(s, L, g):
        s.L, s.g = L, g


class Track:
    """Linear forms with error bounds linear in B (g . B)."""

    def _r(s, L, g):  # one rounding of a result with form L and incoming error g
        return Val(L, g + U * (np.abs(L) + g))

    def add(s, a, b):
        return s._r(a.L + b.L, a.g + b.g)

    def sub(s, a, b):
        return s._r(a.L - b.L, a.g + b.g)

    def neg(s, a):
        return Val(-a.L, a.g)  # exact

    def mul(s, a, k):
        kt = F32(k)
        return s._r(a.L * k, a.g * abs(kt) + np.abs(a.L) * abs(kt - k))

    def fma(s, k, a, b):
        kt = F32(k)
        return s._r(a.L * k + b.L, a.g * abs(kt) + np.abs(a.L) * abs(kt - k) + b.g)


def bound():
    T = Track()
    eye = np.eye(64)
    X = [[Val(eye[u * 8 + v].copy(), (2 * U + 4 * U * U) * eye[u * 8 + v]) for v in range(8)] for u in range(8)]
    cols = [aan8t([X[u][v] for u in range(8)], T) for v in range(8)]    # cols[v][i]
    rows = [aan8t([cols[v][i] for v in range(8)], T) for i in range(8)]  # rows[i][j]
    G = np.array([[rows[i][j].g for j in range(8)] for i in range(8)]).reshape(64, 64)
    L = np.array([[rows[i][j].L for j in range(8)] for i in range(8)]).reshape(64, 64)
    return G, L


def check_linear(L):
    """y_ij = sum_uv D[u][i] D[v][j] X_uv with x_uv = S_u S_v X_uv (src/dct.c:80-105)."""
    S = np.array(scales())
    n = 8
    D = np.array([[(1 / math.sqrt(n) if i == 0 else math.sqrt(2 / n)) * math.cos(math.pi * (2 * j + 1) * i / (2 * n))
                   for j in range(n)] for i in range(n)])
    for i in range(8):
        for j in range(8):
            want = np.outer(D[:, i], D[:, j]).ravel() / np.outer(S, S).ravel()
            assert np.allclose(L[i * 8 + j], want, atol=1e-12), (i, j)


STD = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]  # src/quantization.c:8-17


def quant_table(q):
    """src/quantization.c:51-77 (8x8)."""
    q = min(max(q, 1), 100)
    s = (5000.0 / q if q < 50 else 200.0 - 2 * q) / 100.0
    return np.array([min(max(v * s, 1.0), 255.0) for v in STD])


def coef_max():
    """max |c_uv| over centred blocks x in [-128, 127]: 128 * L1(D[u]) * L1(D[v])."""
    n = 8
    D = np.array([[(1 / math.sqrt(n) if i == 0 else math.sqrt(2 / n)) * math.cos(math.pi * (2 * j + 1) * i / (2 * n))
                   for j in range(n)] for i in range(n)])
    l1 = np.abs(D).sum(axis=1)
    return 128.0 * np.outer(l1, l1).ravel()


def plan_error(q, G, L, tol=5e-5):
    Q = quant_table(q)
    S = np.array(scales())
    qmax = np.floor(coef_max() / Q + 0.5)  # |round(c / Q)| (half away from zero)
    B = qmax * (1.0 / Q) * np.outer(S, S).ravel()
    e = (G @ B) * (1 + U) + U * (128.0 + np.abs(L) @ B) + 1e-9
    return float(e.max()), float((np.abs(L) @ B).max())


def block_magnitudes(coef, dequant):
    """x_k = |q_k| * dequant_k * S_u S_v per block: the inverse's exact input magnitudes,
    [n, 64], of int blocks coef [n, 64] under the dequantisation multipliers dequant
    ([64], or [n, 64] for the per-block multipliers of adaptive plans)."""
    S = np.array(scales())
    return np.abs(np.asarray(coef, np.float64)) * np.asarray(dequant, np.float64) * np.outer(S, S).ravel()


def block_error(q, coef, G, L):
    """The bound of plan_error evaluated at each block's ACTUAL magnitudes instead of
    the plan's forward range: e [n, 64], |fp32 recon - reference| <= e[b, p] for pixel p
    of block b of ANY int coefficients coef [n, 64] decoded by the non-adaptive plan of
    quality q.  Linear in the magnitudes, so it is below plan_error for every block
    inside the forward range and grows in proportion outside it."""
    x = block_magnitudes(coef, 1.0 / quant_table(q))
    return (x @ G.T) * (1 + U) + U * (128.0 + x @ np.abs(L).T) + 1e-9


def header(G, L):
    fmt = lambda a: ",\n    ".join(", ".join("%.17g" % x for x in row) for row in a)  # noqa: E731
    return f"""// GENERATED by tools/inv_bound.py -- do not edit.
// Rigorous error bound of the round trip's fp32 inverse DCT (DESIGN.md 3.7): for
// inputs x_k = fl32(q_k * s_k) with |x_k exact| <= B_k, output pixel p = 8i + j has
//   |y_p computed - y_p exact| <= sum_k kInvErrG[p][k] * B_k,   |y_p exact| <= sum_k kInvAbsL[p][k] * B_k.
#pragma once
constexpr double kInvTol = 5e-5;  // admitted plans: bound of |recon - reference| (north_star: 1e-4)
static const double kInvErrG[64][64] = {{
    {fmt(G)}}};
static const double kInvAbsL[64][64] = {{
    {fmt(np.abs(L))}}};
"""


if __name__ == "__main__":
    G, L = bound()
    check_linear(L)
    for q in (10, 25, 50, 75, 80, 85, 90, 95, 100):
        e, m = plan_error(q, G, L)
        print(f"q{q:3d}: bound {e:.3e}  max|y| {m:8.2f}  {'fp32' if e <= 5e-5 else 'fp64'}")
    ok = [q for q in range(1, 101) if plan_error(q, G, L)[0] <= 5e-5]
    print("fp32 plans:", ok[0] if ok else None, "..", ok[-1] if ok else None, len(ok))
    out = sys.argv[1] if len(sys.argv) > 1 else None
    if out:
        open(out, "w").write(header(G, L))
