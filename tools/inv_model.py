"""Operation-for-operation numpy model of the decoders' fp32 inverse
(dct_amd/csrc/inverse_core.h inverse_half_f32_rows): x_uv = fl32(q_uv * s_uv), the
transposed AAN graph (tools/aan_model.py aan8t) over the columns then the rows, + 128,
every operation rounded to fp32 exactly as the hardware rounds it.  The sequence
tools/inv_bound.py bounds; the CPU bound test and the GPU foreign-coefficient tests
compare it with the oracle and, bit for bit, with the kernel.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
from aan_model import aan8t, scales  # noqa: E402


def round_odd_sum(p, b):
    """p + b for fp64 arrays, rounded to ODD: the exact sum when fp64 holds it, else the
    one of its two fp64 neighbours whose last mantissa bit is set.  A later rounding to
    fp32 (53 >= 2 * 24 + 2 bits) then equals a single rounding of the exact sum."""
    s = p + b
    bb = s - p
    e = (p - (s - bb)) + (b - bb)  # TwoSum: p + b = s + e exactly
    toward = np.where(e > 0, np.inf, -np.inf)
    even = (s.view(np.int64) & 1) == 0
    return np.where((e != 0) & even, np.nextafter(s, toward), s)


class F32:
    """The kernel's fp32 arithmetic on numpy arrays: every op rounded once to fp32.
    add / sub / mul of two fp32 values are exact in fp64 or round the same way twice
    (53 >= 2 * 24 + 2); fma(k, a, b) = fl32(k * a + b): the product is exact in fp64 (48
    bits), the sum is rounded to odd before the rounding to fp32, so no double rounding."""
    f = staticmethod(np.float32)

    def add(self, a, b): return (a + b).astype(np.float32)
    def sub(self, a, b): return (a - b).astype(np.float32)
    def neg(self, a): return -a
    def mul(self, a, k): return (a * np.float32(k)).astype(np.float32)

    def fma(self, k, a, b):
        p = np.float64(np.float32(k)) * a.astype(np.float64)
        return round_odd_sum(p, b.astype(np.float64)).astype(np.float32)


def iscale32(dequant):
    """The plan's fp32 inverse scale fl32(dequant_uv * S_u * S_v) from the fp64 dequantisation
    table [64] (non-adaptive: 1/Q, src/quantization.c:139,144)."""
    S = np.array(scales())
    return (np.asarray(dequant, np.float64).ravel() * np.outer(S, S).ravel()).astype(np.float32)


def kernel_inverse(q, scale32):
    """fp32 recon [n, 64] of int coefficient blocks q [n, 64] as inverse_half_f32_rows computes it."""
    A = F32()
    x = (q.astype(np.float32) * scale32[None, :]).astype(np.float32)
    x = [x[:, k] for k in range(64)]
    for v in range(8):
        col = aan8t([x[u * 8 + v] for u in range(8)], A)
        for i in range(8):
            x[i * 8 + v] = col[i]
    for i in range(8):
        row = aan8t(x[i * 8:i * 8 + 8], A)
        x[i * 8:i * 8 + 8] = row
    return np.stack([(xx + np.float32(128.0)).astype(np.float32) for xx in x], axis=1)


def pixels_of(recon):
    """The decoders' u8 pixel of an fp32 recon: rne(clamp(r, 0, 255)) (decode_core.h pack_u8x4)."""
    return np.rint(np.clip(recon, np.float32(0.0), np.float32(255.0))).astype(np.uint8)
