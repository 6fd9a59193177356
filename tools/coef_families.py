"""Coefficient blocks no forward DCT of u8 pixels produces: the inputs of the decoder
tests that stand for somebody else's bitstream (tests/test_inverse_bound.py on the CPU,
tests/test_decode_foreign_gpu.py on the device).  Every family is int16 [n, 64] in
natural (row-major) order, generated with fixed seeds; a 4-byte symbol carries any int16
and a 2-byte symbol any value in [-512, 511], whatever the plan's forward range
|q_k| <= qmax_k = round(128 L1(D_u) L1(D_v) / Q_k) (tools/inv_bound.py).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import inv_bound as IB  # noqa: E402

N_RANDOM = 4096  # one 512 x 512 plane
RANDOM = ["int16", "pm511", "range_x1", "range_x4", "range_x32", "sparse"]
FIXED = ["at_range_edge", "one_hot", "saturated"]
NAMES = RANDOM + FIXED


def qmax(quality):
    """The plan's forward range: max |q_k| over u8 blocks, [64] (half away from zero)."""
    return np.floor(IB.coef_max() / IB.quant_table(quality) + 0.5)


def zigzag_order():
    """order[k] = natural index of the k-th zigzag element (src/entropy.c:158-178)."""
    order = []
    for s in range(15):
        rows = range(min(s, 7), max(s - 7, 0) - 1, -1) if s % 2 == 0 else range(max(s - 7, 0), min(s, 7) + 1)
        order += [i * 8 + (s - i) for i in rows]
    return np.array(order)


def _pad(blocks):
    """Zero blocks up to a multiple of 64: a plane of 8k x 8 blocks."""
    blocks = np.asarray(blocks, np.int16).reshape(-1, 64)
    n = -(-blocks.shape[0] // 64) * 64
    return np.concatenate([blocks, np.zeros((n - blocks.shape[0], 64), np.int16)])


def family(name, quality, n=N_RANDOM, seed=None):
    """The family `name` for a plan of `quality` (range_*, at_range_edge depend on it)."""
    rng = np.random.default_rng(seed if seed is not None else 1000 + NAMES.index(name))
    qm = qmax(quality)
    if name == "int16":        # (a) everything a 4-byte symbol can carry
        c = rng.integers(-32768, 32768, (n, 64))
    elif name == "pm511":      # (b) the documented range of a 2-byte symbol
        c = rng.integers(-511, 512, (n, 64))
    elif name.startswith("range_x"):  # (c) s times the plan's forward range
        s = int(name[len("range_x"):])
        c = np.clip(np.round(rng.uniform(-1.0, 1.0, (n, 64)) * qm[None, :] * s), -32768, 32767)
    elif name == "sparse":     # (g) 1 to 3 nonzeros at random zigzag positions, log-uniform magnitudes
        zz = zigzag_order()
        c = np.zeros((n, 64))
        for b in range(n):
            k = rng.integers(1, 4)
            pos = rng.choice(64, k, replace=False)
            mag = np.floor(np.exp(rng.uniform(0.0, np.log(32767.0), k)) + 0.5)
            c[b, zz[pos]] = np.clip(mag, 1, 32767) * rng.choice([-1, 1], k)
    elif name == "at_range_edge":  # (d) the last value inside the forward range and the first outside
        sg = rng.choice([-1, 1], (32, 64))
        c = _pad(np.concatenate([sg[:16] * qm[None, :], sg[16:] * (qm[None, :] + 1)]))
    elif name == "one_hot":    # (e) each position alone, at both ends of int16 and at +-1
        c = np.zeros((256, 64))
        for i, v in enumerate([32767, -32768, 1, -1]):
            c[64 * i + np.arange(64), np.arange(64)] = v
    elif name == "saturated":  # (f) all +32767, all -32768, the +- checkerboard
        chk = np.where((np.arange(64) // 8 + np.arange(64) % 8) % 2 == 0, 32767, -32768)
        c = _pad([np.full(64, 32767), np.full(64, -32768), chk])
    else:
        raise KeyError(name)
    c = np.ascontiguousarray(c, np.int16).reshape(-1, 64)
    c.setflags(write=False)
    return c


def plane_shape(nblocks):
    """(H, W) in pixels of the plane the decoders fill with nblocks blocks (a multiple of 64)."""
    assert nblocks % 64 == 0
    bw = 64 if nblocks % 4096 == 0 else 16 if nblocks % 256 == 0 else 8
    return (nblocks // bw * 8, bw * 8)
