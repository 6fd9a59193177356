"""The reduced-size decode, stated in plain numpy (CPU only): the pixels
dctq_decode_bits_window_scaled_planes writes, from the quantized coefficients of the blocks.

Scale s in {2, 4, 8}, n = 8 / s: every stored 8 x 8 block gives n x n pixels, from its
coefficients q[u][v] with u, v < n.  Everything is IEEE fp64, every multiply and add rounded
separately (numpy's elementwise * and + on float64 arrays do exactly that: no fma), sums left
to right in ascending index.  Q is the plan's quantization table (8 x 8 float64).

    dequantize   non-adaptive:  x = q * (1.0 / Q)               (the multiplication by 1 / Q of
                                                                 every decoder of this library)
                 adaptive:      sc = 2.0 - min(1.0, max(0.1, (var_num / 4096.0) / 1000.0))
                                x = (q * Q) * sc,  x[0][0] = q[0][0] * Q[0][0]
    temp[u][j] = sum over v of x[u][v] * Dn[v][j]
    out[i][j]  = sum over u of Dn[u][i] * temp[u][j]
    R          = out[i][j] * (n / 8.0) + 128.0
    pixel      = uint8(rint(min(max(R, 0.0), 255.0))),  ties to even

Dn is the n-point DCT matrix as the literals below, never through cos (libm results differ in
the last place).  For s = 8 a pixel is the dequantized DC / 8 + 128: the block's mean.

    dequantize(q, Q, n, adaptive, var_num) -> x      float64 [N, n, n]
    unrounded(q, Q, scale, adaptive, var_num) -> R   float64 [N, n, n]
    blocks(q, Q, scale, adaptive, var_num) -> uint8 [N, n, n]
    planes(coef, shapes, Q, scale, adaptive, var_nums, windows) -> per plane uint8
                                                     [f1 - f0, (y1 - y0) / s, (x1 - x0) / s]

    python tools/scaled_ref.py     # a worked example
"""
import numpy as np

SCALES = (2, 4, 8)
_r = float.fromhex("0x1.6a09e667f3bcdp-1")
_h, _a, _b = 0.5, float.fromhex("0x1.4e7ae9144f0fcp-1"), float.fromhex("0x1.1517a7bdb3896p-2")
D = {
    1: np.array([[1.0]]),
    2: np.array([[_r, _r], [_r, -_r]]),
    4: np.array([[_h, _h, _h, _h], [_a, _b, -_b, -_a], [_h, -_h, -_h, _h], [_b, -_a, _a, -_b]]),
}


def _corner(q, n):
    q = np.asarray(q)
    if q.dtype != np.int16 or q.size % 64:
        raise ValueError("coefficients must be int16 blocks of 64")
    return q.reshape(-1, 8, 8)[:, :n, :n].astype(np.float64)


def dequantize(q, Q, n, adaptive, var_num=None):
    """x [N, n, n] of int16 blocks q [N, 64] (natural order)."""
    c = _corner(q, n)
    Q = np.asarray(Q, dtype=np.float64).reshape(8, 8)[:n, :n]
    if not adaptive:
        return c * (1.0 / Q)
    if var_num is None:
        raise ValueError("an adaptive plan needs var_num")
    vn = np.asarray(var_num).reshape(-1).astype(np.float64)
    if len(vn) != len(c):
        raise ValueError("one var_num per block")
    sc = 2.0 - np.minimum(1.0, np.maximum(0.1, (vn / 4096.0) / 1000.0))
    t = c * Q
    x = t * sc[:, None, None]
    x[:, 0, 0] = t[:, 0, 0]
    return x


def unrounded(q, Q, scale, adaptive, var_num=None):
    """R [N, n, n]: the pixels before the clamp and the rounding."""
    if scale not in SCALES:
        raise ValueError("scale must be 2, 4 or 8")
    n = 8 // scale
    x, d = dequantize(q, Q, n, adaptive, var_num), D[n]
    temp = np.empty_like(x)
    for u in range(n):
        for j in range(n):
            s = x[:, u, 0] * d[0, j]
            for v in range(1, n):
                s = s + x[:, u, v] * d[v, j]
            temp[:, u, j] = s
    out = np.empty_like(x)
    for i in range(n):
        for j in range(n):
            s = d[0, i] * temp[:, 0, j]
            for u in range(1, n):
                s = s + d[u, i] * temp[:, u, j]
            out[:, i, j] = s
    return out * (n / 8.0) + 128.0


def blocks(q, Q, scale, adaptive, var_num=None):
    """The n x n pixels of every block: uint8 [N, n, n]."""
    r = unrounded(q, Q, scale, adaptive, var_num)
    return np.rint(np.minimum(np.maximum(r, 0.0), 255.0)).astype(np.uint8)


def planes(coef, shapes, Q, scale, adaptive, var_nums=None, windows=None):
    """The reduced pictures of a stream's planes.  coef: int16 [N, 64], the blocks of the stored
    planes shapes[k] = (F, H, W) one plane after the other, in raster order; var_nums[k]: the
    stored plane's; windows[k] = ((f0, f1), (y0, y1), (x0, x1)) in stored pixels, multiples of
    8 (None: the whole planes)."""
    coef = np.asarray(coef).reshape(-1, 64)
    n = 8 // scale
    res, first = [], 0
    for k, (f, h, w) in enumerate(shapes):
        bh, bw = h // 8, w // 8
        nb = f * bh * bw
        vn = None if not adaptive else np.asarray(var_nums[k]).reshape(-1)[:nb]
        px = blocks(coef[first:first + nb], Q, scale, adaptive, vn)
        pic = px.reshape(f, bh, bw, n, n).transpose(0, 1, 3, 2, 4).reshape(f, bh * n, bw * n)
        if windows is not None:
            (f0, f1), (y0, y1), (x0, x1) = windows[k]
            if any(v % 8 for v in (y0, y1, x0, x1)):
                raise ValueError("window rows and columns must be multiples of 8")
            pic = pic[f0:f1, y0 // scale:y1 // scale, x0 // scale:x1 // scale]
        res.append(np.ascontiguousarray(pic))
        first += nb
    if first != len(coef):
        raise ValueError(f"{len(coef)} blocks, the shapes hold {first}")
    return res


if __name__ == "__main__":
    rng = np.random.default_rng(1)
    Q = np.full((8, 8), 16.0)
    q = np.zeros((1, 64), np.int16)
    q[0, :4] = rng.integers(-40, 40, 4)
    q[0, 8:12] = rng.integers(-20, 20, 4)
    for s in SCALES:
        print(f"scale {s}:\n{blocks(q, Q, s, True, [4096 * 500])[0]}")
