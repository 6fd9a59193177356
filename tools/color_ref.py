"""The colour transform of dctq_rgb_to_ycbcr_planes / dctq_ycbcr_to_rgb_planes in plain numpy.

Full-range BT.601 (JFIF) in 16-bit fixed point.  Everything is int64 here; every intermediate
fits int32, which is what the kernels use.  >> is an arithmetic shift (floor).  This file is the
definition and the tests' yardstick: the kernels are held to it byte for byte.

    forward(rgb, "420" | "444") -> (y, cb, cr)     rgb u8 [..., H, W, 3]
    inverse(y, cb, cr)          -> rgb             subsampling read from the shapes

Pictures of any size (dctq_rgb_to_ycbcr_pad_planes / dctq_ycbcr_to_rgb_crop_planes): with m = 8
("444") or 16 ("420") the picture is extended to the next multiples of m by edge replication,
pixel'(x, y) = pixel(min(x, W - 1), min(y, H - 1)); forward runs on the extended picture; the way
back runs inverse on the extended planes and keeps the pixels with x < W and y < H.

    pad_edge(a, m)                       -> a, its axes -3 and -2 (H, W of [..., H, W, C]) extended
    forward_padded(rgb, "420" | "444")   -> forward(pad_edge(rgb, m))
    inverse_cropped(y, cb, cr, H, W)     -> inverse(y, cb, cr)[..., :H, :W, :]
"""
import numpy as np


def ycc_pixels(rgb):
    """Per pixel, no subsampling, NO clamp: (Y, Cb, Cr) as int64 arrays shaped rgb.shape[:-1]."""
    r, g, b = (np.asarray(rgb)[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def subsample(c):
    """[..., H, W] -> [..., H/2, W/2]: (c00 + c01 + c10 + c11 + 2) >> 2 over each 2x2."""
    c = np.asarray(c).astype(np.int64)
    return (c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2] + 2) >> 2


def forward(rgb, subsampling="420"):
    y, cb, cr = ycc_pixels(rgb)
    for p in (y, cb, cr):  # true for every colour (test_color_cpu checks all 2^24)
        assert p.min() >= 0 and p.max() <= 255
    if subsampling == "420":
        cb, cr = subsample(cb), subsample(cr)
    elif subsampling != "444":
        raise ValueError(subsampling)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def rgb_pixels(y, cb, cr):
    """Per pixel, equal shapes, BEFORE the clamp: (R, G, B) as int64."""
    y = np.asarray(y).astype(np.int64)
    cb, cr = np.asarray(cb).astype(np.int64) - 128, np.asarray(cr).astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return r, g, b


def inverse(y, cb, cr):
    """u8 planes [..., H, W] and chroma of the same size or half of it -> u8 [..., H, W, 3]."""
    y, cb, cr = np.asarray(y), np.asarray(cb), np.asarray(cr)
    if cb.shape != y.shape:  # 4:2:0: nearest neighbour, each sample to its 2x2 pixels
        assert cb.shape == cr.shape == y.shape[:-2] + (y.shape[-2] // 2, y.shape[-1] // 2)
        cb, cr = (c.repeat(2, axis=-2).repeat(2, axis=-1) for c in (cb, cr))
    return np.clip(np.stack(rgb_pixels(y, cb, cr), axis=-1), 0, 255).astype(np.uint8)


def pad_edge(a, m):
    """[..., H, W, C] -> [..., ceil(H / m) m, ceil(W / m) m, C] by edge replication, written as the
    definition's index clamp (not np.pad)."""
    a = np.asarray(a)
    h, w = a.shape[-3], a.shape[-2]
    if h < 1 or w < 1:
        raise ValueError("a picture needs at least one pixel")
    ys = np.minimum(np.arange(-(-h // m) * m), h - 1)
    xs = np.minimum(np.arange(-(-w // m) * m), w - 1)
    return a[..., ys[:, None], xs[None, :], :]


def forward_padded(rgb, subsampling="420"):
    if subsampling not in ("420", "444"):
        raise ValueError(subsampling)
    return forward(pad_edge(rgb, 16 if subsampling == "420" else 8), subsampling)


def inverse_cropped(y, cb, cr, H, W):
    """The inverse over the whole extended planes, then the crop: u8 [..., H, W, 3]."""
    return np.ascontiguousarray(inverse(y, cb, cr)[..., :H, :W, :])


def all_colours():
    """u8 [4096, 4096, 3]: every colour once, pixel (i, j) = colour number 4096 i + j
    (R the high byte, B the low one)."""
    n = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(n >> 16) & 255, (n >> 8) & 255, n & 255], axis=-1).astype(np.uint8)
