"""GPU: the decoders on coefficients no forward of ours produced (dctq_decode_planes,
dctq_decode_symbols_planes, dctq_inverse fed as somebody else's bitstream would feed
them): tools/coef_families.py -- any int16, +-511, multiples of the plan's forward range,
the range's edge, one-hot, saturated and sparse blocks -- and var_num the caller made up.

Bounds (include/dct_amd.h).  A pixel is rne(clamp(r, 0, 255)) of an fp32 recon r.
  * fp32 plans (non-adaptive, q <= 71): |r - reference| <= e_p(block), the plan's bound
    evaluated at the block's own magnitudes (tools/inv_bound.py block_error), and r is,
    bit for bit, tools/inv_model.py -- the operation order the bound is proved for.
  * fp64 plans (the others) and dctq_inverse (always fp64): one rounding to fp32 of a
    value whose fp64 error is the project's 1e-9 allowance scaled with the input (the
    arithmetic is linear): e_p = 2^-24 max(|reference|, 128) + 1e-9 max(1, sum_k x_k / 1024),
    x_k = |q_k| m_k S_u S_v with m_k the multiplier the reference dequantises with (1/Q_k;
    adaptive: Q_k (2 - nv), DC Q_0, src/quantization.c:137,144,193,198).
Clamping does not increase a distance and rounding moves a value by at most 0.5, so
|pix - clip(reference, 0, 255)| <= 0.5 + e_p, and the clamp is exact beyond e_p.

In-range shares (pixels with 0 < reference < 255, where a rounding check means
something), measured on the CPU for the random families int16 / pm511 / range_x1 /
range_x4 / range_x32 / sparse, in per cent (test_pixels_against_oracle prints them):
    (1,0)    91.4  100   100   100   100   100
    (50,0)   14.1  100   100   100    99.2  96.5
    (71,0)    8.2  100   100   100    65.8  93.1
    (72,0)    7.9  100   100   100    62.4  92.8
    (100,0)   0.5   33.3  19.6   4.9   0.6  51.6
    (50,1)    0.0    0.4  16.7   4.1   0.5  14.7
    (100,1)   0.5   28.5  16.7   4.2   0.5  49.3
    (1,1)     0.0    0.1  16.5   4.2   0.5   5.8
(adaptive plans with var_num uniform in [0, 2^23)).  int16 falls short of 5 % at q100 and on
every adaptive plan (they multiply by Q, and range_x1 drives all 64 coefficients to their
range at once, which no pixel block does): there the rounding check rests on range_x1 and
sparse, and on pm511 where it is above 5 %.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import coef_families as CF  # noqa: E402
import inv_bound as IB  # noqa: E402
import inv_model as IM  # noqa: E402

F32_PLANS = [(1, 0), (50, 0), (71, 0)]
F64_PLANS = [(72, 0), (100, 0)]   # 72: the first plan the fp32 bound refuses
ADAPTIVE_PLANS = [(50, 1), (100, 1), (1, 1)]
PLANS = F32_PLANS + F64_PLANS + ADAPTIVE_PLANS
U = 2.0 ** -24
# the two clamp edges of nv = min(1, max(0.1, var / 1000)), var = var_num / 4096, each +- 1, and the ends of int32
VAR_NUMS = [-2 ** 31, -1, 0, 1, 409599, 409600, 409601, 4095999, 4096000, 4096001, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import dct_amd
    dct_amd.lib()
    return torch


@pytest.fixture(scope="module")
def dm(T):
    import dct_amd
    return dct_amd


def gpu(T, a):
    return T.from_numpy(np.array(a)).cuda()  # a copy: the cached arrays are read-only


def blocks_of(img):
    """u8 / float image [1, H, W] or [H, W] -> [n, 64] in raster order of blocks."""
    h, w = img.shape[-2:]
    return img.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


@functools.lru_cache(maxsize=None)
def GL():
    G, L = IB.bound()
    IB.check_linear(L)
    return G, L


@functools.lru_cache(maxsize=None)
def plain_var_num(n):
    """var_num of the adaptive cases that are not about var_num: var in [0, 2048), both sides of both clamp edges."""
    vn = np.random.default_rng(99).integers(0, 1 << 23, n).astype(np.int32)
    vn.setflags(write=False)
    return vn


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(name, q, ad, foreign_var=False):
    """(coef [n, 64], var_num int32 [n], reference recon + 128 [n, 64], fp64-path tolerance [n, 64])."""
    import oracle as O
    coef = CF.family(name, q)
    n = coef.shape[0]
    vn = np.resize(np.array(VAR_NUMS, np.int64), n).astype(np.int32) if foreign_var else plain_var_num(n)
    Q = O.quant_matrix(8, q).ravel()
    if ad:
        var = vn / 4096.0
        want = O.inverse_plane(coef, q, 1, var) + 128.0
        nv = np.minimum(1.0, np.maximum(0.1, var / 1000.0))
        mult = Q[None, :] * (2.0 - nv)[:, None]
        mult[:, 0] = Q[0]
    else:
        want = O.inverse_plane(coef, q, 0) + 128.0
        mult = (1.0 / Q)[None, :]
    sx = IB.block_magnitudes(coef, mult).sum(axis=1, keepdims=True)
    tol64 = U * np.maximum(np.abs(want), 128.0) + 1e-9 * np.maximum(1.0, sx / 1024.0)
    return frozen(coef, vn, want, tol64)


@functools.lru_cache(maxsize=None)
def pixel_bound(name, q, ad, foreign_var=False):
    """e_p [n, 64] of the decoders' fp32 recon: the fp32 inverse's per-block bound, or the fp64 path's."""
    coef, _, _, tol64 = reference(name, q, ad, foreign_var)
    if (q, ad) in F32_PLANS:
        return frozen(IB.block_error(q, coef, *GL()))[0]
    return tol64


@functools.lru_cache(maxsize=None)
def model_pixels(name, q):
    import oracle as O
    scale32 = IM.iscale32(O.dequant_matrix(O.quant_matrix(8, q)))
    return frozen(IM.pixels_of(IM.kernel_inverse(CF.family(name, q), scale32)))[0]


def check_pixels(pix, want, e, what):
    """pix u8 [n, 64] against the reference; returns the share of pixels strictly inside (0, 255)."""
    pix = pix.astype(np.float64)
    over = np.abs(pix - np.clip(want, 0.0, 255.0)) - 0.5
    inside = (want > 0.0) & (want < 255.0)
    print(f"{what}: {100.0 * inside.mean():5.1f} % of pixels in range, max (|pix - clip(reference)| - 0.5) / e_p = "
          f"{(over / e).max():.3f}")
    assert (over <= e).all(), (what, float((over / e).max()))
    assert (pix[want < -e] == 0.0).all(), (what, "not clamped to 0")
    assert (pix[want > 255.0 + e] == 255.0).all(), (what, "not clamped to 255")
    return float(inside.mean())


def decode(T, plan, coef, vn, ad):
    shape = CF.plane_shape(coef.shape[0])
    pix = plan.decode(gpu(T, coef), shape, var_num=gpu(T, vn) if ad else None)
    assert pix.dtype == T.uint8 and tuple(pix.shape) == (1,) + shape
    return pix


# ---- 1. pixels against the fp64 oracle -------------------------------------------------
@pytest.mark.parametrize("q,ad", PLANS)
def test_pixels_against_oracle(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    shares = {}
    for name in CF.NAMES:
        coef, vn, want, _ = reference(name, q, ad)
        pix = blocks_of(decode(T, plan, coef, vn, ad).cpu().numpy())
        shares[name] = check_pixels(pix, want, pixel_bound(name, q, ad), f"q{q} a{ad} {name}")
    # a rounding check needs pixels that land inside the range (the shares in the module docstring)
    assert max(shares[name] for name in CF.RANDOM) >= 0.05, shares


# ---- 2. bit for bit against the model (the operation order the bound is proved for) ------
@pytest.mark.parametrize("q,ad", F32_PLANS)
def test_fp32_pixels_equal_the_model(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    for name in CF.NAMES:
        coef, vn, _, _ = reference(name, q, ad)
        pix = blocks_of(decode(T, plan, coef, vn, ad).cpu().numpy())
        want = model_pixels(name, q)
        assert np.array_equal(pix, want), (q, name, int((pix != want).sum()), np.argwhere(pix != want)[:4].tolist())


# ---- 3. dctq_inverse: one fp32 rounding of the reference value ---------------------------
@pytest.mark.parametrize("q,ad", PLANS)
def test_inverse_is_one_rounding(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    for name in ["int16", "range_x1", "range_x4", "range_x32", "saturated"]:
        coef, vn, want, tol = reference(name, q, ad)
        rec = plan.inverse(gpu(T, coef), var_num=gpu(T, vn) if ad else None).cpu().numpy().astype(np.float64)
        err = np.abs(rec - want)
        print(f"q{q} a{ad} {name}: max |recon| {np.abs(want).max():.4g}, max err {err.max():.3e}, "
              f"max err / tolerance {(err / tol).max():.3f}")
        assert (err <= tol).all(), (q, ad, name, float((err / tol).max()))


# ---- 4. var_num the caller made up ----------------------------------------------------------
@pytest.mark.parametrize("q,ad", ADAPTIVE_PLANS)
def test_foreign_var_num(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    for name in ["pm511", "range_x1"]:
        coef, vn, want, tol = reference(name, q, ad, True)
        assert set(vn[:len(VAR_NUMS)].tolist()) == set(VAR_NUMS)
        pix = blocks_of(decode(T, plan, coef, vn, ad).cpu().numpy())
        check_pixels(pix, want, tol, f"q{q} a{ad} {name}, foreign var_num")
        rec = plan.inverse(gpu(T, coef), var_num=gpu(T, vn)).cpu().numpy().astype(np.float64)
        err = np.abs(rec - want)
        print(f"q{q} a{ad} {name}, foreign var_num: dctq_inverse max err / tolerance {(err / tol).max():.3f}")
        assert (err <= tol).all(), (q, name, float((err / tol).max()))


# ---- 5. symbols -------------------------------------------------------------------------------
def rle_decode_cpu(off, sym):
    """run_length_decode + zigzag_to_block of a 4-byte stream (src/entropy.c:327-351, 183-210): pos += run;
    the value lands while pos < 64; pos++."""
    n = off.size - 1
    off = off.astype(np.int64)
    value = (sym & 0xFFFF).astype(np.uint16).view(np.int16)
    block = np.repeat(np.arange(n), np.diff(off))
    step = np.cumsum((sym >> 16).astype(np.int64) + 1)
    before = np.concatenate([[0], step])[off[:-1]]  # steps taken before the block's first symbol
    pos = step - before[block] - 1
    out = np.zeros((n, 64), np.int16)
    keep = pos < 64
    out[block[keep], CF.zigzag_order()[pos[keep]]] = value[keep]
    return out


@functools.lru_cache(maxsize=None)
def streams(name, q):
    """The family's symbols from the reference's run-length coder: (offsets, 4-byte symbols, 2-byte symbols or None)."""
    import oracle as O
    coef = CF.family(name, q)
    off, sym = O.rle_encode_plane(coef)
    assert off[-1] == sym.size and (np.diff(off.astype(np.int64)) >= 1).all()
    # the run-length round trip is lossless for every family (no family is left out)
    assert np.array_equal(rle_decode_cpu(off, sym), coef), name
    sym16 = O.pack16(sym) if np.abs(coef.astype(np.int32)).max() <= 511 else None
    if sym16 is not None:
        assert np.array_equal(O.unpack16(sym16), sym)
    return off, sym, sym16


@pytest.mark.parametrize("q,ad", PLANS)
def test_symbols_equal_two_step_and_coefficients(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    narrow = []
    for name in CF.NAMES:
        coef, vn, _, _ = reference(name, q, ad)
        off, sym, sym16 = streams(name, q)
        shape = CF.plane_shape(coef.shape[0])
        vns = [gpu(T, vn)] if ad else None
        direct = plan.decode_planes([gpu(T, coef)], shapes=[shape], var_nums=vns)[0]
        goff = gpu(T, off.view(np.int32))
        for s in [sym.view(np.int32)] + ([sym16.view(np.int16)] if sym16 is not None else []):
            gs = gpu(T, s)
            got = plan.decode_symbols(gs, goff, shapes=[shape], var_nums=vns)[0]
            back = dm.rle_decode(gs, goff)
            assert T.equal(back.cpu(), T.from_numpy(np.array(coef))), (q, ad, name, s.dtype)
            two = plan.decode_planes([back], shapes=[shape], var_nums=vns)[0]
            assert T.equal(got, two), (q, ad, name, s.dtype, int((got != two).sum()))
            assert T.equal(got, direct), (q, ad, name, s.dtype, int((got != direct).sum()))
        if sym16 is not None:
            narrow.append(name)
    # a 2-byte stream was decoded under every plan, the 4-byte plans (q100) included
    assert "pm511" in narrow and plan.symbol_bytes == (4 if q == 100 else 2), (narrow, plan.symbol_bytes)


@pytest.mark.parametrize("q,ad", [(50, 0), (100, 0), (50, 1)])
def test_two_byte_payload_0x200(T, dm, q, ad):
    """0x200 is the 10-bit pattern outside the documented [-511, 511]: rle_decode_core.h sym_value<2>
    sign-extends the low 10 bits, so it is -512."""
    zz = CF.zigzag_order()
    blocks = [  # (payload, run) per symbol
        [(0x200, 0)],
        [(0x200, 63)],
        [(0x1FF, 0), (0x200, 5), (0x201, 0), (0x200, 55)],   # 511, -512, -511, -512
        [(0x200, 0)] * 64,
        [(0x200, 10), (0x200, 60)],                          # the second lands past the block: dropped
    ]
    want = np.zeros((64, 64), np.int16)
    want[0, zz[0]] = -512
    want[1, zz[63]] = -512
    want[2, zz[[0, 6, 7, 63]]] = [511, -512, -511, -512]
    want[3, :] = -512
    want[4, zz[10]] = -512
    units, counts = [], []
    for b in range(64):
        syms = blocks[b] if b < len(blocks) else None
        units += [(r << 10) | p for p, r in syms] if syms else [0x0000]  # 0x0000: the all-zero block (0, 64)
        counts.append(len(syms) if syms else 1)
    off = np.cumsum([0] + counts).astype(np.uint32)
    assert off[-1] == len(units)
    gs, go = gpu(T, np.array(units, np.uint16).view(np.int16)), gpu(T, off.view(np.int32))
    coef = dm.rle_decode(gs, go)
    assert np.array_equal(coef.cpu().numpy(), want)
    plan = dm.Plan(q, ad)
    vns = [gpu(T, plain_var_num(64))] if ad else None
    got = plan.decode_symbols(gs, go, shapes=[(64, 64)], var_nums=vns)[0]
    assert T.equal(got, plan.decode_planes([coef], shapes=[(64, 64)], var_nums=vns)[0])
