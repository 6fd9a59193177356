"""GPU: per-block distortion from pixels in one launch (dctq_distortion_planes /
Plan.distortion_planes).

Contract.  sse[b] is the squared error of block b of the u8 picture that
decode_planes(forward_quant_planes(planes)) writes, against the source: equal, not close.

Bounds against the oracle.  A decoded pixel is rne(clamp(r, 0, 255)) of the fp32 recon r with
|r - reference| <= 1e-4 (the round trip's and the decoder's bound, tests/test_decode_gpu.py);
clamping does not increase a distance and rounding to nearest moves a value by at most 0.5, so
|dec - c| <= T = 0.5 + 1e-4 for c = clip(reference, 0, 255).  With e = src - c the error of a
pixel, |src - dec|, lies in [max(|e| - T, 0), |e| + T], hence for every block
    floor(sum max(|e| - T, 0)^2) <= sse <= ceil(sum (|e| + T)^2)
(sse is an integer, so the bounds may be rounded outwards to integers)."""
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the plan list of tests/test_decode_gpu.py: fp32-admitted (50,0), not admitted non-adaptive
# (75,0) (100,0), adaptive -- all three kernels, both clamp ends
PLANS = [(50, 0), (75, 0), (100, 0), (50, 1), (10, 1), (90, 1), (100, 1), (1, 1)]
KIND_NAMES = ["uniform", "smooth", "const", "extreme"]
W, H, SEED = 64, 48, 21
TOL = 0.5 + 1e-4
SENTINEL = 0x5A5A5A5A


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


def block_sums(a, f, h, w):
    """[f, h, w] per-pixel values -> [f * h/8 * w/8] per-block sums (frame, block row, block
    column); numpy or torch."""
    return a.reshape(f, h // 8, 8, w // 8, 8).sum((2, 4)).reshape(-1)


def untile(blocks, f, h, w):
    """[f*h/8*w/8, 64] block-major -> [f, h, w] (numpy)."""
    return blocks.reshape(f, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(f, h, w)


@functools.lru_cache(maxsize=None)
def oracle_case(kind, q, ad):
    """(pixels [H, W] u8, reference recon + 128 as an image [H, W] float64) from the oracle."""
    import oracle as O
    px = O.synth_plane(SEED, O.KINDS[kind], W, H)
    var = O.plane_variance(px)
    want = O.inverse_plane(O.forward_plane(px, q, ad), q, ad, var if ad else None) + 128.0
    out = (px, untile(want, 1, H, W)[0])
    for a in out:
        a.setflags(write=False)
    return out


def composition(T, plan, px, ad):
    """The parent's route: forward_quant_planes + decode_planes + a reduction by torch, in int64.
    px: [F, H, W] u8 (contiguous or a view)."""
    f, h, w = px.shape
    vn = T.zeros(f * (h // 8) * (w // 8), dtype=T.int32, device="cuda")
    coefs = plan.forward_quant_planes([px.contiguous()], var_nums=[vn])
    pix = plan.decode_planes(coefs, shapes=[(f, h, w)], var_nums=[vn] if ad else None)[0]
    return block_sums((px.long() - pix.long()).square(), f, h, w)


@functools.lru_cache(maxsize=None)
def device_case(kind, q, ad):
    """(sse int64 [N] of distortion_planes, the composition's int64 [N]) for oracle_case's pixels,
    both on the host; computed once per case and shared by the tests below."""
    import torch
    import dct_amd
    px, _ = oracle_case(kind, q, ad)
    gp = torch.from_numpy(np.array(px)).cuda()
    plan = dct_amd.Plan(q, ad)
    got = plan.distortion_planes([gp])
    assert got.dtype == torch.int32 and tuple(got.shape) == ((W // 8) * (H // 8),)
    return got.long().cpu(), composition(torch, plan, gp.unsqueeze(0), ad).cpu()


# ---- 1. exact equivalence with the composition -------------------------------------------------
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("q,ad", PLANS)
def test_distortion_equals_composition(T, dm, q, ad, kind):
    _, want = oracle_case(kind, q, ad)
    if kind == "const" and (q, ad) == (1, 1):
        # exact x.5 reconstructions: the tie rule (to even) decides these pixels
        ties = np.abs(want - np.floor(want) - 0.5) < 1e-9
        assert (ties & (want > 0) & (want < 255)).any()
    if kind == "extreme" and (q, ad) == (100, 0):
        below, above = int((want < 0).sum()), int((want > 255).sum())
        print(f"q{q} a{ad}: {below} pixels below 0, {above} above 255")
        assert below > 0 and above > 0
    got, expect = device_case(kind, q, ad)
    print(f"{kind} q{q} a{ad}: sse total {int(got.sum())}, max {int(got.max())}, "
          f"{int((got != expect).sum())} blocks differ")
    assert T.equal(got, expect), (kind, q, ad)


# ---- 2. sandwich against the oracle ------------------------------------------------------------
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("q,ad", PLANS)
def test_distortion_within_oracle_sandwich(T, dm, q, ad, kind):
    px, want = oracle_case(kind, q, ad)
    e = np.abs(px.astype(np.float64) - np.clip(want, 0.0, 255.0))
    lo = np.floor(block_sums(np.maximum(e - TOL, 0.0)[None] ** 2, 1, H, W))
    hi = np.ceil(block_sums((e + TOL)[None] ** 2, 1, H, W))
    sse = device_case(kind, q, ad)[0].numpy().astype(np.float64)
    print(f"{kind} q{q} a{ad}: min (sse - lo) = {(sse - lo).min():.3f}, min (hi - sse) = {(hi - sse).min():.3f}")
    assert (lo <= sse).all() and (sse <= hi).all(), (kind, q, ad)


# ---- 3. geometry ---------------------------------------------------------------------------------
GEOMETRY = [  # width, height, frames, row padding, extra rows between frames
    (8, 8, 1, 0, 0),          # one block
    (264, 8, 1, 8, 0),        # 33 blocks: both inverses of a batch, the second nearly empty
    (520, 8, 1, 0, 0),        # 65 blocks: crosses the 64-block batch
    (136, 56, 3, 16, 5),      # 119 blocks per frame: batches straddle frames; strided views
    (1920, 16, 2, 0, 0),      # 480 blocks per frame over two frames: long rows, several batches per wave
]


def strided_source(T, dm, w, h, f, pad, gap):
    """A [f, h, w] view of synthetic pixels inside a buffer with padded rows and gap rows between
    frames (frame_stride beyond one frame)."""
    buf = T.full((f, h + gap, w + pad), 0xA5, dtype=T.uint8, device="cuda")
    view = buf[:, :h, :w]
    view.copy_(dm.synth(4000 + w, "uniform", w, h, f))
    return view


def run_with_sentinel(T, plan, planes, stream=None):
    n = sum(p.numel() // 64 for p in planes)
    out = T.full((n + 16,), SENTINEL, dtype=T.int32, device="cuda")
    got = plan.distortion_planes(planes, out=out, stream=stream)
    assert got.data_ptr() == out.data_ptr()
    return out, n


@pytest.mark.parametrize("q,ad", [(50, 0), (75, 0), (90, 1)])
@pytest.mark.parametrize("w,h,f,pad,gap", GEOMETRY)
def test_distortion_geometry(T, dm, w, h, f, pad, gap, q, ad):
    plan = dm.Plan(q, ad)
    view = strided_source(T, dm, w, h, f, pad, gap)
    if pad or gap:
        assert not view.is_contiguous()
    expect = composition(T, plan, view, ad)
    out, n = run_with_sentinel(T, plan, [view])
    assert n == f * (w // 8) * (h // 8)
    assert T.equal(out[:n].long(), expect), (w, h, f, int((out[:n].long() != expect).sum()))
    assert bool((out[n:] == SENTINEL).all()), "words past the last block were written"


# ---- 4. four planes of independent geometry in one launch -----------------------------------------
@pytest.mark.parametrize("q,ad", [(50, 0), (50, 1)])
def test_distortion_four_planes_one_launch(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    shapes = [(32, 16), (16, 8), (16, 8), (72, 8)]  # Y, Cb, Cr of a 4:2:0 frame + a fourth plane
    planes = [dm.synth(900 + k, KIND_NAMES[k], w, h) for k, (w, h) in enumerate(shapes)]
    out, n = run_with_sentinel(T, plan, planes)
    assert n == 8 + 2 + 2 + 9
    single = T.cat([plan.distortion_planes([p]) for p in planes])
    assert T.equal(out[:n], single)
    assert bool((out[n:] == SENTINEL).all())
    expect = T.cat([composition(T, plan, p, ad) for p in planes])
    assert T.equal(out[:n].long(), expect)


# ---- 5. rate and distortion together -----------------------------------------------------------------
@pytest.mark.parametrize("q,ad", [(50, 0), (90, 1)])
def test_rate_distortion_planes(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    planes = [dm.synth(77, "uniform", 64, 48, 2), dm.synth(78, "smooth", 32, 24, 2)]
    bits, sse = plan.rate_distortion_planes(planes)
    assert T.equal(bits, plan.huffman_bits_planes(planes))
    assert T.equal(sse, plan.distortion_planes(planes))
    assert bits.shape == sse.shape and bits.dtype == sse.dtype == T.int32
    psnr = dm.psnr_u8(sse.sum().item(), 64 * sse.numel())
    assert 0.0 < psnr < 100.0


# ---- 6. a non-default stream ------------------------------------------------------------------------
@pytest.mark.parametrize("q,ad", [(50, 0), (90, 1)])
def test_distortion_on_side_stream(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    view = strided_source(T, dm, 520, 8, 1, 0, 0)
    expect = composition(T, plan, view, ad)
    T.cuda.synchronize()
    stream = T.cuda.Stream()
    with T.cuda.stream(stream):
        out, n = run_with_sentinel(T, plan, [view], stream=stream)
    stream.synchronize()
    assert n == 65
    assert T.equal(out[:n].long(), expect)
    assert bool((out[n:] == SENTINEL).all())
    dm.stream_release(stream)


# ---- 7. argument errors -------------------------------------------------------------------------------
def test_distortion_invalid_arguments(T, dm):
    import ctypes as C
    plan = dm.Plan(50, 0)
    px = dm.synth(5, "uniform", 32, 16)
    n = 8
    with pytest.raises(dm.DctqError):
        plan.distortion_planes([])
    with pytest.raises(dm.DctqError):
        plan.distortion_planes([px] * 5)
    with pytest.raises(dm.DctqError):
        plan.distortion_planes([px], out=T.zeros(n, dtype=T.int64, device="cuda"))
    with pytest.raises(dm.DctqError):
        plan.distortion_planes([px], out=T.zeros(n - 1, dtype=T.int32, device="cuda"))
    # the library itself refuses the same, and writes nothing
    L, EINVAL = dm.lib(), -1
    out = T.full((n + 16,), SENTINEL, dtype=T.int32, device="cuda")
    descs = (dm._Plane * 5)(*[dm.plane_desc(px)] * 5)
    bad12 = dm.plane_desc(px)
    bad12.width = 12
    for what, args in {
        "nplanes 0": (plan._h, descs, 0, out.data_ptr()),
        "nplanes 5": (plan._h, descs, 5, out.data_ptr()),
        "nplanes -1": (plan._h, descs, -1, out.data_ptr()),
        "NULL plan": (None, descs, 1, out.data_ptr()),
        "NULL planes": (plan._h, None, 1, out.data_ptr()),
        "NULL sse": (plan._h, descs, 1, None),
        "misaligned sse": (plan._h, descs, 1, out.data_ptr() + 2),
        "width 12": (plan._h, C.pointer(bad12), 1, out.data_ptr()),
    }.items():
        assert L.dctq_distortion_planes(args[0], args[1], args[2], C.c_void_p(args[3]), None) == EINVAL, what
        assert L.dctq_error_string(EINVAL), what
    T.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote"
    assert L.dctq_distortion_planes(plan._h, descs, 1, C.c_void_p(out.data_ptr()), None) == 0
    T.cuda.synchronize()
    assert T.equal(out[:n], plan.distortion_planes([px])) and bool((out[n:] == SENTINEL).all())


# ---- 8. C host --------------------------------------------------------------------------------------------
def test_frame_rd_host(T, dm):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_rd"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for (w, h, f, q, ad, kind) in [(64, 48, 2, 90, 1, 1), (80, 32, 1, 50, 0, 0)]:
        r = subprocess.run([os.path.join(ROOT, "host", "frame_rd"), str(w), str(h), str(f), str(q), str(ad), "12345",
                            str(kind)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = dict(l.split(":", 1) for l in r.stdout.strip().splitlines())
        assert got["distortion_equal"] == "1" and int(got["abi_version"]) == 6, got
        plan = dm.Plan(q, ad)
        planes = [dm.synth(12345 + 1000 * k, kind, w >> (k > 0), h >> (k > 0), f) for k in range(3)]
        bits, sse = plan.rate_distortion_planes(planes)
        assert int(got["blocks"]) == sse.numel() == f * (w // 8) * (h // 8) * 3 // 2
        assert int(got["sse_total"]) == int(sse.sum().item()), (w, h, q, ad)
        assert int(got["bits_total"]) == int(bits.sum().item()), (w, h, q, ad)
        assert abs(float(got["psnr_u8"]) - dm.psnr_u8(sse.sum().item(), 64 * sse.numel())) < 1e-3
