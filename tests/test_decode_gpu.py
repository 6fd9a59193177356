"""GPU: the pixel decoder (dctq_decode_planes / Plan.decode_planes): coefficients ->
clamped u8 pixels at their image position.

Bounds.  A pixel is rne(clamp(r, 0, 255)) of the fp32 recon r, and |r - reference| <=
1e-4 (BASELINE.json north_star; the round trip's and dctq_inverse's bound), clamping
does not increase a distance, and rounding to nearest moves a value by at most 0.5:
|pix - clip(reference, 0, 255)| <= 0.5 + 1e-4.  Against the round trip's own recon the
decoder must agree bit for bit (same arithmetic, operation for operation)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fp32-admitted (50,0), not admitted non-adaptive (75,0) (100,0), adaptive
PLANS = [(50, 0), (50, 1), (10, 1), (90, 1), (100, 0), (100, 1), (1, 1), (75, 0)]
KIND_NAMES = ["uniform", "smooth", "const", "extreme"]
W, H, SEED = 64, 48, 21
TOL = 0.5 + 1e-4
SENTINEL = 0xA5


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


def untile(blocks, f, h, w):
    """[f*h/8*w/8, 64] block-major (raster order of blocks) -> [f, h, w]; numpy or torch."""
    b = blocks.reshape(f, h // 8, w // 8, 8, 8)  # frame, block row, block column, row, column
    b = b.permute(0, 1, 3, 2, 4) if hasattr(b, "permute") else b.transpose(0, 1, 3, 2, 4)
    return b.reshape(f, h, w)


@functools.lru_cache(maxsize=None)
def oracle_case(kind, q, ad, w=W, h=H, seed=SEED):
    """(pixels [h, w], coefficients, var_num int32, reference recon + 128 as an image [h, w]) from the oracle."""
    import oracle as O
    px = O.synth_plane(seed, O.KINDS[kind], w, h)
    coef = O.forward_plane(px, q, ad)
    var = O.plane_variance(px)
    vn = var * 4096.0
    assert np.array_equal(vn, np.round(vn))
    want = O.inverse_plane(coef, q, ad, var if ad else None) + 128.0
    out = (px, coef, vn.astype(np.int32), untile(want, 1, h, w)[0])
    for a in out:
        a.setflags(write=False)
    return out


def check_against_oracle(pix, want, what):
    err = np.abs(pix.astype(np.float64) - np.clip(want, 0.0, 255.0)).max()
    print(f"{what}: max |pix - clip(reference)| = {err:.6f}")
    assert err <= TOL, (what, err)


def gpu(T, a):
    return T.from_numpy(np.array(a)).cuda()  # a copy: the cached oracle arrays are read-only


def rounded_recon(T, rec, f, h, w):
    """The round trip's fp32 recon [nblk, 64] -> the u8 image the decoder must produce."""
    return untile(T.round(rec.clamp(0, 255)).to(T.uint8), f, h, w).contiguous()


# ---- 1. oracle parity ---------------------------------------------------------
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("q,ad", PLANS)
def test_decode_matches_oracle(T, dm, q, ad, kind):
    px, coef, vn, want = oracle_case(kind, q, ad)
    if kind == "extreme" and (q, ad) in ((100, 0), (1, 1)):
        # the clamp is exercised at both ends (oracle, on the CPU: 787 / 767 and 819 / 726 pixels)
        below, above = int((want < 0).sum()), int((want > 255).sum())
        print(f"q{q} a{ad}: {below} pixels below 0, {above} above 255")
        assert below > 0 and above > 0
    plan = dm.Plan(q, ad)
    pix = plan.decode(gpu(T, coef), (H, W), var_num=gpu(T, vn) if ad else None)
    assert pix.dtype == T.uint8 and tuple(pix.shape) == (1, H, W)
    check_against_oracle(pix.cpu().numpy()[0], want, f"{kind} q{q} a{ad}")


# ---- 2. exact agreement with the round trip -------------------------------------
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("q,ad", PLANS)
def test_decode_equals_rounded_round_trip(T, dm, q, ad, kind):
    px, _, _, want = oracle_case(kind, q, ad)
    if kind == "const" and (q, ad) == (1, 1):
        # exact x.5 reconstructions: the tie rule (to even) decides these pixels
        ties = np.abs(want - np.floor(want) - 0.5) < 1e-9
        assert (ties & (want > 0) & (want < 255)).any()
    plan = dm.Plan(q, ad)
    gp = gpu(T, px)
    vn = T.zeros(px.size // 64, dtype=T.int32, device="cuda")
    coefs, recs = plan.round_trip_planes([gp], var_nums=[vn])
    pix = plan.decode_planes(coefs, shapes=[(H, W)], var_nums=[vn] if ad else None)[0]
    expect = rounded_recon(T, recs[0], 1, H, W)
    ntie = int(((recs[0] * 2) % 2 == 1).sum())
    print(f"{kind} q{q} a{ad}: {ntie} exact .5 values in the recon")
    assert T.equal(pix, expect), (kind, q, ad, int((pix != expect).sum()))


# ---- 3. geometry ------------------------------------------------------------------
GEOMETRY = [  # width, height, frames, row padding, extra rows between frames
    (8, 8, 1, 0, 0),          # one block
    (40, 24, 1, 0, 0),        # 15 blocks
    (264, 8, 1, 8, 0),        # 33 blocks: crosses a 32-block batch
    (136, 56, 3, 16, 5),      # 119 blocks per frame: batches straddle frames; frame_stride beyond one frame
    (520, 72, 1, 0, 0),       # 585 blocks
    (1920, 16, 2, 0, 0),      # 480 blocks
]


@pytest.mark.parametrize("q,ad", [(50, 0), (75, 0), (90, 1)])
@pytest.mark.parametrize("w,h,f,pad,gap", GEOMETRY)
def test_decode_geometry_and_untouched_bytes(T, dm, w, h, f, pad, gap, q, ad):
    plan = dm.Plan(q, ad)
    px = dm.synth(4000 + w, "uniform", w, h, f)
    vn = T.zeros(f * (w // 8) * (h // 8), dtype=T.int32, device="cuda")
    coefs, recs = plan.round_trip_planes([px], var_nums=[vn])
    expect = rounded_recon(T, recs[0], f, h, w)
    buf = T.full((f, h + gap, w + pad), SENTINEL, dtype=T.uint8, device="cuda")
    view = buf[:, :h, :w]
    out = plan.decode_planes(coefs, outs=[view], var_nums=[vn] if ad else None)[0]
    assert out.data_ptr() == buf.data_ptr()
    assert T.equal(view, expect), (w, h, f, int((view != expect).sum()))
    outside = buf.clone()
    outside[:, :h, :w] = SENTINEL
    assert bool((outside == SENTINEL).all()), "bytes outside width x height were written"
    # the same into a contiguous tensor the call allocates
    assert T.equal(plan.decode(coefs[0], (f, h, w), var_num=vn if ad else None), expect)


# ---- 4. multi-plane -----------------------------------------------------------------
@pytest.mark.parametrize("q,ad", [(90, 1), (50, 0), (100, 0)])
def test_decode_four_planes_one_launch(T, dm, q, ad):
    import oracle as O
    plan = dm.Plan(q, ad)
    shapes = [(1, 48, 64), (1, 24, 32), (1, 24, 32), (3, 16, 40)]  # 4:2:0 Y, Cb, Cr + a 3-frame stack
    planes = [dm.synth(900 + k, KIND_NAMES[k], s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    vns = [T.zeros(s[0] * (s[1] // 8) * (s[2] // 8), dtype=T.int32, device="cuda") for s in shapes]
    coefs = plan.forward_quant_planes(planes, var_nums=vns)
    got = plan.decode_planes(coefs, shapes=shapes, var_nums=vns if ad else None)
    for k, s in enumerate(shapes):
        single = plan.decode(coefs[k], s, var_num=vns[k] if ad else None)
        assert T.equal(got[k], single), (k, s)
        host_px, host_c, host_pix = planes[k].cpu().numpy(), coefs[k].cpu().numpy(), got[k].cpu().numpy()
        per = (s[1] // 8) * (s[2] // 8)
        for fr in range(s[0]):
            want = O.inverse_plane(host_c[fr * per:(fr + 1) * per], q, ad,
                                   O.plane_variance(host_px[fr]) if ad else None) + 128.0
            check_against_oracle(host_pix[fr], untile(want, 1, s[1], s[2])[0], f"plane {k} frame {fr} q{q} a{ad}")


# ---- 5. end to end: pixels -> symbols -> pixels ------------------------------------------
@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("q,ad", [(50, 0), (90, 1), (100, 0)])
def test_symbols_to_pixels(T, dm, q, ad, side_stream):
    px, _, _, want = oracle_case("uniform", q, ad)
    plan = dm.Plan(q, ad)
    widths = [4, 2] if plan.symbol_bytes == 2 else [4]
    assert (q, ad, widths) in [(50, 0, [4, 2]), (90, 1, [4, 2]), (100, 0, [4])]
    stream = T.cuda.Stream() if side_stream else T.cuda.current_stream()
    gp = gpu(T, px)
    T.cuda.synchronize()
    with T.cuda.stream(stream):
        vn = T.zeros(px.size // 64, dtype=T.int32, device="cuda")
        direct = plan.decode(plan.forward_quant(gp, var_num=vn), (H, W), var_num=vn if ad else None)
        results = []
        for sb in widths:
            _, off, sym = plan.encode_planes([gp], symbol_bytes=sb)
            coef = dm.rle_decode(sym, off)
            results.append(plan.decode_planes([coef], shapes=[(H, W)], var_nums=[vn] if ad else None)[0])
    stream.synchronize()
    for sb, pix in zip(widths, results):
        assert T.equal(pix, direct), (q, ad, sb)
        check_against_oracle(pix.cpu().numpy()[0], want, f"q{q} a{ad} {sb}-byte symbols")
    if side_stream:
        dm.stream_release(stream)


# ---- 6. invalid arguments -----------------------------------------------------------------
def test_decode_invalid_arguments(T, dm):
    L = dm.lib()
    EINVAL = -1
    plans = {0: dm.Plan(50, 0), 1: dm.Plan(50, 1)}
    w, h = 32, 16
    nblk = (w // 8) * (h // 8)
    buf = T.full((h * w + 64,), SENTINEL, dtype=T.uint8, device="cuda")
    coef = T.zeros(nblk * 64 + 64, dtype=T.int16, device="cuda")
    vn = T.zeros(nblk, dtype=T.int32, device="cuda")
    assert buf.data_ptr() % 8 == 0 and coef.data_ptr() % 16 == 0

    def call(ad=0, plan="ok", coefs="ok", vns="ok", dst="ok", nplanes=1, **geo):
        g = dict(pixels=buf.data_ptr(), stride=w, frame_stride=w * h, width=w, height=h, nframes=1, coef=coef.data_ptr(),
                 vn=vn.data_ptr())
        g.update(geo)
        n = max(nplanes, 1)
        descs = (dm._Plane * n)(*[dm._Plane(g["pixels"], g["stride"], g["frame_stride"], g["width"], g["height"],
                                            g["nframes"]) for _ in range(n)])
        cp = (C.c_void_p * n)(*[g["coef"]] * n)
        vp = (C.c_void_p * n)(*[g["vn"]] * n)
        return L.dctq_decode_planes(plans[ad]._h if plan == "ok" else None,
                                    C.cast(cp, C.c_void_p) if coefs == "ok" else None,
                                    C.cast(vp, C.c_void_p) if vns == "ok" else None,
                                    descs if dst == "ok" else None, nplanes, None)

    bad = {
        "NULL plan": dict(plan=None),
        "NULL coef": dict(coefs=None),
        "NULL dst": dict(dst=None),
        "NULL coef[k]": dict(coef=None),
        "NULL dst[k].pixels": dict(pixels=None),
        "nplanes 0": dict(nplanes=0),
        "nplanes 5": dict(nplanes=5),
        "nplanes -1": dict(nplanes=-1),
        "width 12": dict(width=12),
        "width 0": dict(width=0),
        "width -8": dict(width=-8),
        "height 0": dict(height=0),
        "height 12": dict(height=12),
        "nframes 0": dict(nframes=0),
        "stride < width": dict(stride=w - 8),
        "stride % 8": dict(width=16, stride=20),
        "pixels misaligned": dict(pixels=buf.data_ptr() + 4),
        "coef misaligned": dict(coef=coef.data_ptr() + 8),
        "adaptive without var_num": dict(ad=1, vns=None),
        "adaptive with a NULL var_num[k]": dict(ad=1, vn=None),
        "2^31 blocks": dict(width=8 * 65536, stride=8 * 65536, height=8 * 32768),
        "2^31 blocks in frames": dict(nframes=2 ** 31 // nblk),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        assert L.dctq_error_string(EINVAL), what
    # non-adaptive plans ignore var_num: NULL, or entries that are NULL
    assert call(vns=None) == 0 and call(vn=None) == 0
    T.cuda.synchronize()
    assert bool((buf[w * h:] == SENTINEL).all())
    buf.fill_(SENTINEL)
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
    T.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call wrote pixels"
    # the Python layer refuses short or mistyped tensors before the library sees them
    with pytest.raises(dm.DctqError):
        plans[0].decode(coef[:nblk * 64 - 64], (h, w))
    with pytest.raises(dm.DctqError):
        plans[0].decode(coef.to(T.int32), (h, w))
    with pytest.raises(dm.DctqError):
        plans[1].decode(coef, (h, w))  # adaptive, no var_num
    with pytest.raises(dm.DctqError):
        plans[0].decode_planes([coef])  # neither shapes nor outs


# ---- 7. C host --------------------------------------------------------------------------------
def test_frame_decode_host(T, dm):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for (w, h, q, ad, kind) in [(640, 480, 90, 1, 1), (64, 48, 50, 0, 0)]:
        r = subprocess.run([os.path.join(ROOT, "host", "frame_decode"), str(w), str(h), str(q), str(ad), "12345",
                            str(kind)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = dict(l.split(":", 1) for l in r.stdout.strip().splitlines())
        assert int(got["abi_version"]) == 6 and got["padding_intact"] == "1", got
        plan = dm.Plan(q, ad)
        px = dm.synth(12345, kind, w, h)
        vn = T.zeros((w // 8) * (h // 8), dtype=T.int32, device="cuda")
        pix = plan.decode(plan.forward_quant(px, var_num=vn), (h, w), var_num=vn if ad else None)
        fnv = 1469598103934665603
        for b in pix.cpu().numpy().tobytes():
            fnv = ((fnv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert int(got["pixels_fnv1a"], 16) == fnv, (w, h, q, ad)
        d = pix.cpu().numpy()[0].astype(np.float64) - px.cpu().numpy()[0]
        psnr = 10.0 * np.log10(255.0 * 255.0 / (d * d).mean())
        assert abs(float(got["psnr_u8"]) - psnr) < 1e-3, (got, psnr)
