"""GPU: the colour front and back end (dctq_rgb_to_ycbcr_planes / dctq_ycbcr_to_rgb_planes;
dct_amd.rgb_desc / rgb_to_ycbcr / ycbcr_to_rgb).

The yardstick is tools/color_ref.py, plain numpy written from the definition: every case is
compared to it byte for byte, never to the kernels themselves or to floating point."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import color_ref  # noqa: E402

SENTINEL = 0xA5
EINVAL = -1
# (F, H, W): one chroma block; frames; a width that is no multiple of a wave's 64 lanes x 8 pixels,
# so row tails and frame boundaries fall inside a wave; more than one wave per row
SHAPES = [(1, 16, 16), (2, 32, 48), (3, 48, 80), (1, 16, 1040)]
# layout -> (interleaved pixel step or 0 for planar, memory holds B first)
LAYOUTS = {"rgb": (3, False), "rgbx": (4, False), "bgr": (3, True), "bgrx": (4, True),
           "planar": (0, False), "planar_reversed": (0, True)}


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
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(shape, sub):
    """Random RGB [F, H, W, 3] with its reference planes, and random planes (any bytes, so the
    inverse clamps on both sides) with their reference picture."""
    f, h, w = shape
    rng = np.random.default_rng(1000 * w + 10 * h + f + (sub == "420"))
    rgb = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    s = 2 if sub == "420" else 1
    planes = (rng.integers(0, 256, (f, h, w), dtype=np.uint8),
              rng.integers(0, 256, (f, h // s, w // s), dtype=np.uint8),
              rng.integers(0, 256, (f, h // s, w // s), dtype=np.uint8))
    return rgb, color_ref.forward(rgb, sub), planes, color_ref.inverse(*planes)


def rgb_buffer(T, layout, shape, pad=0, gap=0, fill=0):
    """(buf, view, bgr): a flat u8 device buffer filled with `fill` and the [F, H, W, C] view into
    it that rgb_desc(view, bgr) describes as `layout`; rows padded by `pad` bytes, frames (and
    channel planes) separated by `gap` more."""
    step, bgr = LAYOUTS[layout]
    f, h, w = shape
    if step:
        row = w * step + pad
        frame = row * h + gap
        buf = T.full((f * frame,), fill, dtype=T.uint8, device="cuda")
        return buf, buf.as_strided((f, h, w, step), (frame, row, step, 1)), bgr
    row = w + pad
    plane = row * h + gap
    buf = T.full((f * 3 * plane,), fill, dtype=T.uint8, device="cuda")
    return buf, buf.as_strided((f, h, w, 3), (3 * plane, row, 1, plane)), bgr


def in_memory(T, layout, rgb, x=None):
    """The logical picture rgb [F, H, W, 3] as the channels of the layout's view hold it: B first
    for the B-first layouts, and a fourth channel x for 4-byte pixels."""
    step, bgr = LAYOUTS[layout]
    mem = rgb[..., ::-1] if bgr else rgb
    if step == 4:
        mem = np.concatenate([mem, x if x is not None else np.full(rgb.shape[:3] + (1,), 255, np.uint8)], axis=-1)
    return gpu(T, mem)


def plane_buffers(T, shapes, pad=0, gap=0):
    """[(buf, view)] per plane: [F, H, W] views into sentinel-filled buffers, rows padded by `pad`
    bytes and frames separated by `gap` rows."""
    out = []
    for f, h, w in shapes:
        buf = T.full((f, h + gap, w + pad), SENTINEL, dtype=T.uint8, device="cuda")
        out.append((buf, buf[:, :h, :w]))
    return out


def untouched_outside(T, buf, view):
    """Every byte of buf outside view is still the sentinel."""
    b = buf.clone()
    b.as_strided(view.size(), view.stride(), view.storage_offset()).fill_(SENTINEL)
    return bool((b == SENTINEL).all())


def plane_shapes(shape, sub):
    f, h, w = shape
    s = 2 if sub == "420" else 1
    return [(f, h, w), (f, h // s, w // s), (f, h // s, w // s)]


# ---- 1. every colour once ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every():
    rgb = color_ref.all_colours()[None]  # [1, 4096, 4096, 3]
    return rgb, color_ref.forward(rgb, "444")


def test_every_colour_forward_and_back(T, dm, every):
    rgb, want = every
    got = dm.rgb_to_ycbcr(gpu(T, rgb), "444")
    for name, g, w in zip(("y", "cb", "cr"), got, want):
        assert np.array_equal(g.cpu().numpy(), w), name
    back = dm.ycbcr_to_rgb(*got).cpu().numpy()
    assert np.array_equal(back, color_ref.inverse(*want))
    assert int(np.abs(back.astype(np.int16) - rgb.astype(np.int16)).max()) == 1


def test_every_byte_triple_inverse(T, dm, every):
    rgb, _ = every
    planes = [np.ascontiguousarray(rgb[..., c]) for c in range(3)]  # every (Y, Cb, Cr) once
    got = dm.ycbcr_to_rgb(*[gpu(T, p) for p in planes]).cpu().numpy()
    assert np.array_equal(got, color_ref.inverse(*planes))


# ---- 2. layouts x subsampling ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(T, dm, layout, sub, shape):
    rgb, want_planes, planes, want_rgb = case(shape, sub)
    step, bgr = LAYOUTS[layout]
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, rgb.shape[:3] + (1,), dtype=np.uint8)  # the fourth byte: ignored on input
    _, view, _ = rgb_buffer(T, layout, shape)
    view.copy_(in_memory(T, layout, rgb, x))
    d = dm.rgb_desc(view, bgr)
    assert (d.pixel_step, d.width, d.height, d.nframes) == (step or 1, shape[2], shape[1], shape[0])
    assert d.channel_stride == (-1 if bgr else 1) * (1 if step else shape[1] * shape[2])
    got = dm.rgb_to_ycbcr(view, sub, bgr=bgr)
    assert [tuple(g.shape) for g in got] == plane_shapes(shape, sub)
    for name, g, w in zip(("y", "cb", "cr"), got, want_planes):
        assert np.array_equal(g.cpu().numpy(), w), name
    # and back, from planes of any bytes, into the same layout; the fourth byte comes out 255
    _, out, _ = rgb_buffer(T, layout, shape)
    ret = dm.ycbcr_to_rgb(*[gpu(T, p) for p in planes], out=out, bgr=bgr)
    assert ret is out
    assert T.equal(out, in_memory(T, layout, want_rgb))


def test_allocating_forms(T, dm):
    shape, sub = (2, 32, 48), "420"
    _, _, planes, want_rgb = case(shape, sub)
    dev = [gpu(T, p) for p in planes]
    for kw, layout in ((dict(), "rgb"), (dict(channels=4), "rgbx"), (dict(bgr=True), "bgr"),
                       (dict(channels=4, bgr=True), "bgrx"), (dict(planar=True), "planar"),
                       (dict(planar=True, bgr=True), "planar_reversed")):
        out = dm.ycbcr_to_rgb(*dev, **kw)
        assert tuple(out.shape) == shape + (4 if kw.get("channels") == 4 else 3,), kw
        assert out.is_contiguous() != bool(kw.get("planar")), kw
        assert T.equal(out, in_memory(T, layout, want_rgb)), kw
    # a [H, W, C] picture and [H, W] planes are one frame
    one = case((1, 16, 16), "444")
    got = dm.rgb_to_ycbcr(gpu(T, one[0][0]), "444")
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, one[1]))
    assert np.array_equal(dm.ycbcr_to_rgb(*[gpu(T, p[0]) for p in one[2]]).cpu().numpy(), one[3])


# ---- 3. padding: sources with padded strides read correctly, nothing outside width x height is written ----
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_padding(T, dm, layout, sub):
    shape = (2, 32, 48)
    rgb, want_planes, planes, want_rgb = case(shape, sub)
    _, bgr = LAYOUTS[layout]
    _, src, _ = rgb_buffer(T, layout, shape, pad=12, gap=40, fill=SENTINEL)
    src.copy_(in_memory(T, layout, rgb))
    dst = plane_buffers(T, plane_shapes(shape, sub), pad=24, gap=3)
    dm.rgb_to_ycbcr(src, sub, outs=[v for _, v in dst], bgr=bgr)
    for name, (buf, view), w in zip(("y", "cb", "cr"), dst, want_planes):
        assert np.array_equal(view.cpu().numpy(), w), name
        assert untouched_outside(T, buf, view), name
    # back: padded planes in, a padded picture out
    srcp = plane_buffers(T, plane_shapes(shape, sub), pad=8, gap=1)
    for (_, view), p in zip(srcp, planes):
        view.copy_(gpu(T, p))
    buf, out, _ = rgb_buffer(T, layout, shape, pad=20, gap=64, fill=SENTINEL)
    dm.ycbcr_to_rgb(*[v for _, v in srcp], out=out, bgr=bgr)
    assert T.equal(out, in_memory(T, layout, want_rgb))
    assert untouched_outside(T, buf, out)


# ---- 4. refusals: the library's invalid-argument code, DctqError from Python, nothing written ------------
def test_refusals(T, dm):
    L = dm.lib()
    f, h, w = 2, 32, 32
    rgb = T.full((f, h, w, 3), SENTINEL, dtype=T.uint8, device="cuda")
    big = [T.full((f, h, w), SENTINEL, dtype=T.uint8, device="cuda") for _ in range(3)]

    def call(rgb_kw=None, y=None, cb=None, cr=None, null=None):
        """Both entry points on a 4:2:0 call that is valid until the overrides are applied."""
        r = dm._Rgb(rgb.data_ptr(), 3 * w, 3 * w * h, 1, 3, w, h, f)
        for k, v in (rgb_kw or {}).items():
            setattr(r, k, v)
        pl = [dm._Plane(big[0].data_ptr(), w, w * h, w, h, f),
              dm._Plane(big[1].data_ptr(), w // 2, w * h // 4, w // 2, h // 2, f),
              dm._Plane(big[2].data_ptr(), w // 2, w * h // 4, w // 2, h // 2, f)]
        for p, kw in zip(pl, (y, cb, cr)):
            for k, v in (kw or {}).items():
                setattr(p, k, v)
        ptr = [None if null == k else C.byref(p) for k, p in enumerate(pl)]
        rcs = (L.dctq_rgb_to_ycbcr_planes(None if null == "rgb" else C.byref(r), *ptr, None),
               L.dctq_ycbcr_to_rgb_planes(*ptr, None if null == "rgb" else C.byref(r), None))
        T.cuda.synchronize()
        return rcs

    half = dict(width=12, height=12, stride=16, frame_stride=16 * 12)
    cases = {
        "luma 24 x 24 with 4:2:0 chroma": dict(rgb_kw=dict(width=24, height=24), y=dict(width=24, height=24),
                                               cb=half, cr=half),
        "chroma neither equal nor half": dict(cb=dict(width=8, height=8), cr=dict(width=8, height=8)),
        "chroma half in one direction only": dict(cb=dict(height=32), cr=dict(height=32)),
        "Cb and Cr differ": dict(cr=dict(width=32, height=32, stride=32, frame_stride=32 * 32)),
        "nframes of the picture": dict(rgb_kw=dict(nframes=1)),
        "nframes of a plane": dict(cb=dict(nframes=1)),
        "the picture is not luma's size": dict(rgb_kw=dict(width=16)),
        "pixel_step 2": dict(rgb_kw=dict(pixel_step=2)),
        "pixel_step 0": dict(rgb_kw=dict(pixel_step=0)),
        "base offset by 1 byte": dict(rgb_kw=dict(pixels=rgb.data_ptr() + 1)),
        "BGR at an aligned R byte": dict(rgb_kw=dict(channel_stride=-1)),  # its lowest byte is pixels - 2
        "stride not a multiple of 4": dict(rgb_kw=dict(stride=3 * w + 2)),
        "frame_stride not a multiple of 4": dict(rgb_kw=dict(frame_stride=3 * w * h + 2)),
        "stride below a row": dict(rgb_kw=dict(stride=3 * w - 4)),
        "interleaved channel_stride": dict(rgb_kw=dict(channel_stride=4)),
        "planar channel_stride not a multiple of 4": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h,
                                                                      channel_stride=w * h * f + 2)),
        "NULL picture": dict(null="rgb"),
        "NULL pixels": dict(rgb_kw=dict(pixels=None)),
        "NULL Y plane": dict(null=0),
        "NULL Cb plane": dict(null=1),
        "NULL Cr pixels": dict(cr=dict(pixels=None)),
        "plane width not a multiple of 8": dict(rgb_kw=dict(width=28), y=dict(width=28), cb=dict(width=14),
                                                cr=dict(width=14)),
        "frame_stride below a frame": dict(rgb_kw=dict(frame_stride=3 * w * h - 4)),
        "planar channel_stride 0": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h, channel_stride=0)),
        "planar channel_stride below a row": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h,
                                                              channel_stride=w - 4)),
        "planar channel_stride below a row, B first": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h,
                                                                       channel_stride=4 - w)),
        "picture width 0": dict(rgb_kw=dict(width=0)),
        "picture nframes 0": dict(rgb_kw=dict(nframes=0)),
        # what the any-size entry points take: 17 x 9 with planes of whole blocks
        "a 17 x 9 picture": dict(rgb_kw=dict(width=17, height=9), y=dict(height=16), cb=dict(height=8),
                                 cr=dict(height=8)),
        # 4:4:4, 2^28 blocks a plane but 2^31 patches: refused before anything is touched
        "2^31 patches": dict(rgb_kw=dict(width=1 << 16, height=1 << 16, nframes=4, stride=3 << 16, frame_stride=3 << 32),
                             **{p: dict(width=1 << 16, height=1 << 16, nframes=4, stride=1 << 16, frame_stride=1 << 32)
                                for p in ("y", "cb", "cr")}),
    }
    for name, kw in cases.items():
        assert call(**kw) == (EINVAL, EINVAL), name
        assert L.dctq_error_string(EINVAL), name
    assert all(bool((t == SENTINEL).all()) for t in [rgb, *big]), "a refused call wrote"
    assert call() == (0, 0)  # the harness itself is valid

    # the same from Python
    ok = T.zeros((f, h, w, 3), dtype=T.uint8, device="cuda")
    planes = lambda *s: [T.full(x, SENTINEL, dtype=T.uint8, device="cuda") for x in s]
    bad = {
        "luma 24 x 24 with 4:2:0": lambda: dm.rgb_to_ycbcr(ok[:, :24, :24].contiguous(), "420"),
        "chroma neither equal nor half": lambda: dm.rgb_to_ycbcr(ok, outs=planes((f, h, w), (f, 8, 8), (f, 8, 8))),
        "nframes": lambda: dm.rgb_to_ycbcr(ok, outs=planes((1, h, w), (1, h // 2, w // 2), (1, h // 2, w // 2))),
        "pixel stride 2": lambda: dm.rgb_desc(T.zeros(2 * w * h + 4, dtype=T.uint8, device="cuda")
                                              .as_strided((h, w, 3), (2 * w, 2, 1))),
        "base offset by 1 byte": lambda: dm.rgb_to_ycbcr(
            T.zeros(3 * w * h + 4, dtype=T.uint8, device="cuda")[1:1 + 3 * w * h].view(h, w, 3)),
        "stride not a multiple of 4": lambda: dm.rgb_to_ycbcr(
            T.zeros((3 * w + 2) * h, dtype=T.uint8, device="cuda").as_strided((h, w, 3), (3 * w + 2, 3, 1))),
        "a plane that is None": lambda: dm.rgb_to_ycbcr(ok, outs=[*planes((f, h, w), (f, h // 2, w // 2)), None]),
        "subsampling": lambda: dm.rgb_to_ycbcr(ok, "422"),
        "back: chroma neither equal nor half": lambda: dm.ycbcr_to_rgb(*planes((f, h, w), (f, 8, 8), (f, 8, 8))),
        "back: nframes": lambda: dm.ycbcr_to_rgb(*planes((f, h, w), (1, h // 2, w // 2), (f, h // 2, w // 2))),
        "back: out of another size": lambda: dm.ycbcr_to_rgb(*planes((f, h, w), (f, h // 2, w // 2), (f, h // 2, w // 2)),
                                                             out=ok[:, :16]),
        "back: channels 5": lambda: dm.ycbcr_to_rgb(*planes((f, h, w), (f, h // 2, w // 2), (f, h // 2, w // 2)),
                                                    channels=5),
        "back: a host plane": lambda: dm.ycbcr_to_rgb(T.zeros((f, h, w), dtype=T.uint8),
                                                      *planes((f, h // 2, w // 2), (f, h // 2, w // 2))),
    }
    for name, fn in bad.items():
        with pytest.raises(dm.DctqError):
            fn()
            pytest.fail(name)
    T.cuda.synchronize()
    assert not ok.any(), "a refused call wrote"


# ---- 5. the pipeline closes: RGB -> bytes -> RGB, library calls only ------------------------------------
@pytest.mark.parametrize("q,ad", [(50, 0), (90, 1)])
def test_pipeline_closes(T, dm, q, ad):
    shape = (2, 32, 48)
    rgb, want_planes, _, _ = case(shape, "420")
    plan = dm.Plan(q, ad)
    planes = list(dm.rgb_to_ycbcr(gpu(T, rgb)))
    for name, g, w in zip(("y", "cb", "cr"), planes, want_planes):
        assert np.array_equal(g.cpu().numpy(), w), name
    vns = None
    if ad:
        vns = [T.zeros(p.numel() // 64, dtype=T.int32, device="cuda") for p in planes]
        plan.forward_quant_planes(planes, var_nums=vns)
    _, boff, packed = plan.encode_bits_planes(planes)
    assert packed.numel() > 0
    dec = plan.decode_bits(packed, boff, shapes=[tuple(p.shape) for p in planes], var_nums=vns)
    back = dm.ycbcr_to_rgb(*dec)
    assert tuple(back.shape) == rgb.shape
    assert np.array_equal(back.cpu().numpy(), color_ref.inverse(*[d.cpu().numpy() for d in dec]))


# ---- 6. a side stream ----------------------------------------------------------------------------------
def test_side_stream(T, dm):
    shape = (3, 48, 80)
    rgb, want_planes, planes, want_rgb = case(shape, "420")
    src, dev = gpu(T, rgb), [gpu(T, p) for p in planes]
    T.cuda.synchronize()
    stream = T.cuda.Stream()
    with T.cuda.stream(stream):
        got = dm.rgb_to_ycbcr(src, stream=stream)
        back = dm.ycbcr_to_rgb(*dev, stream=stream)
    stream.synchronize()
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want_planes))
    assert np.array_equal(back.cpu().numpy(), want_rgb)
    dm.stream_release(stream)


# ---- 7. the C host ----------------------------------------------------------------------------------------
def test_frame_rgb_host(T, dm):
    exe = os.path.join(ROOT, "host", "frame_rgb")
    if not os.access(exe, os.X_OK):
        out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_rgb"], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([exe, "64", "48", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(l.split(":", 1) for l in out.stdout.split())
    assert (kv["ycc_equal"], kv["rgb_equal"], kv["padding_intact"], kv["abi_version"]) == ("1", "1", "1", "6"), kv
    assert int(kv["bytes_total"]) > 0 and float(kv["bytes_per_pixel"]) > 0
