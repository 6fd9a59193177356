"""GPU: pictures of any size at any alignment (dctq_rgb_to_ycbcr_pad_planes /
dctq_ycbcr_to_rgb_crop_planes / dctq_pad_planes; rgb_to_ycbcr(pad=True), ycbcr_to_rgb(size=),
pad_planes, compress / decompress through the container "frame c1").

The yardstick is tools/color_ref.py (forward_padded, inverse_cropped), numpy's edge padding and
tools/frame_ref.py: every case is compared byte for byte."""
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
import frame_ref  # noqa: E402

SENTINEL = 0xA5
EINVAL = -1
# W x H: one pixel; smaller than a patch; whole blocks; every patch kind in 4:2:0 (32 x 16 extended:
# patch columns 0-1 interior, 2 straddling, 3 outside); several patch rows with an odd last row
SIZES = [(1, 1), (7, 3), (16, 16), (17, 9), (33, 31)]
# layout -> (interleaved pixel step or 0 for planar, memory holds B first)
LAYOUTS = {"rgb": (3, False), "rgbx": (4, False), "bgr": (3, True), "bgrx": (4, True), "planar": (0, False)}
LEAD = 16  # bytes of the buffer in front of the picture, before the misalignment


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


def ext(n, m):
    return -(-n // m) * m


@functools.lru_cache(maxsize=None)
def case(f, h, w, sub):
    """A random picture [F, H, W, 3] with the reference planes of its extension, and random planes
    of the extended size (any bytes: the inverse clamps on both sides) with their cropped picture."""
    m, s = (16, 2) if sub == "420" else (8, 1)
    rng = np.random.default_rng(10000 * w + 100 * h + 10 * f + s)
    rgb = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    eh, ew = ext(h, m), ext(w, m)
    planes = (rng.integers(0, 256, (f, eh, ew), dtype=np.uint8),
              rng.integers(0, 256, (f, eh // s, ew // s), dtype=np.uint8),
              rng.integers(0, 256, (f, eh // s, ew // s), dtype=np.uint8))
    return rgb, color_ref.forward_padded(rgb, sub), planes, color_ref.inverse_cropped(*planes, h, w)


def rgb_view(T, layout, f, h, w, mis, padded, fill):
    """(buf, view): a flat u8 device buffer (random bytes for fill None, else the constant) and the
    [F, H, W, C] view of `layout` that starts LEAD + mis bytes into it.  padded: rows, frames and
    channel planes are separated by odd numbers of bytes; otherwise the picture is contiguous, so
    its rows rotate through every misalignment whenever a row is no multiple of 4 bytes."""
    step = LAYOUTS[layout][0]
    if step:
        row = w * step + (5 if padded else 0)
        frame = row * h + (7 if padded else 0)
        size, strides, span = (f, h, w, step), (frame, row, step, 1), f * frame
    else:
        row = w + (5 if padded else 0)
        plane = row * h + (3 if padded else 0)
        size, strides, span = (f, h, w, 3), (3 * plane, row, 1, plane), 3 * f * plane
    n = LEAD + mis + span + 16
    if fill is None:
        buf = gpu(T, np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8))
    else:
        buf = T.full((n,), fill, dtype=T.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, buf.as_strided(size, strides, LEAD + mis)


def in_memory(T, layout, rgb, x=None):
    """The logical picture rgb [F, H, W, 3] as the channels of the layout's view hold it."""
    step, bgr = LAYOUTS[layout]
    mem = rgb[..., ::-1] if bgr else rgb
    if step == 4:
        mem = np.concatenate([mem, x if x is not None else np.full(rgb.shape[:3] + (1,), 255, np.uint8)], axis=-1)
    return gpu(T, mem)


def plane_buffers(T, shapes):
    """[(buf, view)] per plane: [F, H, W] views into sentinel-filled buffers, rows padded by 8 bytes
    and frames separated by 3 rows (every dctq_plane rule still holds)."""
    out = []
    for f, h, w in shapes:
        buf = T.full((f, h + 3, w + 8), SENTINEL, dtype=T.uint8, device="cuda")
        out.append((buf, buf[:, :h, :w]))
    return out


def untouched_outside(T, buf, view):
    """Every byte of buf outside view is still the sentinel."""
    b = buf.clone()
    b.as_strided(view.size(), view.stride(), view.storage_offset()).fill_(SENTINEL)
    return bool((b == SENTINEL).all())


def forward_case(T, dm, layout, sub, f, h, w, mis, padded):
    """The planes of one forward call, with everything around them checked."""
    bgr = LAYOUTS[layout][1]
    rgb, want, _, _ = case(f, h, w, sub)
    _, src = rgb_view(T, layout, f, h, w, mis, padded, None)   # random bytes all around the picture
    x = np.random.default_rng(3).integers(0, 256, rgb.shape[:3] + (1,), dtype=np.uint8)
    src.copy_(in_memory(T, layout, rgb, x))                     # the fourth byte: ignored on input
    dst = plane_buffers(T, [p.shape for p in want])
    got = dm.rgb_to_ycbcr(src, sub, outs=[v for _, v in dst], bgr=bgr, pad=True)
    tag = (layout, sub, f, h, w, mis, padded)
    for name, g, (buf, view), p in zip(("y", "cb", "cr"), got, dst, want):
        assert g is view
        assert np.array_equal(view.cpu().numpy(), p), (name, tag)
        assert untouched_outside(T, buf, view), (name, tag)
    return [v for _, v in dst]


def inverse_case(T, dm, layout, sub, f, h, w, mis, padded):
    bgr = LAYOUTS[layout][1]
    _, _, planes, want = case(f, h, w, sub)
    buf, out = rgb_view(T, layout, f, h, w, mis, padded, SENTINEL)
    ret = dm.ycbcr_to_rgb(*[gpu(T, p) for p in planes], out=out, bgr=bgr, size=(h, w))
    tag = (layout, sub, f, h, w, mis, padded)
    assert ret is out
    assert T.equal(out, in_memory(T, layout, want)), tag          # the fourth byte comes out 255
    assert untouched_outside(T, buf, out), tag                    # rows' tails, gaps, the bytes before the base
    return out


# ---- 5 and 6. forward and inverse against color_ref, every layout, size, misalignment and stride --------
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_forward_padded(T, dm, layout, sub):
    for w, h in SIZES:
        for f in (1, 3):
            for mis in range(4):
                for padded in (False, True):
                    forward_case(T, dm, layout, sub, f, h, w, mis, padded)


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_inverse_cropped(T, dm, layout, sub):
    for w, h in SIZES:
        for f in (1, 3):
            for mis in range(4):
                for padded in (False, True):
                    inverse_case(T, dm, layout, sub, f, h, w, mis, padded)


def test_allocating_forms(T, dm):
    rgb, want, planes, back = case(3, 9, 17, "420")
    got = dm.rgb_to_ycbcr(gpu(T, rgb), pad=True)
    assert [tuple(g.shape) for g in got] == [(3, 16, 32), (3, 8, 16), (3, 8, 16)]
    assert all(np.array_equal(g.cpu().numpy(), p) for g, p in zip(got, want))
    dev = [gpu(T, p) for p in planes]
    for kw, layout in ((dict(), "rgb"), (dict(channels=4, bgr=True), "bgrx"), (dict(planar=True), "planar")):
        out = dm.ycbcr_to_rgb(*dev, size=(9, 17), **kw)
        assert tuple(out.shape) == (3, 9, 17, 4 if kw.get("channels") == 4 else 3), kw
        assert T.equal(out, in_memory(T, layout, back)), kw


# ---- 7. agreement with the aligned entry points -------------------------------------------------------------
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_agrees_with_the_aligned_entry_points(T, dm, layout, sub):
    f, h, w = 2, 48, 32
    bgr = LAYOUTS[layout][1]
    rgb, want, planes, back = case(f, h, w, sub)
    _, src = rgb_view(T, layout, f, h, w, 0, False, 0)
    src.copy_(in_memory(T, layout, rgb))
    old, new = dm.rgb_to_ycbcr(src, sub, bgr=bgr), dm.rgb_to_ycbcr(src, sub, bgr=bgr, pad=True)
    for a, b, p in zip(old, new, want):
        assert T.equal(a, b) and np.array_equal(b.cpu().numpy(), p)
    dev = [gpu(T, p) for p in planes]
    outs = []
    for kw in (dict(), dict(size=(h, w))):
        buf, out = rgb_view(T, layout, f, h, w, 0, False, SENTINEL)
        dm.ycbcr_to_rgb(*dev, out=out, bgr=bgr, **kw)
        assert untouched_outside(T, buf, out)
        outs.append(out)
    assert T.equal(outs[0], outs[1]) and T.equal(outs[1], in_memory(T, layout, back))


# ---- 8. more than one trip of the grid-stride loop ----------------------------------------------------------
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_grid_stride_trips(T, dm, layout, sub):
    f, h, w = 3, 31, 33
    free_planes = forward_case(T, dm, layout, sub, f, h, w, 1, True)
    free_rgb = inverse_case(T, dm, layout, sub, f, h, w, 1, True)
    with dm.grid_limit(1):
        planes = forward_case(T, dm, layout, sub, f, h, w, 1, True)
        assert dm.last_grid() == 1   # 288 patches (4:2:0) or 480 (4:4:4) for one workgroup of 256 lanes: two trips
        rgb = inverse_case(T, dm, layout, sub, f, h, w, 1, True)
        assert dm.last_grid() == 1
    assert all(T.equal(a, b) for a, b in zip(planes, free_planes)) and T.equal(rgb, free_rgb)


# ---- 9. plain planes ----------------------------------------------------------------------------------------
def pad_planes_case(T, dm):
    """Four planes in one call, at odd addresses and strides: (sources, expected, call)."""
    rng = np.random.default_rng(9)
    shapes = [(1, 1, 1), (2, 5, 13), (1, 8, 24), (1, 17, 9)]  # F, H, W
    srcs, want = [], []
    for k, (f, h, w) in enumerate(shapes):
        row, frame = w + 2 * k + 1, (w + 2 * k + 1) * h + 5
        n = 3 + k + f * frame
        a = rng.integers(0, 256, n, dtype=np.uint8)
        buf = gpu(T, a)
        view = buf.as_strided((f, h, w), (frame, row, 1), 1 + k)
        srcs.append(view)
        pic = np.lib.stride_tricks.as_strided(a[1 + k:], (f, h, w), (frame, row, 1))
        want.append(np.pad(pic, ((0, 0), (0, -h % 8), (0, -w % 8)), mode="edge"))
    return srcs, want


def test_pad_planes(T, dm):
    srcs, want = pad_planes_case(T, dm)
    dst = plane_buffers(T, [p.shape for p in want])
    got = dm.pad_planes(srcs, outs=[v for _, v in dst])
    for k, (g, (buf, view), p) in enumerate(zip(got, dst, want)):
        assert g is view
        assert np.array_equal(view.cpu().numpy(), p), k     # 24 x 8 is a plain copy
        assert untouched_outside(T, buf, view), k
    alloc = dm.pad_planes(srcs)
    assert all(np.array_equal(a.cpu().numpy(), p) for a, p in zip(alloc, want))
    one = dm.pad_planes([srcs[3][0]])                        # [H, W] is one frame
    assert np.array_equal(one[0].cpu().numpy(), want[3])
    # more than one trip of the grid-stride loop: 40 x 13 = 520 patches for one workgroup of 256 lanes
    wide = np.random.default_rng(4).integers(0, 256, (1, 37, 99), dtype=np.uint8)
    with dm.grid_limit(1):
        again = dm.pad_planes([*srcs[:3], gpu(T, wide)])
        assert dm.last_grid() == 1
    assert all(T.equal(a, b) for a, b in zip(again[:3], alloc))
    assert np.array_equal(again[3].cpu().numpy(), np.pad(wide, ((0, 0), (0, 3), (0, 5)), mode="edge"))


# ---- 10. refusals: the library's invalid-argument code, DctqError from Python, nothing written -------------
def test_refusals(T, dm):
    L = dm.lib()
    f, h, w = 2, 9, 17
    rgb = T.full((f * h * w * 3 + 8,), SENTINEL, dtype=T.uint8, device="cuda")
    big = [T.full((f, 16, 32), SENTINEL, dtype=T.uint8, device="cuda") for _ in range(3)]

    def call(rgb_kw=None, y=None, cb=None, cr=None, null=None):
        """Both colour entry points on a 4:2:0 call that is valid until the overrides are applied."""
        r = dm._Rgb(rgb.data_ptr() + 1, 3 * w, 3 * w * h, 1, 3, w, h, f)
        for k, v in (rgb_kw or {}).items():
            setattr(r, k, v)
        pl = [dm._Plane(big[0].data_ptr(), 32, 32 * 16, 32, 16, f),
              dm._Plane(big[1].data_ptr(), 16, 16 * 8, 16, 8, f),
              dm._Plane(big[2].data_ptr(), 16, 16 * 8, 16, 8, f)]
        for p, kw in zip(pl, (y, cb, cr)):
            for k, v in (kw or {}).items():
                setattr(p, k, v)
        ptr = [None if null == k else C.byref(p) for k, p in enumerate(pl)]
        rcs = (L.dctq_rgb_to_ycbcr_pad_planes(None if null == "rgb" else C.byref(r), *ptr, None),
               L.dctq_ycbcr_to_rgb_crop_planes(*ptr, None if null == "rgb" else C.byref(r), None))
        T.cuda.synchronize()
        return rcs

    cases = {
        "y not W' x H': too wide": dict(y=dict(width=48, stride=48, frame_stride=48 * 16),
                                        cb=dict(width=24, stride=24, frame_stride=24 * 8),
                                        cr=dict(width=24, stride=24, frame_stride=24 * 8)),
        "y not W' x H': too tall": dict(y=dict(height=32, frame_stride=32 * 32), cb=dict(height=16, frame_stride=16 * 16),
                                        cr=dict(height=16, frame_stride=16 * 16)),
        "y of the true size": dict(y=dict(width=17, height=9)),
        "chroma neither equal nor half": dict(cb=dict(width=8), cr=dict(width=8)),
        "chroma half in one direction only": dict(cb=dict(height=16, frame_stride=16 * 16),
                                                  cr=dict(height=16, frame_stride=16 * 16)),
        "Cb and Cr differ": dict(cr=dict(width=32, height=16, stride=32, frame_stride=32 * 16)),
        "4:4:4 planes for a size that needs 24 x 16": dict(cb=dict(width=32, height=16, stride=32, frame_stride=512),
                                                           cr=dict(width=32, height=16, stride=32, frame_stride=512)),
        "nframes of the picture": dict(rgb_kw=dict(nframes=1)),
        "nframes of a plane": dict(cb=dict(nframes=1)),
        "width 0": dict(rgb_kw=dict(width=0)),
        "height 0": dict(rgb_kw=dict(height=0)),
        "pixel_step 2": dict(rgb_kw=dict(pixel_step=2)),
        "stride below a row": dict(rgb_kw=dict(stride=3 * w - 1)),
        "frame_stride below a frame": dict(rgb_kw=dict(frame_stride=3 * w * h - 1)),
        "interleaved channel_stride": dict(rgb_kw=dict(channel_stride=4)),
        "planar channel_stride 0": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h, channel_stride=0)),
        "NULL picture": dict(null="rgb"),
        "NULL pixels": dict(rgb_kw=dict(pixels=None)),
        "NULL Y plane": dict(null=0),
        "NULL Cr plane": dict(null=2),
        "NULL Cb pixels": dict(cb=dict(pixels=None)),
        "a misaligned plane": dict(y=dict(pixels=big[0].data_ptr() + 4)),
        "nframes 0": dict(rgb_kw=dict(nframes=0)),
        "pixel_step 0": dict(rgb_kw=dict(pixel_step=0)),
        "planar channel_stride below a row": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h,
                                                              channel_stride=w - 1)),
        "planar channel_stride below a row, B first": dict(rgb_kw=dict(pixel_step=1, stride=w, frame_stride=w * h,
                                                                       channel_stride=1 - w)),
        # 4:4:4, 2^28 blocks a plane but 2^31 patches: refused before anything is touched
        "2^31 patches": dict(rgb_kw=dict(width=65529, height=65529, nframes=4, stride=3 << 16, frame_stride=3 << 32),
                             **{p: dict(width=1 << 16, height=1 << 16, nframes=4, stride=1 << 16, frame_stride=1 << 32)
                                for p in ("y", "cb", "cr")}),
    }
    for name, kw in cases.items():
        assert call(**kw) == (EINVAL, EINVAL), name
    assert all(bool((t == SENTINEL).all()) for t in [rgb, *big]), "a refused call wrote"

    # dctq_pad_planes
    src = T.full((13 * 5 + 8,), SENTINEL, dtype=T.uint8, device="cuda")
    dst = T.full((4, 8, 16), SENTINEL, dtype=T.uint8, device="cuda")

    def pad(n=1, s=None, d=None, null=None):
        sp = (dm._Plane * 4)(*[dm._Plane(src.data_ptr() + 1, 13, 13 * 5, 13, 5, 1) for _ in range(4)])
        dp = (dm._Plane * 4)(*[dm._Plane(dst[k].data_ptr(), 16, 16 * 8, 16, 8, 1) for k in range(4)])
        for k, v in (s or {}).items():
            setattr(sp[0], k, v)
        for k, v in (d or {}).items():
            setattr(dp[0], k, v)
        rc = L.dctq_pad_planes(None if null == "src" else sp, None if null == "dst" else dp, n, None)
        T.cuda.synchronize()
        return rc

    pads = {
        "nplanes 0": dict(n=0), "nplanes 5": dict(n=5), "NULL src": dict(null="src"), "NULL dst": dict(null="dst"),
        "NULL src pixels": dict(s=dict(pixels=None)), "NULL dst pixels": dict(d=dict(pixels=None)),
        "src == dst": dict(s=dict(pixels=dst.data_ptr())),
        "dst of src's size": dict(d=dict(width=13, height=5)),
        "dst too wide": dict(d=dict(width=24, stride=24)),
        "nframes differ": dict(s=dict(nframes=2, frame_stride=13 * 5)),
        "src width 0": dict(s=dict(width=0)),
        "src stride below a row": dict(s=dict(stride=12)),
        "dst misaligned": dict(d=dict(pixels=dst.data_ptr() + 1)),
        "src == dst of another plane": dict(n=2, s=dict(pixels=dst[1].data_ptr())),
        "dst rounded down": dict(d=dict(width=8)),
        "dst too tall": dict(d=dict(height=16, frame_stride=16 * 16)),
        "dst with more frames": dict(d=dict(nframes=2)),
        "src height 0": dict(s=dict(height=0)),
        "src nframes 0": dict(s=dict(nframes=0)),
        "src frame_stride below a frame": dict(s=dict(nframes=2, frame_stride=13 * 5 - 1), d=dict(nframes=2)),
        # 2^28 blocks but 2^31 patches: refused before anything is touched
        "2^31 patches": dict(s=dict(width=65529, height=65529, nframes=4, stride=1 << 16, frame_stride=1 << 32),
                             d=dict(width=1 << 16, height=1 << 16, nframes=4, stride=1 << 16, frame_stride=1 << 32)),
    }
    for name, kw in pads.items():
        assert pad(**kw) == EINVAL, name
    assert bool((src == SENTINEL).all()) and bool((dst == SENTINEL).all()), "a refused call wrote"
    assert L.dctq_error_string(EINVAL)

    # the harnesses themselves are valid
    assert call() == (0, 0) and pad() == 0 and pad(n=2) == 0

    # the aligned entry points refuse what they refused: a 24 x 24 picture in 4:2:0
    r = dm._Rgb(big[0].data_ptr(), 72, 72 * 24, 1, 3, 24, 24, 1)
    pl = [dm._Plane(big[0].data_ptr(), 24, 24 * 24, 24, 24, 1), dm._Plane(big[1].data_ptr(), 16, 16 * 12, 12, 12, 1),
          dm._Plane(big[2].data_ptr(), 16, 16 * 12, 12, 12, 1)]
    assert L.dctq_rgb_to_ycbcr_planes(C.byref(r), *map(C.byref, pl), None) == EINVAL
    assert L.dctq_ycbcr_to_rgb_planes(*map(C.byref, pl), C.byref(r), None) == EINVAL

    # one rule at a time: what the any-size entry points take and the aligned ones refuse
    pic = T.zeros(1024, dtype=T.uint8, device="cuda")

    def four(sub, w=None, h=None, **rgb_kw):
        """(any-size forward, inverse, aligned forward, inverse) on one frame of whole blocks, 16 x 16
        in 4:2:0 or 8 x 8 in 4:4:4, that all four take until the overrides are applied; w x h: the
        picture's size when its planes are its extension."""
        m, s = (16, 2) if sub == "420" else (8, 1)
        w, h = w or m, h or m
        ew, eh = ext(w, m), ext(h, m)
        r = dm._Rgb(pic.data_ptr(), 3 * w + (-3 * w) % 4, 0, 1, 3, w, h, 1)
        for k, v in rgb_kw.items():
            setattr(r, k, v)
        pl = [C.byref(dm._Plane(big[k].data_ptr(), ew // d, 0, ew // d, eh // d, 1)) for k, d in enumerate((1, s, s))]
        rcs = (L.dctq_rgb_to_ycbcr_pad_planes(C.byref(r), *pl, None), L.dctq_ycbcr_to_rgb_crop_planes(*pl, C.byref(r), None),
               L.dctq_rgb_to_ycbcr_planes(C.byref(r), *pl, None), L.dctq_ycbcr_to_rgb_planes(*pl, C.byref(r), None))
        T.cuda.synchronize()
        return rcs

    only_any_size = (0, 0, EINVAL, EINVAL)
    for sub, n in (("420", 16), ("444", 8)):
        assert four(sub) == (0, 0, 0, 0), sub
        assert four(sub, pixels=pic.data_ptr() + 1) == only_any_size, sub
        assert four(sub, pixels=pic.data_ptr() + 4, channel_stride=-1) == only_any_size, sub  # B at +2
        assert four(sub, pixels=pic.data_ptr() + 2, channel_stride=-1) == (0, 0, 0, 0), sub
        assert four(sub, stride=3 * n + 2) == only_any_size, sub
        assert four(sub, frame_stride=2) == only_any_size, sub
        planar = dict(pixel_step=1, stride=n)
        assert four(sub, channel_stride=n * n, **planar) == (0, 0, 0, 0), sub
        assert four(sub, channel_stride=n * n + 2, **planar) == only_any_size, sub
        assert four(sub, w=17, h=9) == only_any_size, sub                                    # 32 x 16 or 24 x 16 planes
        assert four(sub, w=n - 1) == only_any_size, sub

    # the same from Python
    ok = T.zeros((f, h, w, 3), dtype=T.uint8, device="cuda")
    planes = lambda *s: [T.full(x, SENTINEL, dtype=T.uint8, device="cuda") for x in s]
    half = [(f, 16, 32), (f, 8, 16), (f, 8, 16)]
    bad = {
        "no pad: 17 x 9": lambda: dm.rgb_to_ycbcr(ok),
        "no pad: 24 x 24 in 4:2:0": lambda: dm.rgb_to_ycbcr(T.zeros((24, 24, 3), dtype=T.uint8, device="cuda")),
        "y not W' x H'": lambda: dm.rgb_to_ycbcr(ok, pad=True, outs=planes((f, 16, 24), (f, 8, 12), (f, 8, 12))),
        "chroma neither equal nor half": lambda: dm.rgb_to_ycbcr(ok, pad=True, outs=planes(half[0], (f, 8, 8), (f, 8, 8))),
        "nframes": lambda: dm.rgb_to_ycbcr(ok, pad=True, outs=planes((1, 16, 32), (1, 8, 16), (1, 8, 16))),
        "pixel stride 2": lambda: dm.rgb_to_ycbcr(T.zeros(2 * w * h + 4, dtype=T.uint8, device="cuda")
                                                  .as_strided((h, w, 3), (2 * w, 2, 1)), pad=True),
        "rows overlap": lambda: dm.rgb_to_ycbcr(T.zeros(3 * w * h, dtype=T.uint8, device="cuda")
                                                .as_strided((h, w, 3), (3 * w - 1, 3, 1)), pad=True),
        "back: size does not round up to y": lambda: dm.ycbcr_to_rgb(*planes(*half), size=(9, 16)),
        "back: size 0": lambda: dm.ycbcr_to_rgb(*planes(*half), size=(0, 17)),
        "back: out of the padded size": lambda: dm.ycbcr_to_rgb(*planes(*half), size=(9, 17),
                                                                out=T.zeros((f, 16, 32, 3), dtype=T.uint8, device="cuda")),
        "pad_planes: none": lambda: dm.pad_planes([]),
        "pad_planes: five": lambda: dm.pad_planes(planes(*[(5, 13)] * 5)),
        "pad_planes: outs of the source's size": lambda: dm.pad_planes([ok[..., 0].contiguous()],
                                                                       outs=planes((f, h, w))),
        "pad_planes: a host plane": lambda: dm.pad_planes([T.zeros((5, 13), dtype=T.uint8)]),
    }
    for name, fn in bad.items():
        with pytest.raises(dm.DctqError):
            fn()
            pytest.fail(name)
    T.cuda.synchronize()
    assert not ok.any(), "a refused call wrote"


# ---- 11. the pipeline closes: a picture of any size -> bytes -> the picture's size ----------------------------
def u32(t):
    return t.cpu().numpy().view(np.uint32)


def host_bytes(t):
    return t.cpu().numpy().tobytes()


def manual(T, dm, planes, q, adaptive):
    """The stream of `planes` made call by call, as compress makes it: (bytes, offsets, var_nums, decoded)."""
    plan = dm.Plan(q, adaptive)
    vns = None
    if adaptive:
        nbs = [p.numel() // 64 for p in planes]
        coef = T.empty((sum(nbs), 64), dtype=T.int16, device="cuda")
        vn = T.empty(sum(nbs), dtype=T.int32, device="cuda")
        vns = list(T.split(vn, nbs))
        plan.forward_quant_planes(planes, outs=list(T.split(coef, nbs)), var_nums=vns)
        off, sym = dm.rle_encode(coef)
        by, boff = dm.bits_pack(sym, off)
    else:
        _, boff, by = plan.encode_bits_planes(planes)
    dec = plan.decode_bits(by, boff, shapes=[tuple(p.shape) for p in planes], var_nums=vns)
    return by, boff, vns, dec


def picture(T, dm, f, h, w):
    """A smooth picture [F, H, W, 3] of any size: three synthetic planes, cropped."""
    eh, ew = ext(h, 8), ext(w, 8)
    return T.stack([dm.synth(11 + c, "smooth", ew, eh, f)[:, :h, :w] for c in range(3)], dim=-1).contiguous()


@pytest.mark.parametrize("f,h,w,q,adaptive", [(2, 30, 50, 50, False), (2, 30, 50, 90, True), (1, 1080, 1920, 50, False)],
                         ids=["50x30x2-q50", "50x30x2-q90-adaptive", "1920x1080-q50"])
def test_pipeline_closes(T, dm, f, h, w, q, adaptive):
    x = picture(T, dm, f, h, w)
    box = dm.compress(x, q, adaptive)                       # raised DctqError before there was padding
    raw = host_bytes(box)
    assert raw[:8] == b"DCTQFRC1"
    planes = list(dm.rgb_to_ycbcr(x, pad=True))
    shapes = [tuple(p.shape) for p in planes]
    assert shapes[0] == (f, ext(h, 16), ext(w, 16))
    by, boff, vns, dec = manual(T, dm, planes, q, adaptive)
    crops = [(-h % 16, -w % 16), (0, 0), (0, 0)]
    ref = frame_ref.pack(by.cpu().numpy(), u32(boff), shapes, q, adaptive,
                         None if vns is None else [v.cpu().numpy() for v in vns], colour=True, crops=crops)
    assert raw == ref, "the container differs from tools/frame_ref.py pack"
    d = dm.frame_unpack(box)
    assert d["crops"] == crops and d["shapes"] == shapes and d["colour"]
    want = dm.ycbcr_to_rgb(*dec, size=(h, w))
    for source in (box, raw):
        got = dm.decompress(source)
        assert tuple(got.shape) == tuple(x.shape)
        assert T.equal(got, want)
    assert np.array_equal(want.cpu().numpy(), color_ref.inverse_cropped(*[p.cpu().numpy() for p in dec], h, w))


@pytest.mark.parametrize("q,adaptive", [(50, False), (90, True)])
def test_pipeline_closes_for_plain_planes(T, dm, q, adaptive):
    srcs = [dm.synth(5, "smooth", 16, 24, 1)[:, :21, :13], dm.synth(6, "uniform", 8, 8, 1)]  # 13 x 21 and 8 x 8
    box = dm.compress(srcs, q, adaptive)
    raw = host_bytes(box)
    assert raw[:8] == b"DCTQFRC1"
    padded = dm.pad_planes(srcs)
    assert np.array_equal(padded[0].cpu().numpy(), np.pad(srcs[0].cpu().numpy(), ((0, 0), (0, 3), (0, 3)), mode="edge"))
    shapes = [tuple(p.shape) for p in padded]
    by, boff, vns, dec = manual(T, dm, padded, q, adaptive)
    crops = [(3, 3), (0, 0)]
    assert raw == frame_ref.pack(by.cpu().numpy(), u32(boff), shapes, q, adaptive,
                                 None if vns is None else [v.cpu().numpy() for v in vns], crops=crops)
    got = dm.decompress(box)
    assert [tuple(g.shape) for g in got] == [(1, 21, 13), (1, 8, 8)]
    assert T.equal(got[0], dec[0][:, :21, :13]) and T.equal(got[1], dec[1])
    assert frame_ref.parse(raw)["crops"] == crops and dm.frame_unpack(raw)["crops"] == crops


def test_whole_blocks_still_give_frame_v1(T, dm):
    x = picture(T, dm, 1, 1088, 1920)
    box = host_bytes(dm.compress(x, 50))
    planes = list(dm.rgb_to_ycbcr(x))
    by, boff, _, _ = manual(T, dm, planes, 50, False)
    assert box[:8] == b"DCTQFRM1"
    assert box == frame_ref.pack(by.cpu().numpy(), u32(boff), [tuple(p.shape) for p in planes], 50, colour=True)
    assert dm.frame_unpack(box)["crops"] is None
    # frame_pack with no crop, said either way, is frame v1 too
    shapes = [tuple(p.shape) for p in planes]
    assert host_bytes(dm.frame_pack(by, boff, shapes, 50, colour=True, crops=[(0, 0)] * 3)) == box


# ---- 12. hostile containers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [True, False])
def test_every_refusal_and_nothing_decoded(T, dm, colour, monkeypatch):
    src = picture(T, dm, 2, 30, 50) if colour else [dm.synth(5, "smooth", 16, 24, 1)[:, :21, :13]]
    good = host_bytes(dm.compress(src, 50))
    assert good[:8] == b"DCTQFRC1"
    dm.decompress(good)
    decoded = []
    real = dm.Plan.decode_bits
    monkeypatch.setattr(dm.Plan, "decode_bits", lambda self, *a, **kw: decoded.append(1) or real(self, *a, **kw))
    cases = frame_ref.refusal_cases(good)
    assert len(cases) > 20
    for rule, bad in cases:
        with pytest.raises(frame_ref.FrameError):
            frame_ref.parse(bad)
        for source in (bad, gpu(T, np.frombuffer(bad, np.uint8).copy())):
            with pytest.raises(dm.DctqError):
                dm.frame_unpack(source)
                pytest.fail(f"frame_unpack accepted: {rule}")
            with pytest.raises(dm.DctqError):
                dm.decompress(source)
                pytest.fail(f"decompress accepted: {rule}")
    T.cuda.synchronize()
    assert not decoded, "a refused container reached the decoder"
    dm.decompress(good)
    assert decoded == [1]


# ---- 13. the C host -------------------------------------------------------------------------------------------
def test_color_pad_host(T, dm):
    exe = os.path.join(ROOT, "host", "color_pad")
    if not os.access(exe, os.X_OK):
        out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "color_pad"], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(l.split("=", 1) for l in out.stdout.split())
    assert (kv["ycc_equal"], kv["rgb_equal"], kv["padding_intact"], kv["abi_version"]) == ("1", "1", "1", "6"), kv
