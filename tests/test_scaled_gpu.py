"""GPU: decode at 1/2, 1/4 and 1/8 size straight from a "bits v1" stream --
dctq_decode_bits_window_scaled_planes, Plan.decode_bits_scaled and decompress(scale=).

The yardstick is always tools/scaled_ref.py (the definition of include/dct_amd.h in plain numpy)
applied to the coefficients bits_decode returns for the same bytes; bits_decode is pinned to
tools/bits_ref.py by the rest of the suite.  Pixels must be equal byte for byte.

Stored set: a 4:2:0 trio of 2 frames, luma 1040 x 48 (130 blocks a row: runs of 64, 64 and 2),
chroma 520 x 24 (65 blocks a row: runs of 64 and 1), and one 24 x 16 plane, all in one launch:
2 352 blocks, 64 runs for the whole planes.

What a case can show depends on its plan (tests/test_window_gpu.py says why): below q100 a
non-adaptive plan's pictures stay within a level or two of 128, on adaptive plans and at q100
they span the range.  The sweep keeps every plan, and the poison, sentinel and grid-limit cases
use plans whose pictures show a misplaced block."""
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
import scaled_ref  # noqa: E402
import window_ref  # noqa: E402

SHAPES = [(2, 48, 1040), (2, 24, 520), (2, 24, 520), (2, 16, 24)]
NBS = [f * (h // 8) * (w // 8) for f, h, w in SHAPES]
SCALES = (2, 4, 8)
SENTINEL = 0xA5
STAGE = 2560  # bits_core.h kBitsStage
ALL = [((0, f), (0, h), (0, w)) for f, h, w in SHAPES]


def blk(f, y, x):
    """Block ranges -> a window in frames and pixels."""
    return (f, (8 * y[0], 8 * y[1]), (8 * x[0], 8 * x[1]))


WINDOWS = {
    "whole": ALL,
    # 33 blocks wide: a half plus one
    "33 wide": [blk((0, 2), (0, 6), (2, 35)), blk((0, 2), (0, 3), (2, 35)), blk((0, 2), (0, 3), (32, 65)), blk((0, 2), (0, 2), (0, 3))],
    "1 wide": [blk((0, 2), (0, 6), (129, 130)), blk((0, 2), (0, 3), (64, 65)), blk((0, 2), (0, 3), (0, 1)), blk((0, 2), (0, 2), (2, 3))],
    # one frame that is not the stream's first
    "frame 1": [((1, 2), (0, h), (0, w)) for _, h, w in SHAPES],
    # an origin away from block 0, rows and columns
    "origin": [blk((0, 2), (1, 5), (3, 100)), blk((1, 2), (1, 3), (1, 65)), blk((0, 1), (2, 3), (63, 65)), blk((1, 2), (1, 2), (1, 3))],
}
PLANS = [(50, 0), (90, 0), (50, 1)]


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


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def plan_of(q, adaptive):
    import dct_amd
    return dct_amd.Plan(q, adaptive)


@functools.lru_cache(maxsize=None)
def table(q, adaptive):
    import dct_amd
    return dct_amd.debug_tables(q, adaptive)[3].reshape(8, 8)


@functools.lru_cache(maxsize=None)
def var_nums():
    """One set of var_nums for every adaptive case: those of the uniform planes."""
    import dct_amd
    import torch
    planes = [dct_amd.synth(900 + k, "uniform", s[2], s[1], s[0]) for k, s in enumerate(SHAPES)]
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in NBS]
    plan_of(50, 1).forward_quant_planes(planes, var_nums=vns)
    torch.cuda.synchronize()
    return vns


@functools.lru_cache(maxsize=None)
def stream_of(kind, q, adaptive):
    """The stored set's packed stream and its var_nums: (bytes, offsets, var_nums)."""
    import dct_amd
    import torch
    plan = plan_of(q, adaptive)
    planes = [dct_amd.synth(900 + k, kind, s[2], s[1], s[0]) for k, s in enumerate(SHAPES)]
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in NBS]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, boff, by = plan.encode_bits_planes(planes)
    torch.cuda.synchronize()
    return by, boff, vns if adaptive else None


class Ref:
    """scaled_ref over the coefficients bits_decode gives for (bytes, offsets): computed once per
    stream and scale for the whole planes and left unchanged; a window is its slice."""

    def __init__(self, dm, by, boff, q, adaptive, vns):
        self.coef = dm.bits_decode(by, boff).cpu().numpy()
        self.q, self.adaptive = q, adaptive
        self.vns = None if vns is None else [v.cpu().numpy() for v in vns]
        self.whole = {}

    def __call__(self, scale, windows):
        if scale not in self.whole:
            self.whole[scale] = scaled_ref.planes(self.coef, SHAPES, table(self.q, self.adaptive), scale,
                                                  self.adaptive, self.vns)
            for p in self.whole[scale]:
                p.setflags(write=False)
        return [p[f0:f1, y0 // scale:y1 // scale, x0 // scale:x1 // scale]
                for p, ((f0, f1), (y0, y1), (x0, x1)) in zip(self.whole[scale], windows)]


@functools.lru_cache(maxsize=None)
def ref_of(kind, q, adaptive):
    import dct_amd
    by, boff, vns = stream_of(kind, q, adaptive)
    return Ref(dct_amd, by, boff, q, adaptive, vns)


def assert_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(g, w), (what, f"plane {k}", int((g != w).sum()), "pixels differ",
                                      np.argwhere(g != w)[:4].tolist())


def sweep(plan, by, boff, vns, ref, what):
    for scale in SCALES:
        for name, windows in WINDOWS.items():
            got = plan.decode_bits_scaled(by, boff, SHAPES, scale, windows, var_nums=vns)
            assert_equal(got, ref(scale, windows), (*what, scale, name))
        got = plan.decode_bits_scaled(by, boff, SHAPES, scale, var_nums=vns)      # windows=None: the whole planes
        assert_equal(got, ref(scale, ALL), (*what, scale, "default"))


# ---- 1. every window, scale, content and plan ----------------------------------------------------------
def test_the_runs_are_what_the_module_says():
    r = window_ref.runs(SHAPES, ALL)
    assert len(r) == 64 and sorted(set(r[:, 1].tolist())) == [1, 2, 3, 64]
    assert sorted(set(window_ref.runs(SHAPES, WINDOWS["33 wide"])[:, 1].tolist())) == [3, 33]


@pytest.mark.parametrize("q,adaptive", PLANS)
@pytest.mark.parametrize("kind", ["smooth", "uniform"])
def test_scaled_equals_the_definition(T, dm, kind, q, adaptive):
    by, boff, vns = stream_of(kind, q, adaptive)
    ref = ref_of(kind, q, adaptive)
    if adaptive and kind == "uniform":  # pictures in which a misplaced block shows (at 1/8 noise is its blocks' means)
        assert all(int(p.max()) - int(p.min()) > 64 for p in ref(2, ALL)[:3])
    sweep(plan_of(q, adaptive), by, boff, vns, ref, (kind, q, adaptive))


@pytest.mark.parametrize("adaptive", [0, 1])
def test_extremes_at_q100(T, dm, adaptive):
    """Dense halves beyond the 2 560 B stage: the chunk loop runs, with the early stop in every chunk."""
    by, boff, vns = stream_of("extreme", 100, adaptive)
    off = u32(boff).astype(np.int64)
    by2, boff2, _ = stream_of("uniform", 100, 0)
    off2 = u32(boff2).astype(np.int64)
    print(f"first half of block 0: extreme {off[32] - off[0]} B, uniform {off2[32] - off2[0]} B")
    assert max(off[32] - off[0], off2[32] - off2[0]) > STAGE
    ref = ref_of("extreme", 100, adaptive)
    assert all(int(p.max()) - int(p.min()) > 128 for p in ref(2, ALL)[:3])
    sweep(plan_of(100, adaptive), by, boff, vns, ref, ("extreme", 100, adaptive))
    if not adaptive:
        sweep(plan_of(100, 0), by2, boff2, None, ref_of("uniform", 100, 0), ("uniform", 100, 0))


@pytest.mark.parametrize("q,adaptive", PLANS)
def test_foreign_bytes(T, dm, q, adaptive):
    """Seeded random payload behind valid non-decreasing offsets (lengths 0..400: empty blocks and
    blocks above the format's 368 B both occur), and a stream of nothing but empty blocks."""
    rng = np.random.default_rng(23 + q + adaptive)
    n = sum(NBS)
    lengths = rng.integers(0, 401, n)
    lengths[rng.integers(0, n, 60)] = 0
    assert (lengths > 368).any() and (lengths == 0).any()
    vns = var_nums() if adaptive else None
    plan = plan_of(q, adaptive)
    for lens in (lengths, np.zeros(n, np.int64)):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        by = T.from_numpy(rng.integers(0, 256, max(int(off[-1]), 4), dtype=np.uint8)).cuda()
        boff = T.from_numpy(off.view(np.int32)).cuda()
        ref = Ref(dm, by, boff, q, adaptive, vns)
        if lens.any():
            assert any(int(p.min()) != int(p.max()) for p in ref(2, ALL))
        else:
            assert not ref.coef.any() and all((p == 128).all() for p in ref(8, ALL))
        sweep(plan, by, boff, vns, ref, ("foreign", q, adaptive, bool(lens.any())))


# ---- 2. only the window is read ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,q,adaptive", [("uniform", 50, 1), ("extreme", 100, 0)])
def test_only_the_window_is_read(T, dm, kind, q, adaptive):
    """Every payload byte outside the window's runs (window_ref.outside) is overwritten from a second
    seed, offsets unchanged: the result is what it was."""
    by, boff, vns = stream_of(kind, q, adaptive)
    ref = ref_of(kind, q, adaptive)
    plan = plan_of(q, adaptive)
    off = u32(boff).astype(np.int64)
    host = by.cpu().numpy()
    noise = np.random.default_rng(77).integers(0, 256, host.size, dtype=np.uint8)
    for name, windows in WINDOWS.items():
        if name == "whole":
            continue
        keep = np.ones(host.size, dtype=bool)
        for b in window_ref.outside(SHAPES, windows):
            keep[off[b]:off[b + 1]] = False
        inside = np.concatenate([b.ravel() for b in window_ref.blocks(SHAPES, windows)])
        assert all(keep[off[b]:off[b + 1]].all() for b in inside) and not keep.all()
        poisoned = T.from_numpy(np.where(keep, host, noise)).cuda()
        for scale in SCALES:
            got = plan.decode_bits_scaled(poisoned, boff, SHAPES, scale, windows, var_nums=vns)
            assert_equal(got, ref(scale, windows), (kind, q, name, scale, "poisoned outside"))


# ---- 3. destinations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", ["whole", "33 wide", "origin"])
def test_strided_outs_at_the_minimum_alignment(T, dm, name, scale):
    """Every destination starts n bytes into its buffer and has row and frame strides that are odd
    multiples of n: the minimum alignment, n = 8 / scale.  Every byte that is no pixel keeps its
    sentinel."""
    by, boff, vns = stream_of("uniform", 50, 1)
    windows = WINDOWS[name]
    n = 8 // scale
    bufs, outs, owns = [], [], []
    for (f0, f1), (y0, y1), (x0, x1) in windows:
        f, h, w = f1 - f0, (y1 - y0) // scale, (x1 - x0) // scale
        st = w + (n if (w // n) % 2 == 0 else 2 * n)
        fs = st * h + (n if (st * h // n) % 2 == 0 else 2 * n)
        assert (st // n) % 2 == 1 and (fs // n) % 2 == 1
        b = T.full((n + fs * f + 64,), SENTINEL, dtype=T.uint8, device="cuda")
        assert b.data_ptr() % 16 == 0
        o = b.as_strided((f, h, w), (fs, st, 1), n)
        own = T.zeros_like(b, dtype=T.bool)
        own.as_strided((f, h, w), (fs, st, 1), n).fill_(True)
        bufs.append(b), outs.append(o), owns.append(own)
    got = plan_of(50, 1).decode_bits_scaled(by, boff, SHAPES, scale, windows, outs=outs, var_nums=vns)
    assert all(g is o for g, o in zip(got, outs))
    assert_equal(got, ref_of("uniform", 50, 1)(scale, windows), (name, scale, "strided"))
    for b, own in zip(bufs, owns):
        assert bool((b[~own] == SENTINEL).all()), (name, scale, "a byte outside width x height was written")


def test_side_stream(T, dm):
    by, boff, vns = stream_of("uniform", 50, 1)
    windows = WINDOWS["origin"]
    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    T.cuda.synchronize()
    got = plan_of(50, 1).decode_bits_scaled(by, boff, SHAPES, 4, windows, var_nums=vns, stream=s)
    s.synchronize()
    dm.stream_release(s)
    assert_equal(got, ref_of("uniform", 50, 1)(4, windows), "side stream")


# ---- 4. the persistent loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("q,adaptive", [(100, 0), (50, 1)])
def test_grid_limit(T, dm, q, adaptive):
    """One workgroup: 64 runs over 4 waves, so every wave's loop runs 16 times."""
    kind = "extreme" if q == 100 else "uniform"
    by, boff, vns = stream_of(kind, q, adaptive)
    ref = ref_of(kind, q, adaptive)
    for scale in SCALES:
        for name in ("whole", "origin"):
            T.cuda.synchronize()
            with dm.grid_limit(1):
                got = dm.Plan(q, adaptive).decode_bits_scaled(by, boff, SHAPES, scale, WINDOWS[name], var_nums=vns)
                grid = dm.last_grid()
            T.cuda.synchronize()
            assert grid == 1, (name, grid, "the limit did not reach the launch")
            assert_equal(got, ref(scale, WINDOWS[name]), (name, scale, "limit 1"))


# ---- 5. refusals ------------------------------------------------------------------------------------------------
def test_refusals(T, dm):
    by, boff, vns = stream_of("uniform", 50, 1)
    plan, aplan = plan_of(50, 0), plan_of(50, 1)
    for scale in (1, 3, 16, None):
        with pytest.raises(dm.DctqError, match="scale must be 2, 4 or 8"):
            plan.decode_bits_scaled(by, boff, SHAPES, scale)
    with pytest.raises(dm.DctqError, match="adaptive decode needs var_nums"):
        aplan.decode_bits_scaled(by, boff, SHAPES, 2)
    with pytest.raises(dm.DctqError, match="windows needs one entry per plane"):
        plan.decode_bits_scaled(by, boff, SHAPES, 2, ALL[:3])
    with pytest.raises(dm.DctqError, match="offsets must be a contiguous int32 device tensor"):
        plan.decode_bits_scaled(by, boff[:-1], SHAPES, 2)
    outs = [T.full((f, h // 4, w // 4), SENTINEL, dtype=T.uint8, device="cuda") for f, h, w in SHAPES]
    with pytest.raises(dm.DctqError, match=r"outs\[0\] is .* shapes\[0\] says"):
        plan.decode_bits_scaled(by, boff, SHAPES, 2, outs=outs)
    # the library itself: a missing var_num on an adaptive plan is refused before any launch
    import ctypes as C
    descs = (dm._Plane * 4)(*[dm.plane_desc(o) for o in outs])
    wins = (dm._Window * 4)(*[dm._Window(w, h, f, 0, 0, 0) for f, h, w in SHAPES])
    ptrs = (C.c_void_p * 4)(vns[0].data_ptr(), None, vns[2].data_ptr(), vns[3].data_ptr())
    for vp in (None, C.cast(ptrs, C.c_void_p)):
        rc = dm.lib().dctq_decode_bits_window_scaled_planes(aplan._h, C.c_void_p(by.data_ptr()),
                                                            C.c_void_p(boff.data_ptr()), vp, wins, descs, 4, 2, None)
        assert rc == -1, rc
    T.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)


# ---- 6. decompress(scale=) ----------------------------------------------------------------------------------------
def rgb_picture(T, dm, f, h, w, kind="uniform"):
    p = dm.synth(4242, kind, -(-3 * w // 4) * 4, h, f)   # synth takes widths that are multiples of 4
    return p[:, :, :3 * w].reshape(f, h, w, 3).contiguous()


def container_ref(dm, buf, scale):
    """scaled_ref over the container's own coefficients: the whole stored planes, reduced."""
    d = dm.frame_unpack(buf)
    coef = dm.bits_decode(d["bytes"], d["offsets"]).cpu().numpy()
    vns = None if d["var_nums"] is None else [v.cpu().numpy() for v in d["var_nums"]]
    return scaled_ref.planes(coef, d["shapes"], table(d["quality"], d["adaptive"]), scale, d["adaptive"], vns)


@pytest.mark.parametrize("adaptive", [False, True])
def test_decompress_scaled_colour(T, dm, adaptive):
    """A 4:2:0 picture 70 x 50 x 2 frames (frame c1: stored 80 x 64 luma, 40 x 32 chroma): the result is
    color_ref.inverse_cropped of the scaled_ref planes, at ceil(50 / s) x ceil(70 / s)."""
    f, h, w = 2, 50, 70
    buf = dm.compress(rgb_picture(T, dm, f, h, w), 50, adaptive=adaptive)
    assert dm.frame_unpack(buf)["crops"] == [(14, 10), (0, 0), (0, 0)]
    for scale in SCALES:
        y, cb, cr = container_ref(dm, buf, scale)
        assert cb.shape[1:] == (y.shape[1] // 2, y.shape[2] // 2)         # exactly half the reduced luma
        rh, rw = -(-h // scale), -(-w // scale)
        want = color_ref.inverse_cropped(y, cb, cr, rh, rw)
        got = dm.decompress(buf, scale=scale)
        assert tuple(got.shape) == (f, rh, rw, 3) and np.array_equal(got.cpu().numpy(), want), scale
        if adaptive:
            assert int(want.max()) - int(want.min()) > 64
        one = dm.decompress(buf, scale=scale, frames=(1, 2))
        assert T.equal(one, got[1:2]), scale
        bgrx = dm.decompress(buf, scale=scale, channels=4, bgr=True).cpu().numpy()
        assert np.array_equal(bgrx[..., 2::-1], want) and (bgrx[..., 3] == 255).all()
    with pytest.raises(dm.DctqError, match="scale together with region is not supported"):
        dm.decompress(buf, scale=2, region=((0, 8), (0, 8)))
    with pytest.raises(dm.DctqError, match="scale must be 2, 4 or 8"):
        dm.decompress(buf, scale=5)
    with pytest.raises(dm.DctqError):
        dm.decompress(buf, scale=2, frames=(1, 3))


@pytest.mark.parametrize("adaptive", [False, True])
def test_decompress_scaled_plain_planes(T, dm, adaptive):
    """Plain planes, frame c1 (203 x 45 and 100 x 27, true sizes) and frame v1 (64 x 16)."""
    planes = [dm.synth(7, "uniform", 204, 45, 3)[:, :, :203], dm.synth(8, "smooth", 100, 27, 3)]
    for src in (planes, [dm.synth(9, "uniform", 64, 16, 3)]):
        buf = dm.compress(src, 50, adaptive=adaptive)
        for scale in SCALES:
            want = container_ref(dm, buf, scale)
            got = dm.decompress(buf, scale=scale)
            assert len(got) == len(src)
            for g, wnt, p in zip(got, want, src):
                rh, rw = -(-p.shape[1] // scale), -(-p.shape[2] // scale)
                assert tuple(g.shape) == (3, rh, rw)
                assert np.array_equal(g.cpu().numpy(), wnt[:, :rh, :rw]), scale
            one = dm.decompress(buf, scale=scale, frames=(1, 2))
            assert all(T.equal(o, g[1:2]) for o, g in zip(one, got)), scale


# ---- 7. the C host ------------------------------------------------------------------------------------------------
def test_frame_scaled_host(T, dm):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_scaled"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for (w, h, q, ad, kind) in [(640, 480, 50, 1, 0), (64, 48, 50, 0, 1), (96, 80, 100, 0, 3)]:
        for log2s in (1, 2, 3):
            r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(ROOT, "host", "frame_scaled"), str(w), str(h),
                                str(q), str(ad), "12345", str(kind), str(log2s)], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
            assert r.stdout.split() == ["scaled_equal=1", "padding_intact=1", "abi_version=6"], r.stdout
