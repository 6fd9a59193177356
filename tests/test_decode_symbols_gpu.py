"""GPU: the fused symbol decoder (dctq_decode_symbols_planes / Plan.decode_symbols):
run-length symbols -> clamped u8 pixels in one launch, no coefficient buffer.

The contract is an equivalence: bit for bit dctq_rle_decode(16) followed by
dctq_decode_planes.  Against the oracle the bound is test_decode_gpu.py's: a pixel is
rne(clamp(r, 0, 255)) of an fp32 recon r with |r - reference| <= 1e-4, clamping does not
increase a distance and rounding moves a value by at most 0.5, so
|pix - clip(reference, 0, 255)| <= 0.5 + 1e-4."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = [(50, 0), (50, 1), (10, 1), (90, 1), (100, 0), (100, 1), (1, 1), (75, 0)]
KIND_NAMES = ["uniform", "smooth", "const", "extreme"]
W, H, SEED = 64, 48, 21  # 48 blocks: one full 32-block half and a 16-block half
TOL = 0.5 + 1e-4
SENTINEL = 0xA5
LANE_MAX, WALK_MAX = 240, 1024  # rle_decode_core.h kDecLaneMax / kDecWalkMax: symbols per half tile


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
    """[f*h/8*w/8, 64] block-major (raster order of blocks) -> [f, h, w]."""
    return blocks.reshape(f, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(f, h, w)


@functools.lru_cache(maxsize=None)
def oracle_pixels(kind):
    import oracle as O
    px = O.synth_plane(SEED, O.KINDS[kind], W, H)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def oracle_case(kind, q, ad):
    """(coefficients, var_num int32, reference recon + 128 as an image [H, W]) from the oracle."""
    import oracle as O
    px = oracle_pixels(kind)
    coef = O.forward_plane(px, q, ad)
    var = O.plane_variance(px)
    vn = var * 4096.0
    assert np.array_equal(vn, np.round(vn))
    want = untile(O.inverse_plane(coef, q, ad, var if ad else None) + 128.0, 1, H, W)[0]
    out = (coef, vn.astype(np.int32), want)
    for a in out:
        a.setflags(write=False)
    return out


def gpu(T, a):
    return T.from_numpy(np.array(a)).cuda()  # a copy: the cached oracle arrays are read-only


def widths_of(plan):
    return [4, 2] if plan.symbol_bytes == 2 else [4]


def split_planes(coef, nbs):
    """One [N, 64] coefficient tensor -> its per-plane slices {c + 64 * first_k}."""
    out, first = [], 0
    for nb in nbs:
        out.append(coef[first:first + nb])
        first += nb
    return out


def two_step(dm, plan, sym, off, shapes, vns):
    nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
    return plan.decode_planes(split_planes(dm.rle_decode(sym, off), nbs), shapes=shapes, var_nums=vns)


def half_counts(off):
    """Symbols per 32-block half of every 64-block tile, from the offsets."""
    o = off.cpu().numpy().view(np.uint32).astype(np.int64)
    n = o.size - 1
    edges = sorted(set(list(range(0, n, 32)) + [n]))
    return [int(o[b] - o[a]) for a, b in zip(edges[:-1], edges[1:])]


def encode_case(T, dm, plan, kind, ad, sb):
    """GPU-encoded symbols of the oracle's pixels, and var_num (side information of adaptive plans)."""
    gp = gpu(T, oracle_pixels(kind))
    vn = T.zeros(gp.numel() // 64, dtype=T.int32, device="cuda")
    plan.forward_quant(gp, var_num=vn)
    _, off, sym = plan.encode_planes([gp], symbol_bytes=sb)
    return off, sym, [vn] if ad else None


# ---- 1. equals the two-step path ---------------------------------------------------
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("q,ad", PLANS)
def test_equals_two_step(T, dm, q, ad, kind):
    plan = dm.Plan(q, ad)
    for sb in widths_of(plan):
        off, sym, vns = encode_case(T, dm, plan, kind, ad, sb)
        assert sym.dtype == (T.int16 if sb == 2 else T.int32)
        got = plan.decode_symbols(sym, off, shapes=[(H, W)], var_nums=vns)[0]
        want = two_step(dm, plan, sym, off, [(1, H, W)], vns)[0]
        assert got.dtype == T.uint8 and tuple(got.shape) == (1, H, W)
        assert T.equal(got, want), (kind, q, ad, sb, int((got != want).sum()))


# ---- 2. the three density paths ------------------------------------------------------
DENSITY = [("smooth", 50), ("uniform", 10), ("uniform", 50), ("uniform", 100)]


def test_density_paths(T, dm):
    seen = []
    for kind, q in DENSITY:
        plan = dm.Plan(q, 0)
        for sb in widths_of(plan):
            off, sym, _ = encode_case(T, dm, plan, kind, 0, sb)
            counts = half_counts(off)
            print(f"{kind} q{q} {sb}-byte: symbols per half {counts}")
            seen += counts
            got = plan.decode_symbols(sym, off, shapes=[(H, W)])[0]
            assert T.equal(got, two_step(dm, plan, sym, off, [(1, H, W)], None)[0]), (kind, q, sb)
    assert any(c <= LANE_MAX for c in seen), seen
    assert any(LANE_MAX < c <= WALK_MAX for c in seen), seen
    assert any(c > WALK_MAX for c in seen), seen


# ---- 3. symbols built on the CPU, checked against the oracle --------------------------
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("q,ad", [(50, 0), (75, 0), (90, 1)])  # fp32-admitted, fp64 non-adaptive, adaptive
def test_cpu_symbols_against_oracle(T, dm, q, ad, kind):
    import oracle as O
    coef, vn, want = oracle_case(kind, q, ad)
    off, sym = O.rle_encode_plane(coef)
    plan = dm.Plan(q, ad)
    vns = [gpu(T, vn)] if ad else None
    goff = gpu(T, off.view(np.int32))
    for sb in widths_of(plan):
        s = gpu(T, sym.view(np.int32)) if sb == 4 else gpu(T, O.pack16(sym).view(np.int16))
        pix = plan.decode_symbols(s, goff, shapes=[(H, W)], var_nums=vns)[0].cpu().numpy()[0]
        err = np.abs(pix.astype(np.float64) - np.clip(want, 0.0, 255.0)).max()
        print(f"{kind} q{q} a{ad} {sb}-byte: max |pix - clip(reference)| = {err:.6f}")
        assert err <= TOL, (kind, q, ad, sb, err)


# ---- 4. geometry and untouched bytes -----------------------------------------------------
GEOMETRY = [  # shapes (F, H, W) of the planes of one call, row padding, extra rows between frames
    # 48 + 12 + 12 + 30 = 102 blocks: the second half of tile 0 spans three planes, tile 1 starts mid-plane
    ([(1, 48, 64), (1, 24, 32), (1, 24, 32), (3, 16, 40)], 8, 3),
    ([(1, 8, 8)], 0, 0),        # one block
    ([(1, 8, 264)], 8, 0),      # 33 blocks
    ([(3, 56, 136)], 16, 5),    # 357 blocks: halves straddle frames; frame_stride beyond one frame
]


@pytest.mark.parametrize("q,ad", [(50, 0), (75, 0), (90, 1)])
@pytest.mark.parametrize("shapes,pad,gap", GEOMETRY)
def test_geometry_and_untouched_bytes(T, dm, shapes, pad, gap, q, ad):
    plan = dm.Plan(q, ad)
    planes = [dm.synth(900 + k, KIND_NAMES[k], s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    vns = [T.zeros(s[0] * (s[1] // 8) * (s[2] // 8), dtype=T.int32, device="cuda") for s in shapes]
    plan.forward_quant_planes(planes, var_nums=vns)
    for sb in widths_of(plan):
        coefs, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
        assert off.numel() == sum(v.numel() for v in vns) + 1
        bufs = [T.full((s[0], s[1] + gap, s[2] + pad), SENTINEL, dtype=T.uint8, device="cuda") for s in shapes]
        views = [b[:, :s[1], :s[2]] for b, s in zip(bufs, shapes)]
        outs = plan.decode_symbols(sym, off, outs=views, var_nums=vns if ad else None)
        for k, s in enumerate(shapes):
            assert outs[k].data_ptr() == bufs[k].data_ptr()
            expect = plan.decode(coefs[k], s, var_num=vns[k] if ad else None)
            assert T.equal(views[k], expect), (k, s, sb, int((views[k] != expect).sum()))
            outside = bufs[k].clone()
            outside[:, :s[1], :s[2]] = SENTINEL
            assert bool((outside == SENTINEL).all()), ("bytes outside width x height were written", k, s, sb)
        # the same into contiguous tensors the call allocates
        again = plan.decode_symbols(sym, off, shapes=shapes, var_nums=vns if ad else None)
        assert all(T.equal(a, v) for a, v in zip(again, views))


# ---- 5. runs that walk past the end of a block ------------------------------------------------
@pytest.mark.parametrize("q,ad", [(50, 0), (75, 0)])
def test_runs_past_the_block_end(T, dm, q, ad):
    """run_length_decode's rule: pos += run; a value lands only while pos < 64; pos++."""
    blocks = [  # (value, run) per symbol
        [(5, 0), (7, 70)],                  # the second symbol lands at 71: dropped
        [(0, 64)],                          # the all-zero block
        [(3, 60), (4, 2), (9, 0)],          # 60, 63, then 64: dropped
        [(1, 63)],                          # exactly the last position
        [(2, 10), (-3, 100), (6, 0)],       # 10, then 111 and 112: dropped
        [(100, 0), (-50, 0), (0, 62)],      # the closing zero at 64: dropped
    ]
    sym = np.array([(v & 0xFFFF) | (r << 16) for b in blocks for v, r in b], np.uint32)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    assert off[-1] == sym.size and (np.diff(off.astype(np.int64)) > 0).all()
    gs, go = gpu(T, sym.view(np.int32)), gpu(T, off.view(np.int32))
    shape = (1, 8, 8 * len(blocks))
    coef = dm.rle_decode(gs, go).cpu().numpy()
    assert coef[0].tolist().count(0) == 63 and coef[0, 0] == 5  # the dropped value is nowhere
    assert not coef[1].any() and coef[3, 63] == 1 and coef[2, 63] == 4
    plan = dm.Plan(q, ad)
    got = plan.decode_symbols(gs, go, shapes=[shape])[0]
    assert T.equal(got, two_step(dm, plan, gs, go, [shape], None)[0])


# ---- 6. side stream --------------------------------------------------------------------------
def test_side_stream(T, dm):
    plan = dm.Plan(90, 1)
    off, sym, vns = encode_case(T, dm, plan, "uniform", 1, 2)
    want = two_step(dm, plan, sym, off, [(1, H, W)], vns)[0]
    T.cuda.synchronize()
    stream = T.cuda.Stream()
    with T.cuda.stream(stream):
        got = plan.decode_symbols(sym, off, shapes=[(H, W)], var_nums=vns, stream=stream)[0]
    stream.synchronize()
    assert T.equal(got, want)
    dm.stream_release(stream)


# ---- 7. invalid arguments ------------------------------------------------------------------------
def test_invalid_arguments(T, dm):
    L = dm.lib()
    EINVAL = -1
    plans = {0: dm.Plan(50, 0), 1: dm.Plan(50, 1)}
    w, h = 32, 16
    nblk = (w // 8) * (h // 8)
    buf = T.full((h * w + 64,), SENTINEL, dtype=T.uint8, device="cuda")
    sym = T.full((nblk + 2,), 64 << 16, dtype=T.int32, device="cuda")  # every block: (0, 64)
    off = T.arange(nblk + 1, dtype=T.int32, device="cuda")
    vn = T.zeros(nblk, dtype=T.int32, device="cuda")
    assert buf.data_ptr() % 8 == 0 and sym.data_ptr() % 4 == 0

    def call(ad=0, plan="ok", symbols="ok", sb=4, offsets="ok", vns="ok", dst="ok", nplanes=1, **geo):
        g = dict(pixels=buf.data_ptr(), stride=w, frame_stride=w * h, width=w, height=h, nframes=1, vn=vn.data_ptr())
        g.update(geo)
        n = max(nplanes, 1)
        descs = (dm._Plane * n)(*[dm._Plane(g["pixels"], g["stride"], g["frame_stride"], g["width"], g["height"],
                                            g["nframes"]) for _ in range(n)])
        vp = (C.c_void_p * n)(*[g["vn"]] * n)
        return L.dctq_decode_symbols_planes(plans[ad]._h if plan == "ok" else None,
                                            C.c_void_p(sym.data_ptr()) if symbols == "ok" else symbols, sb,
                                            C.c_void_p(off.data_ptr()) if offsets == "ok" else None,
                                            C.cast(vp, C.c_void_p) if vns == "ok" else None,
                                            descs if dst == "ok" else None, nplanes, None)

    bad = {
        "NULL plan": dict(plan=None),
        "NULL symbols": dict(symbols=None),
        "NULL offsets": dict(offsets=None),
        "NULL dst": dict(dst=None),
        "NULL dst[k].pixels": dict(pixels=None),
        "nplanes 0": dict(nplanes=0),
        "nplanes 5": dict(nplanes=5),
        "symbol_bytes 3": dict(sb=3),
        "symbol_bytes 0": dict(sb=0),
        "2-byte stream at an odd 2-byte address": dict(sb=2, symbols=C.c_void_p(sym.data_ptr() + 2)),
        "adaptive without var_num": dict(ad=1, vns=None),
        "adaptive with a NULL var_num[k]": dict(ad=1, vn=None),
        "width 12": dict(width=12),
        "height 12": dict(height=12),
        "stride < width": dict(stride=w - 8),
        # geometry only (nothing is launched): 2^26 blocks, in one plane and over four
        "2^26 blocks": dict(width=8 * 8192, stride=8 * 8192, height=8 * 8192),
        "2^26 blocks over four planes": dict(width=8 * 4096, stride=8 * 4096, height=8 * 4096, nplanes=4),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        assert L.dctq_error_string(EINVAL), what
    T.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call wrote pixels"
    # non-adaptive plans ignore var_num: NULL, or entries that are NULL; a 2-byte stream under a 4-byte plan is fine
    assert call(vns=None) == 0 and call(vn=None) == 0
    T.cuda.synchronize()
    assert bool((buf[w * h:] == SENTINEL).all())
    p100 = dm.Plan(100, 0)
    assert p100.symbol_bytes == 4
    zero16 = T.zeros(nblk, dtype=T.int16, device="cuda")  # every block: 0x0000 = (0, 64)
    a = p100.decode_symbols(zero16, off, shapes=[(h, w)])[0]
    assert T.equal(a, p100.decode_symbols(sym[:nblk], off, shapes=[(h, w)])[0])
    # the Python layer refuses mistyped or mis-sized tensors before the library sees them
    p = plans[0]
    for bad_call in (lambda: p.decode_symbols(sym, off[:-1], shapes=[(h, w)]),
                     lambda: p.decode_symbols(sym, off.to(T.int64), shapes=[(h, w)]),
                     lambda: p.decode_symbols(sym, off.cpu(), shapes=[(h, w)]),
                     lambda: p.decode_symbols(sym.to(T.int64), off, shapes=[(h, w)]),
                     lambda: p.decode_symbols(sym, off),
                     lambda: plans[1].decode_symbols(sym, off, shapes=[(h, w)])):
        with pytest.raises(dm.DctqError):
            bad_call()


# ---- 8. C host ---------------------------------------------------------------------------------------
def test_symbols_decode_host(T, dm):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "symbols_decode"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for (w, h, q, ad, kind, streams) in [(640, 480, 90, 1, 1, 2), (64, 48, 50, 0, 0, 2), (96, 80, 100, 0, 0, 1)]:
        r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(ROOT, "host", "symbols_decode"), str(w), str(h),
                            str(q), str(ad), "12345", str(kind)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        got = dict(l.split(":", 1) for l in r.stdout.strip().splitlines())
        assert got["fused_equal"] == "1" and got["padding_intact"] == "1" and got["abi_version"] == "6", got
        assert int(got["streams"]) == streams, got
