"""GPU: every persistent kernel's grid-stride loop, run more than once per wave.

Every hot kernel is a persistent grid-stride loop whose grid is min(batches / 4 waves,
CUs x resident workgroups x 8..1024): on 256 CUs a wave sees ONE tile up to about 16 M
blocks, so no test-sized input ever reaches a wave's second iteration -- the registers
prefetched for the next batch, the store drain in front of the next LDS read, the LDS stage
and half tile the next tile zeroes and overwrites, a lane's running maximum.  Here
dct_amd.grid_limit (dctq_diag_set_grid_limit) caps every such grid at 1 and at 3 workgroups
(4 and 12 waves) on one picture set of 1 248 blocks, 4:2:0 planes (4, 96, 136) + 2 x (4, 48,
72): 20 tiles of 64 over the concatenation, plane changes inside tiles, a partial last tile.

For every entry point:
  (a) the limited run equals the unlimited run bit for bit in every output, guard bytes
      after the last element and sentinel bytes around strided destinations included;
  (b) the unlimited run, at this same shape, is held once to the CPU yardstick the suite
      already uses for that operation (oracle, tools/bits_ref.py, tools/frame_ref.py,
      tools/color_ref.py, the tolerances of the tests named at each use), so that (a) is not
      two wrong answers agreeing.
Every case first asserts, from the kernel's own batch size, that each wave (each lane, for
the lane-per-item kernels) gets at least 3 iterations at limit 1, and after each limited
call that dctq_diag_last_grid() is the limit: a hook that silently did nothing fails here.
A wrapper that launches several kernels is asserted on its LAST persistent launch; the
earlier ones have their own cases.  One case per family also runs on a side stream."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bits_ref  # noqa: E402
import frame_ref  # noqa: E402
import inv_bound as IB  # noqa: E402
# helpers and yardsticks of the existing tests, used as they stand
import test_color_gpu as TC  # noqa: E402
import test_decode_foreign_gpu as TF  # noqa: E402
import test_distortion_gpu as TD  # noqa: E402
import test_frame_gpu as TFR  # noqa: E402

LIMITS = [1, 3]
WAVES = 4                      # every persistent kernel's workgroup is 4 waves (256 threads)
SHAPES = [(4, 96, 136), (4, 48, 72), (4, 48, 72)]     # 816 + 216 + 216 blocks
SHAPES444 = [(4, 96, 136)] * 3                        # the per-plane emit needs 12 tiles in EVERY plane
PAD, GAP = 8, 3                # bytes after every row, rows after every frame
SENTINEL = 0xA5
GUARD = 64                     # sentinel bytes after the last element of a flat output
TOL_PIXEL = 0.5 + 1e-4         # tests/test_decode_gpu.py
DEC_STAGE = 2560               # bits_core.h kBitsStage (per half tile), as tests/test_bits_gpu.py
MIX = ["smooth", "uniform", "extreme"]
RGB_SHAPE = (4, 96, 144)       # the colour cases: 4:2:0 of it is (4, 96, 144) + 2 x (4, 48, 72), 1 296 blocks


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


# ---- the picture set and its references (computed once, read-only) --------------------------------
def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def nblocks(shapes):
    return [f * (h // 8) * (w // 8) for f, h, w in shapes]


def batches(nbs, per):
    """Batches of `per` blocks when every plane starts a batch of its own."""
    return sum(-(-n // per) for n in nbs)


@functools.lru_cache(maxsize=None)
def host_planes(variant):
    """u8 [F, H, W] per plane.  "mixed": the kind changes from frame to frame and from plane to
    plane, so consecutive tiles of one wave differ in density; "dense": extremes only (with
    q100 every half tile's bytes exceed the decoders' stage).  "...444": full-size chroma."""
    import oracle as O
    out = []
    for k, (f, h, w) in enumerate(SHAPES444 if variant.endswith("444") else SHAPES):
        kinds = ["extreme"] * f if variant.startswith("dense") else [MIX[(k + i) % 3] for i in range(f)]
        out.append(np.stack([O.synth_plane(100 + 10 * k + i, O.KINDS[kinds[i]], w, h) for i in range(f)]))
    return frozen(*out)


@functools.lru_cache(maxsize=None)
def host_rgb(variant, f=RGB_SHAPE[0]):
    """u8 [f, H, W, 3] of RGB_SHAPE's frames: every channel a plane of its own, kinds as host_planes."""
    import oracle as O
    _, h, w = RGB_SHAPE
    chans = []
    for c in range(3):
        kinds = ["extreme"] * f if variant == "dense" else [MIX[(c + i) % 3] for i in range(f)]
        chans.append(np.stack([O.synth_plane(300 + 10 * c + i, O.KINDS[kinds[i]], w, h) for i in range(f)]))
    return frozen(np.stack(chans, axis=-1))[0]


@functools.lru_cache(maxsize=None)
def oracle_case(variant, q, ad):
    """Per plane: (coef int16 [nb, 64], var_num int32 [nb], float coefficients [nb, 64],
    reference recon + 128 [nb, 64]), frames concatenated, all from the oracle."""
    import oracle as O
    out = []
    for p in host_planes(variant):
        cf = [O.forward_plane(fr, q, ad, want_float=True) for fr in p]
        coef = np.concatenate([c for c, _ in cf])
        var = np.concatenate([O.plane_variance(fr) for fr in p])
        vn = var * 4096.0
        assert np.array_equal(vn, np.round(vn))
        want = O.inverse_plane(coef, q, ad, var if ad else None) + 128.0
        out.append(frozen(coef, vn.astype(np.int32), np.concatenate([f for _, f in cf]), want))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def streams(variant, q, ad):
    """The coefficients' streams from the CPU coders: (offsets u32, 4-byte symbols u32, 2-byte
    symbols u16 or None, packed bytes u8, byte offsets u32)."""
    import oracle as O
    coef = np.concatenate([c for c, _, _, _ in oracle_case(variant, q, ad)])
    off, sym = O.rle_encode_plane(coef)
    sym16 = O.pack16(sym) if np.abs(coef.astype(np.int32)).max() <= 511 else None
    by, boff = bits_ref.pack(bits_ref.blocks_of(sym, off))
    return frozen(off, sym, sym16, by, boff)


def untile(blocks, f, h, w):
    return blocks.reshape(f, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(f, h, w)


# ---- device buffers -------------------------------------------------------------------------------------
def gpu(T, a):
    return T.from_numpy(np.array(a)).cuda()  # a copy: the cached arrays are read-only


def padded(T, shapes, content=None):
    """[(buf, view)]: sentinel-filled u8 buffers with padded rows and gap rows between frames,
    and the [F, H, W] views into them (holding content[k] when given)."""
    out = []
    for k, (f, h, w) in enumerate(shapes):
        buf = T.full((f, h + GAP, w + PAD), SENTINEL, dtype=T.uint8, device="cuda")
        view = buf[:, :h, :w]
        if content is not None:
            view.copy_(gpu(T, content[k]))
        out.append((buf, view))
    return out


def untouched_outside(T, buf, view):
    b = buf.clone()
    b[:, :view.shape[1], :view.shape[2]] = SENTINEL
    return bool((b == SENTINEL).all())


def guarded(T, n, dtype):
    """A flat tensor of n elements of dtype followed by GUARD sentinel bytes (every byte 0xA5)."""
    size = T.empty(0, dtype=dtype).element_size()
    return T.full((n * size + GUARD,), SENTINEL, dtype=T.uint8, device="cuda").view(dtype)


def guard_intact(T, t, n):
    raw = t.view(T.uint8)
    return bool((raw[n * t.element_size():] == SENTINEL).all())


def bit_equal(T, a, b):
    """Bit for bit (floats too: -0.0 is not 0.0 here), whole buffers, guards and padding included."""
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and T.equal(a.view(T.uint8), b.view(T.uint8))


def ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- the harness ------------------------------------------------------------------------------------------
def grid_for(nbatch):
    return -(-nbatch // WAVES)


def run_limited(T, dm, what, nbatch, call, want, side=False):
    """call(stream) -> list of device tensors (whole buffers).  nbatch: the batches of the call's
    last persistent launch, the one whose grid is read back -- every wave must get 3 iterations
    at limit 1.  want: the unlimited run's tensors."""
    assert nbatch // WAVES >= 3, (what, nbatch, "fewer than 3 iterations per wave at limit 1: enlarge the case")
    runs = [(limit, None) for limit in LIMITS] + ([(1, T.cuda.Stream())] if side else [])
    for limit, stream in runs:
        T.cuda.synchronize()
        with dm.grid_limit(limit):
            if stream is None:
                got = call(None)
            else:
                with T.cuda.stream(stream):
                    got = call(stream)
                stream.synchronize()
                dm.stream_release(stream)
            grid = dm.last_grid()
        T.cuda.synchronize()
        assert grid == limit, (what, limit, grid, "the limit did not reach the launch")
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert bit_equal(T, g, w), (what, f"limit {limit}", "side stream" if stream is not None else "",
                                        f"output {i}", int((g.contiguous().view(T.uint8) != w.contiguous().view(T.uint8)).sum()))
    assert dm.lib() is not dm.diag(), "outside grid_limit the product library serves the wrappers"


def test_the_hook_itself(T, dm):
    """The limit's range, its reset on exit and on an exception, and that the product library
    neither has nor obeys it."""
    D = dm.diag()
    for bad in (-1, 65536, 1 << 20):
        assert D.dctq_diag_set_grid_limit(bad) != 0, bad
    assert D.dctq_diag_last_grid(None) != 0
    with pytest.raises(AttributeError):
        C.CDLL(dm.LIB_PATH).dctq_diag_set_grid_limit
    coef = gpu(T, np.concatenate([c for c, _, _, _ in oracle_case("mixed", 50, 0)]))
    want = dm.huffman_bits(coef)
    with pytest.raises(RuntimeError, match="on purpose"):
        with dm.grid_limit(2):
            assert dm.lib() is dm.diag()
            with pytest.raises(dm.DctqError):
                with dm.grid_limit(1):
                    pass
            got = dm.huffman_bits(coef)
            assert dm.last_grid() == 2
            raise RuntimeError("on purpose")
    assert dm.lib() is not dm.diag()
    assert T.equal(got, want)
    with dm.grid_limit(0):  # 0 = no limit: the same grid as the product's
        dm.huffman_bits(coef)
        assert dm.last_grid() == grid_for(20)
    dm.diag().dctq_huffman_bits(ptr(coef), coef.shape[0], ptr(got), None)  # the diagnostic library, no limit left
    assert dm.last_grid() == grid_for(20)
    T.cuda.synchronize()


# ---- 1. the forward family: pixels in -----------------------------------------------------------------
FORWARD_CASES = [("mixed", 50, 0), ("mixed", 50, 1), ("dense", 100, 0)]


@pytest.mark.parametrize("variant,q,ad", FORWARD_CASES)
def test_forward_round_trip_huffman(T, dm, variant, q, ad):
    import oracle as O
    ref = oracle_case(variant, q, ad)
    nbs = nblocks(SHAPES)
    planes = [v for _, v in padded(T, SHAPES, host_planes(variant))]
    nbatch = batches(nbs, 64)  # every plane starts a 64-block batch of its own: 13 + 4 + 4
    assert nbatch == 21

    def forward(stream):
        outs, vns = [guarded(T, n * 64, T.int16) for n in nbs], [guarded(T, n, T.int32) for n in nbs]
        dm.Plan(q, ad).forward_quant_planes(planes, outs=outs, var_nums=vns, stream=stream)
        return outs + vns

    def forward_plain(stream):  # no var_num: the instantiation the hot path and the benchmark run
        outs = [guarded(T, n * 64, T.int16) for n in nbs]
        dm.Plan(q, ad).forward_quant_planes(planes, outs=outs, stream=stream)
        return outs

    def forward_counted(stream):  # with the fallback counter (and no var_num): the counting instantiation
        outs = [guarded(T, n * 64, T.int16) for n in nbs]
        with dm._on_stream(stream):
            cnt = T.zeros(1, dtype=T.int64, device="cuda")
        plan = dm.Plan(q, ad)
        plan.set_fallback_counter(cnt)
        plan.forward_quant_planes(planes, outs=outs, stream=stream)
        return outs + [cnt]

    def round_trip(stream):
        outs, recs = [guarded(T, n * 64, T.int16) for n in nbs], [guarded(T, n * 64, T.float32) for n in nbs]
        dm.Plan(q, ad).round_trip_planes(planes, outs=outs, recons=recs, stream=stream)
        return outs + recs

    def huffman_planes(stream):
        out = guarded(T, sum(nbs), T.int32)
        dm.Plan(q, ad).huffman_bits_planes(planes, out=out, stream=stream)
        return [out]

    fwd, rt, hp = forward(None), round_trip(None), huffman_planes(None)
    plain, counted = forward_plain(None), forward_counted(None)
    T.cuda.synchronize()
    print(f"{variant} q{q} a{ad}: {int(counted[3].item())} exact-path fallbacks")
    for k, (coef, _, _, _) in enumerate(ref):
        for got in (plain, counted):
            assert guard_intact(T, got[k], nbs[k] * 64)
            assert np.array_equal(got[k][:nbs[k] * 64].cpu().numpy().reshape(-1, 64), coef), (variant, q, ad, k)
    for k, (coef, vn, _, want) in enumerate(ref):
        n = nbs[k]
        assert guard_intact(T, fwd[k], n * 64) and guard_intact(T, fwd[3 + k], n)
        assert guard_intact(T, rt[k], n * 64) and guard_intact(T, rt[3 + k], n * 64)
        assert np.array_equal(fwd[k][:n * 64].cpu().numpy().reshape(n, 64), coef), (variant, q, ad, k)
        assert np.array_equal(fwd[3 + k][:n].cpu().numpy(), vn), (variant, q, ad, k)
        assert np.array_equal(rt[k][:n * 64].cpu().numpy().reshape(n, 64), coef), (variant, q, ad, k)
        err = np.abs(rt[3 + k][:n * 64].cpu().numpy().reshape(n, 64).astype(np.float64) - want).max()
        print(f"{variant} q{q} a{ad} plane {k}: round trip recon max err {err:.3e}")
        assert err <= 1e-4, (variant, q, ad, k, err)
    want_bits = O.huffman_bits_plane(np.concatenate([c for c, _, _, _ in ref]))
    assert guard_intact(T, hp[0], sum(nbs))
    assert np.array_equal(hp[0][:sum(nbs)].cpu().numpy().view(np.uint32), want_bits)
    run_limited(T, dm, "forward_quant_planes", nbatch, forward, fwd, side=(variant == "mixed" and ad == 1))
    run_limited(T, dm, "forward_quant_planes, no var_num", nbatch, forward_plain, plain)
    run_limited(T, dm, "forward_quant_planes, fallback counter", nbatch, forward_counted, counted)
    run_limited(T, dm, "round_trip_planes", nbatch, round_trip, rt)
    run_limited(T, dm, "huffman_bits_planes", nbatch, huffman_planes, hp)

    # huffman_bits over the concatenated coefficients: 20 tiles of 64
    cat = gpu(T, np.concatenate([c for c, _, _, _ in ref]))

    def huffman(stream):
        out = guarded(T, sum(nbs), T.int32)
        dm.huffman_bits(cat, out=out, stream=stream)
        return [out]

    hb = huffman(None)
    assert guard_intact(T, hb[0], sum(nbs))
    assert np.array_equal(hb[0][:sum(nbs)].cpu().numpy().view(np.uint32), want_bits)
    run_limited(T, dm, "huffman_bits", -(-sum(nbs) // 64), huffman, hb)


@pytest.mark.parametrize("variant,q,ad", [("mixed444", 50, 0), ("mixed444", 50, 1), ("dense444", 100, 0)])
def test_encode_planes(T, dm, variant, q, ad):
    """The encoder emits plane by plane, so this case has 13 tiles in EVERY plane (4:4:4): the
    4:2:0 chroma planes' 4 tiles would give the emit kernel one iteration per wave."""
    import oracle as O
    ref = oracle_case(variant, q, ad)
    nbs = nblocks(SHAPES444)
    planes = [v for _, v in padded(T, SHAPES444, host_planes(variant))]
    woff, wsym = O.rle_encode_plane(np.concatenate([c for c, _, _, _ in ref]))
    widths = [4, 2] if dm.Plan(q, ad).symbol_bytes == 2 else [4]
    assert widths == ([4, 2] if q == 50 else [4])
    for sb in widths:
        def encode(stream, sb=sb):
            outs = [guarded(T, n * 64, T.int16) for n in nbs]
            _, off, sym = dm.Plan(q, ad).encode_planes(planes, outs=outs, stream=stream, symbol_bytes=sb)
            return outs + [off, sym]

        def encode_raw(stream, sb=sb):
            """The C entry point with offsets and symbols in guarded buffers of the caller's (worst-case
            capacity: what the stream leaves unused stays sentinel too)."""
            plan, nb = dm.Plan(q, ad), sum(nbs)
            descs = (dm._Plane * 3)(*[dm.plane_desc(p) for p in planes])
            outs = [guarded(T, n * 64, T.int16) for n in nbs]
            off, sym = guarded(T, nb + 1, T.int32), guarded(T, 64 * nb, T.int16 if sb == 2 else T.int32)
            ws = T.empty(int(plan._L.dctq_encode_workspace_bytes(nb)) // 4 + 1, dtype=T.int32, device="cuda")
            cp = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
            fn = plan._L.dctq_encode_planes16 if sb == 2 else plan._L.dctq_encode_planes
            plan._chk(fn(plan._h, descs, 3, C.cast(cp, C.c_void_p), ptr(off), ptr(sym), 64 * nb, ptr(ws),
                         dm._stream_ptr(stream)))
            return outs + [off, sym]

        got, raw = encode(None), encode_raw(None)
        T.cuda.synchronize()
        total = int(woff[-1])
        assert guard_intact(T, raw[3], sum(nbs) + 1) and guard_intact(T, raw[4], total), "written past the stream's end"
        assert T.equal(raw[3][:sum(nbs) + 1], got[3]) and T.equal(raw[4][:total], got[4])
        for k, (coef, _, _, _) in enumerate(ref):
            assert guard_intact(T, got[k], nbs[k] * 64)
            assert np.array_equal(got[k][:nbs[k] * 64].cpu().numpy().reshape(-1, 64), coef), (variant, q, ad, sb, k)
        assert np.array_equal(got[3].cpu().numpy().view(np.uint32), woff), (variant, q, ad, sb, "offsets")
        s = got[4].cpu().numpy()
        assert np.array_equal(s.view(np.uint16) if sb == 2 else s.view(np.uint32), O.pack16(wsym) if sb == 2 else wsym)
        # the count kernel runs over 3 x 13 batches; the last launch is the emit of the last plane, 13 tiles
        assert batches(nbs, 64) // WAVES >= 3
        run_limited(T, dm, f"encode_planes {sb}-byte", -(-nbs[-1] // 64), encode, got, side=(sb == 4 and ad == 0))
        run_limited(T, dm, f"dctq_encode_planes {sb}-byte, guarded", -(-nbs[-1] // 64), encode_raw, raw)


@pytest.mark.parametrize("q,ad", [(50, 0), (50, 1)])
def test_forward_float_and_inverse(T, dm, q, ad):
    """The paired-lane fp64 kernels: 32 blocks per wave and step.  Tolerances: forward_float's 1e-4
    (test_forward_float_tolerance), the inverse's one-rounding bound (test_inverse_is_one_rounding)."""
    import oracle as O
    ref = oracle_case("mixed", q, ad)
    nbs = nblocks(SHAPES)
    y = padded(T, SHAPES[:1], host_planes("mixed")[:1])[0][1]

    def forward_float(stream):
        out = guarded(T, nbs[0] * 64, T.float32)
        dm.Plan(q, ad).forward_float(y, out=out, stream=stream)
        return [out]

    ff = forward_float(None)
    assert guard_intact(T, ff[0], nbs[0] * 64)
    err = np.abs(ff[0][:nbs[0] * 64].cpu().numpy().reshape(-1, 64).astype(np.float64) - ref[0][2]).max()
    print(f"q{q} a{ad}: forward_float max err {err:.3e}")
    assert err <= 1e-4, (q, ad, err)
    run_limited(T, dm, "forward_float", -(-nbs[0] // 32), forward_float, ff)

    coef = np.concatenate([c for c, _, _, _ in ref])
    vn = np.concatenate([v for _, v, _, _ in ref])
    want = np.concatenate([w for _, _, _, w in ref])
    n = coef.shape[0]
    gc, gv = gpu(T, coef), gpu(T, vn)

    def inverse(stream):
        out = guarded(T, n * 64, T.float32)
        dm.Plan(q, ad).inverse(gc, var_num=gv if ad else None, out=out, stream=stream)
        return [out]

    inv = inverse(None)
    assert guard_intact(T, inv[0], n * 64)
    # the tolerance of tests/test_decode_foreign_gpu.py reference(): one fp32 rounding of a value
    # whose fp64 error is 1e-9 scaled with the block's magnitudes
    Q = O.quant_matrix(8, q).ravel()
    if ad:
        nv = np.minimum(1.0, np.maximum(0.1, vn / 4096.0 / 1000.0))
        mult = Q[None, :] * (2.0 - nv)[:, None]
        mult[:, 0] = Q[0]
    else:
        mult = (1.0 / Q)[None, :]
    sx = IB.block_magnitudes(coef, mult).sum(axis=1, keepdims=True)
    tol = TF.U * np.maximum(np.abs(want), 128.0) + 1e-9 * np.maximum(1.0, sx / 1024.0)
    err = np.abs(inv[0][:n * 64].cpu().numpy().reshape(n, 64).astype(np.float64) - want)
    print(f"q{q} a{ad}: inverse max err / tolerance {(err / tol).max():.3f}")
    assert (err <= tol).all(), (q, ad, float((err / tol).max()))
    run_limited(T, dm, "inverse", -(-n // 32), inverse, inv, side=(ad == 1))


# ---- 2. run-length symbols and the packed stream ---------------------------------------------------------
STREAM_CASES = [("mixed", 50, 0), ("dense", 100, 0)]


@pytest.mark.parametrize("variant,q,ad", STREAM_CASES)
def test_rle(T, dm, variant, q, ad):
    coef = np.concatenate([c for c, _, _, _ in oracle_case(variant, q, ad)])
    off, sym, sym16, _, _ = streams(variant, q, ad)
    n = coef.shape[0]
    ntiles = -(-n // 64)
    assert ntiles == 20
    gc = gpu(T, coef)

    def encode(stream):
        o, s = dm.rle_encode(gc, stream=stream)
        return [o, s]

    enc = encode(None)
    assert np.array_equal(enc[0].cpu().numpy().view(np.uint32), off) and np.array_equal(enc[1].cpu().numpy().view(np.uint32), sym)
    run_limited(T, dm, "rle_encode", ntiles, encode, enc, side=(variant == "mixed"))

    # the count alone (rle_encode's last launch is the emit): offsets into a guarded buffer
    def count(stream):
        o = guarded(T, n + 1, T.int32)
        ws = T.empty(int(dm.lib().dctq_rle_workspace_bytes(n)) // 4 + 1, dtype=T.int32, device="cuda")
        s = dm._stream_ptr(stream)
        dm._check(dm.lib().dctq_rle_count(ptr(gc), n, ptr(o), ptr(ws), s))
        return [o]

    cnt = count(None)
    assert guard_intact(T, cnt[0], n + 1) and np.array_equal(cnt[0][:n + 1].cpu().numpy().view(np.uint32), off)
    run_limited(T, dm, "rle_count", ntiles, count, cnt)

    goff = gpu(T, off.view(np.int32))

    # the emit alone, symbols into a guarded buffer
    def emit(stream):
        out = guarded(T, sym.size, T.int32)
        dm._check(dm.lib().dctq_rle_emit(ptr(gc), n, ptr(goff), ptr(out), dm._stream_ptr(stream)))
        return [out]

    em = emit(None)
    assert guard_intact(T, em[0], sym.size) and np.array_equal(em[0][:sym.size].cpu().numpy().view(np.uint32), sym)
    run_limited(T, dm, "rle_emit", ntiles, emit, em)
    assert np.array_equal(TF.rle_decode_cpu(off, sym), coef)
    for name, s in [("rle_decode", sym.view(np.int32))] + ([("rle_decode16", sym16.view(np.int16))] if sym16 is not None else []):
        gs = gpu(T, s)

        def decode(stream, gs=gs):
            out = guarded(T, n * 64, T.int16)
            dm.rle_decode(gs, goff, out=out, stream=stream)
            return [out]

        dec = decode(None)
        assert guard_intact(T, dec[0], n * 64)
        assert np.array_equal(dec[0][:n * 64].cpu().numpy().reshape(n, 64), TF.rle_decode_cpu(off, sym)), name
        run_limited(T, dm, name, ntiles, decode, dec)
    assert sym16 is not None or q != 50, "a q50 plan admits 2-byte symbols"


def later_halves_exceed_stage(boff):
    """Half tiles (32 blocks) of the tiles a wave meets after its first, at limit 1 and at 3."""
    o = boff.astype(np.int64)
    halves = [int(o[min(b + 32, len(o) - 1)] - o[b]) for b in range(0, len(o) - 1, 32)]
    return [h > DEC_STAGE for h in halves[2 * WAVES * max(LIMITS):]]


@pytest.mark.parametrize("variant,q,ad", STREAM_CASES)
def test_bits_pack_and_decode(T, dm, variant, q, ad):
    coef = np.concatenate([c for c, _, _, _ in oracle_case(variant, q, ad)])
    off, sym, sym16, by, boff = streams(variant, q, ad)
    n = coef.shape[0]
    ntiles = -(-n // 64)
    if variant == "dense":
        assert all(later_halves_exceed_stage(boff)), "the chunked path must run in a wave's later iterations"
    goff = gpu(T, off.view(np.int32))
    for sb, s in [(4, sym.view(np.int32))] + ([(2, sym16.view(np.int16))] if sym16 is not None else []):
        gs = gpu(T, s)

        def pack(stream, gs=gs):
            b, o = dm.bits_pack(gs, goff, stream=stream)
            return [b, o]

        got = pack(None)
        assert np.array_equal(got[1].cpu().numpy().view(np.uint32), boff), (variant, sb, "offsets")
        assert np.array_equal(got[0].cpu().numpy(), by), (variant, sb, "bytes")
        run_limited(T, dm, f"bits_pack {sb}-byte", ntiles, pack, got, side=(sb == 4 and variant == "mixed"))

        # a capacity in the middle of a later tile, and the stream's own size: nothing at or past it is written
        for cap in (int(boff[64 * 9 + 17]) + 1, int(boff[-1])):
            def pack_capped(stream, gs=gs, cap=cap):
                buf = guarded(T, cap, T.uint8)
                o = guarded(T, n + 1, T.int32)
                ws = T.empty(int(dm.lib().dctq_bits_workspace_bytes(n)) // 4 + 1, dtype=T.int32, device="cuda")
                dm._check(dm.lib().dctq_bits_pack(ptr(gs), sb, ptr(goff), n, ptr(o), ptr(buf), cap, ptr(ws), dm._stream_ptr(stream)))
                return [buf, o]

            capped = pack_capped(None)
            assert guard_intact(T, capped[0], cap) and guard_intact(T, capped[1], n + 1)
            assert np.array_equal(capped[0][:cap].cpu().numpy(), by[:cap]) and np.array_equal(capped[1][:n + 1].cpu().numpy().view(np.uint32), boff)
            run_limited(T, dm, f"bits_pack {sb}-byte, capacity", ntiles, pack_capped, capped)

    gby, gboff = gpu(T, by), gpu(T, boff.view(np.int32))

    def decode(stream):
        out = guarded(T, n * 64, T.int16)
        dm.bits_decode(gby, gboff, out=out, stream=stream)
        return [out]

    dec = decode(None)
    assert guard_intact(T, dec[0], n * 64)
    want = bits_ref.unpack(by, boff)
    assert np.array_equal(want, coef)
    assert np.array_equal(dec[0][:n * 64].cpu().numpy().reshape(n, 64), want)
    run_limited(T, dm, "bits_decode", ntiles, decode, dec, side=(variant == "dense"))


# ---- 3. the pixel decoders and the distortion -------------------------------------------------------------
PIXEL_CASES = [("mixed", 50, 0), ("mixed", 75, 0), ("mixed", 50, 1), ("dense", 100, 0)]  # fp32, fp64, adaptive; chunked


@pytest.mark.parametrize("variant,q,ad", PIXEL_CASES)
def test_pixel_decoders(T, dm, variant, q, ad):
    ref = oracle_case(variant, q, ad)
    off, sym, sym16, by, boff = streams(variant, q, ad)
    nbs = nblocks(SHAPES)
    coefs = [gpu(T, c) for c, _, _, _ in ref]
    vns = [gpu(T, v) for _, v, _, _ in ref] if ad else None
    goff, gby, gboff = gpu(T, off.view(np.int32)), gpu(T, by), gpu(T, boff.view(np.int32))
    if variant == "dense":
        assert all(later_halves_exceed_stage(boff))

    def into_padded(decoder):
        def call(stream):
            bv = padded(T, SHAPES)
            decoder(dm.Plan(q, ad), [v for _, v in bv], stream)
            return [b for b, _ in bv]
        return call

    calls = {"decode_planes": (batches(nbs, 32), into_padded(
        lambda plan, outs, stream: plan.decode_planes(coefs, outs=outs, var_nums=vns, stream=stream)))}
    for name, s in [("decode_symbols 4-byte", sym.view(np.int32))] + ([("decode_symbols 2-byte", sym16.view(np.int16))] if sym16 is not None else []):
        calls[name] = (20, into_padded(
            lambda plan, outs, stream, gs=gpu(T, s): plan.decode_symbols(gs, goff, outs=outs, var_nums=vns, stream=stream)))
    calls["decode_bits"] = (20, into_padded(
        lambda plan, outs, stream: plan.decode_bits(gby, gboff, outs=outs, var_nums=vns, stream=stream)))
    assert calls["decode_planes"][0] == 26 + 7 + 7 and -(-sum(nbs) // 64) == 20
    assert "decode_symbols 2-byte" in calls or q != 50, "a q50 plan admits 2-byte symbols"

    first = None
    for name, (nbatch, call) in calls.items():
        bufs = call(None)
        T.cuda.synchronize()
        for k, (f, h, w) in enumerate(SHAPES):
            view = bufs[k][:, :h, :w]
            assert untouched_outside(T, bufs[k], view), (name, k, "bytes outside width x height were written")
            want = np.clip(untile(ref[k][3], f, h, w), 0.0, 255.0)
            err = np.abs(view.cpu().numpy().astype(np.float64) - want).max()
            assert err <= TOL_PIXEL, (variant, q, ad, name, k, err)
        if first is None:
            first = bufs
        assert all(bit_equal(T, a, b) for a, b in zip(bufs, first)), (name, "the decoders disagree")
        run_limited(T, dm, name, nbatch, call, bufs, side=(name == "decode_bits" and variant == "mixed" and ad == 1))


@pytest.mark.parametrize("variant,q,ad", PIXEL_CASES[:3])
def test_distortion(T, dm, variant, q, ad):
    nbs = nblocks(SHAPES)
    planes = [v for _, v in padded(T, SHAPES, host_planes(variant))]
    plan = dm.Plan(q, ad)
    want = T.cat([TD.composition(T, plan, p, ad) for p in planes])  # tests/test_distortion_gpu.py

    def distortion(stream):
        out = guarded(T, sum(nbs), T.int32)
        dm.Plan(q, ad).distortion_planes(planes, out=out, stream=stream)
        return [out]

    got = distortion(None)
    assert guard_intact(T, got[0], sum(nbs))
    assert T.equal(got[0][:sum(nbs)].long(), want), (variant, q, ad, int((got[0][:sum(nbs)].long() != want).sum()))
    run_limited(T, dm, "distortion_planes", batches(nbs, 64), distortion, got, side=(ad == 1))


# ---- 4. block lengths and offsets ------------------------------------------------------------------------------
NLEN = 4003  # 1 001 groups of 4 lengths (width 1), the last one partial; 63 tiles of 64


@pytest.mark.parametrize("lb", [1, 2])
def test_block_lengths(T, dm, lb):
    """A lane takes 4 (width 1) or 2 (width 2) lengths per round and carries its running maximum
    from round to round: the length above 255 and the saturating one sit late in the array, in a
    lane's fourth round at limit 1 (its second at limit 3), so the maximum comes from there."""
    rng = np.random.default_rng(40 + lb)
    ln = rng.integers(0, 256, NLEN)
    ln[NLEN - 100], ln[NLEN - 37] = 300, 70000
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    per = 4 // lb
    ngroups = -(-NLEN // per)
    assert ngroups // (64 * WAVES) >= 3, "every lane gets 3 rounds at limit 1"
    assert (NLEN - 100) // per >= 3 * 64 * WAVES, "the long lengths fall into a lane's fourth round or later"
    goff = gpu(T, off.view(np.int32))

    def lengths(stream):
        buf = guarded(T, NLEN * lb, T.uint8)
        mx = T.full((1,), 0x5A5A5A5A, dtype=T.int32, device="cuda")
        dm._check(dm.lib().dctq_block_lengths(ptr(goff), NLEN, lb, ptr(buf), ptr(mx), dm._stream_ptr(stream)))
        return [buf, mx]

    got = lengths(None)
    want = frame_ref.lengths_from_offsets(off)
    assert np.array_equal(want, ln)
    assert guard_intact(T, got[0], NLEN * lb)
    raw = got[0][:NLEN * lb].cpu().numpy().view(np.uint8 if lb == 1 else np.uint16)
    assert np.array_equal(raw, np.minimum(want, 255 if lb == 1 else 65535))
    assert int(got[1].item()) == 70000
    nbatch = -(-ngroups // 64)
    run_limited(T, dm, f"block_lengths width {lb}", nbatch, lengths, got, side=(lb == 2))


@pytest.mark.parametrize("lb", [1, 2])
def test_block_offsets(T, dm, lb):
    rng = np.random.default_rng(50 + lb)
    ln = rng.integers(0, 256 if lb == 1 else 369, NLEN)
    if lb == 2:
        ln[[7, NLEN - 300, NLEN - 2]] = [369, 65535, 40000]  # clamped to 368, early and in later tiles
    want = frame_ref.offsets_from_lengths(ln)
    g = gpu(T, ln.astype(np.uint8 if lb == 1 else np.uint16).view(np.uint8 if lb == 1 else np.int16))

    def offsets(stream):
        out = guarded(T, NLEN + 1, T.int32)
        dm.block_offsets(g, out=out, stream=stream)
        return [out]

    got = offsets(None)
    assert guard_intact(T, got[0], NLEN + 1)
    assert np.array_equal(got[0][:NLEN + 1].cpu().numpy().view(np.uint32), want)
    run_limited(T, dm, f"block_offsets width {lb}", -(-NLEN // 64), offsets, got, side=(lb == 1))


# ---- 5. colour ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", ["rgb", "rgbx", "planar"])
def test_colour(T, dm, layout, sub):
    """A lane takes one patch (8 pixels by 2 rows, 4:4:4: by 1) per round: 18 patches per row, so
    row ends and frame boundaries fall inside every wave, 13 or 27 rounds per lane at limit 1.
    (4:2:0 needs a width of 16 n: 144, whose chroma planes are the picture set's (4, 48, 72).)"""
    shape = RGB_SHAPE
    f, h, w = shape
    rgb, want_planes, planes, want_rgb = TC.case(shape, sub)
    npatch = f * (h // (2 if sub == "420" else 1)) * (w // 8)
    assert npatch // (64 * WAVES) >= 3
    nbatch = -(-npatch // 64)
    src_buf, src, bgr = TC.rgb_buffer(T, layout, shape, pad=4, gap=8, fill=SENTINEL)
    src.copy_(TC.in_memory(T, layout, rgb))
    pshapes = TC.plane_shapes(shape, sub)

    def forward(stream):
        bv = padded(T, pshapes)
        dm.rgb_to_ycbcr(src, sub, outs=[v for _, v in bv], bgr=bgr, stream=stream)
        return [b for b, _ in bv]

    got = forward(None)
    for k, (pf, ph, pw) in enumerate(pshapes):
        assert untouched_outside(T, got[k], got[k][:, :ph, :pw]), (layout, sub, k)
        assert np.array_equal(got[k][:, :ph, :pw].cpu().numpy(), want_planes[k]), (layout, sub, k)
    run_limited(T, dm, f"rgb_to_ycbcr {layout} {sub}", nbatch, forward, got, side=(layout == "rgb" and sub == "420"))

    gplanes = [v for _, v in padded(T, pshapes, planes)]

    def inverse(stream):
        buf, view, _ = TC.rgb_buffer(T, layout, shape, pad=4, gap=8, fill=SENTINEL)
        dm.ycbcr_to_rgb(*gplanes, out=view, bgr=bgr, stream=stream)
        return [buf]

    back = inverse(None)
    _, view, _ = TC.rgb_buffer(T, layout, shape, pad=4, gap=8, fill=SENTINEL)
    view = back[0].as_strided(view.size(), view.stride(), view.storage_offset())
    assert TC.untouched_outside(T, back[0], view), (layout, sub)
    assert np.array_equal(view[..., :3].cpu().numpy(), want_rgb), (layout, sub)
    assert layout != "rgbx" or bool((view[..., 3] == 255).all())
    run_limited(T, dm, f"ycbcr_to_rgb {layout} {sub}", nbatch, inverse, back, side=(layout == "planar" and sub == "444"))


# ---- 6. the container ------------------------------------------------------------------------------------------
BOX_FRAMES = 12  # 12 x (216 + 54 + 54) = 3 888 blocks: 972 groups of 4 lengths, 3 rounds for every lane of block_lengths


@pytest.mark.parametrize("variant,q,ad", [("mixed", 50, False), ("mixed", 50, True), ("dense", 100, False)])
def test_compress_decompress(T, dm, variant, q, ad):
    """compress and decompress launch the kernels of the cases above one after another (colour,
    forward or encoder, rle, bits, lengths; offsets, the bits decoder, colour).  The grid read back
    is that of each wrapper's LAST launch -- block_lengths for compress, the colour inverse for
    decompress -- so the picture is sized for that launch: 12 frames, 3 888 blocks, which gives every
    lane of block_lengths 3 rounds at limit 1 in either width (and every earlier kernel 60 tiles)."""
    rgb = gpu(T, host_rgb(variant, BOX_FRAMES))
    planes = list(dm.rgb_to_ycbcr(rgb, "420"))
    shapes = [tuple(p.shape) for p in planes]
    assert shapes == [(BOX_FRAMES,) + s[1:] for s in (RGB_SHAPE, SHAPES[1], SHAPES[2])]
    by, boff, vns, dec = TFR.uncontained(T, dm, planes, q, ad)  # tests/test_frame_gpu.py
    want = dm.ycbcr_to_rgb(*dec)
    box = dm.compress(rgb, q, ad)
    ref = frame_ref.pack(by.cpu().numpy(), TFR.u32(boff), shapes, q, ad,
                         None if vns is None else [v.cpu().numpy() for v in vns], colour=True)
    assert TFR.host_bytes(box) == ref, "the container differs from tools/frame_ref.py pack"
    pix = dm.decompress(box)
    assert T.equal(pix, want)
    lb = dm.frame_unpack(box)["length_bytes"]
    assert lb in (1, 2)
    n = sum(nblocks(shapes))
    assert n == 3888
    ngroups = -(-n // (4 // lb))  # block_lengths: a lane takes 4 / lb lengths per round
    assert ngroups // (64 * WAVES) >= 3, "every lane of block_lengths gets 3 rounds at limit 1"
    run_limited(T, dm, "compress", -(-ngroups // 64), lambda stream: [dm.compress(rgb, q, ad, stream=stream)], [box],
                side=ad)
    npatch = BOX_FRAMES * (RGB_SHAPE[1] // 2) * (RGB_SHAPE[2] // 8)  # ycbcr_to_rgb: a lane takes one patch per round
    assert npatch // (64 * WAVES) >= 3
    run_limited(T, dm, "decompress", -(-npatch // 64), lambda stream: [dm.decompress(box, stream=stream)], [pix],
                side=not ad)
