"""GPU: every batched entry point at the weakest alignment its contract admits, on buffers of
exactly their contractual size, all carved out of ONE device arena -- as a C host does that
keeps its planes, coefficient arrays, streams and workspaces in one allocation.

Every case runs three times: in an arena filled with 0xA5, in one filled with 0x00, and on
ordinary torch allocations of natural strides.  It asserts
  1. the arena run against the CPU yardstick the suite already uses for the operation (oracle,
     tools/bits_ref.py, tools/frame_ref.py, tools/color_ref.py): integers bit for bit, floats
     within 1e-4, pixels within 0.5 + 1e-4 of the clamped oracle value;
  2. the arena run against the run on torch allocations, every output bit for bit;
  3. that nothing else moved: every arena byte outside the call's outputs (gaps, margins, the row
     padding and frame gaps inside destination planes) still holds the fill byte, every input is
     byte for byte its snapshot from before the call, and the bytes around a workspace of exactly
     *_workspace_bytes(N) are untouched (its contents are scratch);
  4. that no neighbour leaks in: the outputs of the 0xA5 and the 0x00 arena are equal bit for bit
     (unused capacity and gaps read as valid zeros in one, as implausible data in the other).

Two layouts (LAYOUTS): "low" puts every pointer just above a 256-byte boundary at its minimum
alignment, "high" just below one.  Plane rows are width + 8 bytes apart and frames stride *
height + 8, so frames do not keep the rows' phase (at these widths, all 8 mod 16, a row pitch of
width + 8 is itself 0 mod 16: with the base 8 mod 16 every row of frame 0 starts 8 mod 16 and
every row of frame 1 at 0 mod 16); the RGB pitches are multiples of 4 that are not multiples of 8.

Shapes, the smallest at which each kernel can still go wrong: A, 4:2:0, 90 + 30 + 30 blocks (plane
changes inside 64-block tiles and 32-block batches, partial last tile and batch); B, four planes
of 1 + 65 + 18 + 1 blocks (every plane starts its own encoder batch: the workspace's worst case
per block); C, an RGB picture of (2, 24, 40) frames -- (2, 32, 48) for 4:2:0, whose chroma planes must
themselves be multiples of 8, so luma multiples of 16: the smallest such picture that is no smaller.  Plans (50, 0), (90, 0), (50, 1): the fp32
inverse, the fp64 inverse, the adaptive leaf."""
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
import color_ref  # noqa: E402
import frame_ref  # noqa: E402
# helpers and yardsticks of the existing tests, used as they stand
import test_decode_foreign_gpu as TF  # noqa: E402
import test_distortion_gpu as TD  # noqa: E402
import test_grid_stride_gpu as TG  # noqa: E402

# layout -> alignment class -> (residue, modulus) of every pointer of that class
LAYOUTS = {"low": {8: (8, 256), 16: (16, 256), 4: (4, 16), "rgb": (4, 16)},
           "high": {8: (248, 256), 16: (240, 256), 4: (12, 16), "rgb": (12, 16)}}
FILLS = [0xA5, 0x00]
GAP = 64            # fill bytes between two buffers, at least
MARGIN = 4096       # fill bytes before the first and after the last buffer, at least
ARENA = 512 << 10
SHAPES = {"A": [(2, 40, 72), (2, 24, 40), (2, 24, 40)],       # 90 + 30 + 30 blocks
          "B": [(1, 8, 8), (1, 8, 520), (3, 16, 24), (1, 8, 8)]}  # 1 + 65 + 18 + 1
RGB_SHAPES = {"444": (2, 24, 40), "420": (2, 32, 48)}  # 4:2:0 needs luma multiples of 16 (include/dct_amd.h)
PLANS = [(50, 0), (90, 0), (50, 1)]  # the fp32 inverse, the fp64 inverse, the adaptive leaf
TOL_FLOAT = 1e-4                     # include/dct_amd.h: forward-produced coefficients
TOL_PIXEL = TG.TOL_PIXEL             # tests/test_decode_gpu.py

layouts = pytest.mark.parametrize("layout", list(LAYOUTS))
plans = pytest.mark.parametrize("q,ad", PLANS)
shapes = pytest.mark.parametrize("name", list(SHAPES))


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


@functools.lru_cache(maxsize=None)
def plan_of(q, ad):
    import dct_amd
    return dct_amd.Plan(q, ad)


# ---- pictures and their references (computed once, read-only) -----------------------------------------
@functools.lru_cache(maxsize=None)
def pictures(name):
    """u8 [F, H, W] per plane of SHAPES[name]; the kind changes from frame to frame and from plane to
    plane, as tests/test_grid_stride_gpu.py host_planes mixes them."""
    import oracle as O
    out = []
    for k, (f, h, w) in enumerate(SHAPES[name]):
        out.append(np.stack([O.synth_plane(100 + 10 * k + i, O.KINDS[TG.MIX[(k + i) % 3]], w, h) for i in range(f)]))
    return TG.frozen(*out)


@functools.lru_cache(maxsize=None)
def rgb_picture(sub):
    """u8 [F, H, W, 3] of RGB_SHAPES[sub]: every channel a plane of its own, kinds mixed per frame."""
    import oracle as O
    f, h, w = RGB_SHAPES[sub]
    chans = [np.stack([O.synth_plane(300 + 10 * c + i, O.KINDS[TG.MIX[(c + i) % 3]], w, h) for i in range(f)])
             for c in range(3)]
    return TG.frozen(np.stack(chans, axis=-1))[0]


@functools.lru_cache(maxsize=None)
def oracle_case(name, q, ad):
    """Per plane: (coef int16 [nb, 64], var_num int32 [nb], float coefficients [nb, 64], reference
    recon + 128 [nb, 64]), frames concatenated, all from the oracle (as TG.oracle_case)."""
    import oracle as O
    out = []
    for p in pictures(name):
        cf = [O.forward_plane(fr, q, ad, want_float=True) for fr in p]
        coef = np.concatenate([c for c, _ in cf])
        var = np.concatenate([O.plane_variance(fr) for fr in p])
        vn = var * 4096.0
        assert np.array_equal(vn, np.round(vn))
        want = O.inverse_plane(coef, q, ad, var if ad else None) + 128.0
        out.append(TG.frozen(coef, vn.astype(np.int32), np.concatenate([f for _, f in cf]), want))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def streams(name, q, ad):
    """The coefficients' streams from the CPU coders: (offsets u32, 4-byte symbols u32, 2-byte symbols
    u16 or None, packed bytes u8, byte offsets u32), as TG.streams."""
    import oracle as O
    coef = np.concatenate([c for c, _, _, _ in oracle_case(name, q, ad)])
    off, sym = O.rle_encode_plane(coef)
    sym16 = O.pack16(sym) if np.abs(coef.astype(np.int32)).max() <= 511 else None
    by, boff = bits_ref.pack(bits_ref.blocks_of(sym, off))
    return TG.frozen(off, sym, sym16, by, boff)


def cat(name, q, ad, i):
    return np.concatenate([r[i] for r in oracle_case(name, q, ad)])


# ---- the arena ----------------------------------------------------------------------------------------------
def strided_offsets(start, sizes, strides):
    off = np.full((1,) * len(sizes), start, dtype=np.int64)
    for axis, (n, s) in enumerate(zip(sizes, strides)):
        shape = [1] * len(sizes)
        shape[axis] = n
        off = off + (np.arange(n, dtype=np.int64) * s).reshape(shape)
    return off.ravel()


class Placer:
    """Where a case's buffers live.  Every method returns what the C call takes: an address, or a
    plane / RGB descriptor."""

    def __init__(self, T, dm, fill):
        self.T, self.dm, self.fill = T, dm, fill
        self.ins, self.outs, self.scratches, self.snaps = [], [], [], None

    # -- flat buffers
    def flat_in(self, name, a, alignment):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        v = self.carve(name, raw.size, alignment)
        v.copy_(self.T.from_numpy(raw.copy()))
        self.ins.append((name, v))
        return v.data_ptr()

    def flat_out(self, name, nbytes, alignment):
        v = self.carve(name, nbytes, alignment)
        self.writable(v, None)
        self.outs.append((name, v))
        return v.data_ptr()

    def scratch(self, name, nbytes):
        """A workspace: contents free, and so no output."""
        v = self.carve(name, int(nbytes), 4)
        self.writable(v, None)
        self.scratches.append((name, v))  # an allocation of its own stays alive across the call
        return v.data_ptr()

    # -- a stack of u8 planes: an input when content [F, H, W] is given, else a destination
    def plane(self, name, shape, content=None):
        f, h, w = shape
        stride, fs = self.plane_strides(h, w)
        v = self.carve(name, (f - 1) * fs + (h - 1) * stride + w, 8)
        px = v.as_strided((f, h, w), (fs, stride, 1))
        if content is not None:
            px.copy_(self.T.from_numpy(np.array(content)))
            self.ins.append((name, v))  # the span, row padding and frame gaps included
        else:
            self.writable(v, px)
            self.outs.append((name, px))
        return self.dm._Plane(v.data_ptr(), stride, fs, w, h, f)

    def planes(self, name, shapes, contents=None):
        ds = [self.plane(f"{name}[{k}]", s, None if contents is None else contents[k]) for k, s in enumerate(shapes)]
        return (self.dm._Plane * len(ds))(*ds)

    # -- an interleaved RGB stack: step 3 or 4 bytes per pixel, B first in memory when bgr
    def rgb(self, name, shape, step, bgr, content=None):
        f, h, w = shape
        stride, fs = self.rgb_strides(h, w, step)
        v = self.carve(name, (f - 1) * fs + (h - 1) * stride + w * step, "rgb")
        mem = v.as_strided((f, h, w, step), (fs, stride, step, 1))
        if content is not None:
            m = content[..., ::-1] if bgr else content
            if step == 4:  # the fourth byte is ignored on input
                m = np.concatenate([m, np.full(m.shape[:3] + (1,), 0x5C, np.uint8)], axis=-1)
            mem.copy_(self.T.from_numpy(np.array(m)))
            self.ins.append((name, v))
        else:
            self.writable(v, mem)
            self.outs.append((name, mem))
        # pixels: the R byte of pixel (0,0), the third of the pixel when B comes first
        return self.dm._Rgb(v.data_ptr() + (2 if bgr else 0), stride, fs, -1 if bgr else 1, step, w, h, f)

    def snapshot(self):
        self.snaps = [(name, v, v.clone()) for name, v in self.ins]

    def finish(self):
        self.T.cuda.synchronize()
        for name, v, snap in self.snaps:
            assert self.T.equal(v, snap), f"the call modified its input {name}"
        self.guards()
        return {name: v.contiguous().cpu().numpy().view(np.uint8).copy() for name, v in self.outs}


class Arena(Placer):
    """One u8 device tensor filled with `fill`; carve() hands out views of exactly nbytes at the
    layout's residue for the pointer's alignment class, GAP fill bytes or more apart, MARGIN from
    either end."""

    def __init__(self, T, dm, fill, layout):
        super().__init__(T, dm, fill)
        self.layout = layout
        self.buf = T.full((ARENA,), fill, dtype=T.uint8, device="cuda")
        self.cursor = MARGIN
        self.free = np.zeros(ARENA, dtype=bool)   # bytes the call may write
        self.regions = []

    def place(self, nbytes, alignment, residue, modulus=256):
        """A view of exactly nbytes whose address is `residue` mod `modulus` (and so a multiple of
        `alignment`, the contract's minimum, and of nothing coarser that the residue does not imply)."""
        assert residue % alignment == 0 and modulus % alignment == 0
        base = self.buf.data_ptr()
        off = self.cursor + (residue - (base + self.cursor)) % modulus
        v = self.buf[off:off + nbytes]
        assert v.numel() == nbytes and off - self.cursor < modulus
        assert v.data_ptr() % modulus == residue and v.data_ptr() % alignment == 0, (hex(v.data_ptr()), residue)
        self.cursor = off + nbytes + GAP
        assert self.cursor - GAP + MARGIN <= ARENA, "the arena is too small for this case"
        return v, off

    def carve(self, name, nbytes, alignment):
        residue, modulus = LAYOUTS[self.layout][alignment]
        v, off = self.place(nbytes, 4 if alignment == "rgb" else alignment, residue, modulus)
        self.regions.append((name, off, off + nbytes))
        return v

    def plane_strides(self, h, w):
        stride = w + 8
        return stride, stride * h + 8

    def rgb_strides(self, h, w, step):
        stride = w * step + 4
        fs = stride * h + 4
        assert stride % 4 == 0 and stride % 8 and fs % 4 == 0 and fs % 8
        return stride, fs

    def writable(self, v, strided):
        start = v.data_ptr() - self.buf.data_ptr()
        if strided is None:
            self.free[start:start + v.numel()] = True
        else:
            self.free[strided_offsets(start, strided.size(), strided.stride())] = True

    def guards(self):
        host = self.buf.cpu().numpy()
        held = ~self.free
        for _, v in self.ins:  # inputs hold their content: checked against their snapshots
            start = v.data_ptr() - self.buf.data_ptr()
            held[start:start + v.numel()] = False
        bad = np.flatnonzero(held & (host != self.fill))
        if bad.size:
            b = int(bad[0])
            near = min(self.regions, key=lambda r: 0 if r[1] <= b < r[2] else min(abs(b - r[1]), abs(b - r[2] + 1)))
            raise AssertionError(f"{bad.size} bytes outside the outputs were written; the first at arena offset {b} "
                                 f"({b - near[1]} from the start, {b - near[2]} from the end of {near[0]})")


class Plain(Placer):
    """The same buffers as ordinary torch allocations of their own, planes at natural strides."""

    def carve(self, name, nbytes, alignment):
        return self.T.full((nbytes,), self.fill, dtype=self.T.uint8, device="cuda")

    def plane_strides(self, h, w):
        return w, w * h

    def rgb_strides(self, h, w, step):
        return w * step, w * step * h

    def writable(self, v, strided):
        pass

    def guards(self):
        pass


def run_case(T, dm, layout, build):
    """build(P) places the call's buffers with P and returns the call (-> its return code).  Runs it in
    the two arenas and on torch allocations, with the checks 2 to 4 of the module's docstring;
    returns the outputs of the 0xA5 arena (name -> bytes) for check 1."""
    runs = []
    for P in [Arena(T, dm, fill, layout) for fill in FILLS] + [Plain(T, dm, FILLS[0])]:
        call = build(P)
        P.snapshot()
        rc = call()
        assert rc == 0, (rc, dm.lib().dctq_error_string(rc))
        runs.append(P.finish())
    a5, zero, plain = runs
    assert a5 and a5.keys() == zero.keys() == plain.keys()
    for name, got in a5.items():
        assert got.shape == zero[name].shape and np.array_equal(got, zero[name]), \
            (name, "the output depends on the bytes around the buffers", int((got != zero[name]).sum()))
        assert got.shape == plain[name].shape and np.array_equal(got, plain[name]), \
            (name, "the arena run differs from the run on torch allocations", int((got != plain[name]).sum()))
    return a5


def parr(addresses):
    """A C array of pointers and the void * to it (keep the array alive across the call)."""
    a = (C.c_void_p * len(addresses))(*addresses)
    return a, C.cast(a, C.c_void_p)


def nblocks(name):
    return TG.nblocks(SHAPES[name])


def as_i16(raw):
    return raw.view(np.int16).reshape(-1, 64)


def check_pixels(out, key, name, q, ad, what):
    for k, (f, h, w) in enumerate(SHAPES[name]):
        want = np.clip(TG.untile(oracle_case(name, q, ad)[k][3], f, h, w), 0.0, 255.0)
        pix = out[f"{key}[{k}]"].reshape(f, h, w)
        err = np.abs(pix.astype(np.float64) - want).max()
        print(f"{what} {name} q{q} a{ad} plane {k}: pixel max err {err:.4f}")
        assert err <= TOL_PIXEL, (what, name, q, ad, k, err)


def test_the_arena_itself(T, dm):
    """place() gives the residue asked for, exact sizes, gaps and margins; the guard sees one byte."""
    for layout, classes in LAYOUTS.items():
        A = Arena(T, dm, 0xA5, layout)
        ends = MARGIN - GAP
        for alignment, (residue, modulus) in classes.items():
            for nbytes in (1, 150, 4097):
                v = A.carve(f"{alignment}", nbytes, alignment)
                off = v.data_ptr() - A.buf.data_ptr()
                assert v.data_ptr() % modulus == residue and v.numel() == nbytes
                assert off - ends >= GAP and off >= MARGIN
                ends = off + nbytes
        A.snapshot()
        A.finish()
        A.buf[ends] = 0  # one byte behind the last buffer
        with pytest.raises(AssertionError, match="outside the outputs"):
            A.finish()


# ---- 1. the forward family: pixels in -------------------------------------------------------------------------
@layouts
@plans
def test_forward_quant(T, dm, layout, q, ad):
    plan, px, (coef, vn, _, _) = plan_of(q, ad), pictures("A")[0], oracle_case("A", q, ad)[0]
    nb = nblocks("A")[0]

    def build(P):
        d = P.plane("pixels", px.shape, px)
        c, v = P.flat_out("coef", nb * 128, 16), P.flat_out("var_num", nb * 4, 4)
        return lambda: plan._L.dctq_forward_quant(plan._h, C.byref(d), c, v, dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    assert np.array_equal(as_i16(out["coef"]), coef) and np.array_equal(out["var_num"].view(np.int32), vn)


@layouts
@shapes
@plans
@pytest.mark.parametrize("with_var", [True, False])
def test_forward_quant_planes(T, dm, layout, name, q, ad, with_var):
    plan, ref, nbs = plan_of(q, ad), oracle_case(name, q, ad), nblocks(name)

    def build(P):
        ds = P.planes("pixels", SHAPES[name], pictures(name))
        keep, cp = parr([P.flat_out(f"coef[{k}]", n * 128, 16) for k, n in enumerate(nbs)])
        keep2, vp = parr([P.flat_out(f"var_num[{k}]", n * 4, 4) for k, n in enumerate(nbs)]) if with_var else (None, None)
        return lambda: (keep, keep2, plan._L.dctq_forward_quant_planes(plan._h, ds, len(nbs), cp, vp, dm._stream_ptr()))[2]

    out = run_case(T, dm, layout, build)
    for k, (coef, vn, _, _) in enumerate(ref):
        assert np.array_equal(as_i16(out[f"coef[{k}]"]), coef), (name, q, ad, k)
        assert not with_var or np.array_equal(out[f"var_num[{k}]"].view(np.int32), vn), (name, q, ad, k)


@layouts
@shapes
@plans
def test_round_trip_planes(T, dm, layout, name, q, ad):
    plan, ref, nbs = plan_of(q, ad), oracle_case(name, q, ad), nblocks(name)

    def build(P):
        ds = P.planes("pixels", SHAPES[name], pictures(name))
        k1, cp = parr([P.flat_out(f"coef[{k}]", n * 128, 16) for k, n in enumerate(nbs)])
        k2, vp = parr([P.flat_out(f"var_num[{k}]", n * 4, 4) for k, n in enumerate(nbs)])
        k3, rp = parr([P.flat_out(f"recon[{k}]", n * 256, 16) for k, n in enumerate(nbs)])
        return lambda: (k1, k2, k3, plan._L.dctq_round_trip_planes(plan._h, ds, len(nbs), cp, vp, rp, dm._stream_ptr()))[3]

    out = run_case(T, dm, layout, build)
    for k, (coef, vn, _, want) in enumerate(ref):
        assert np.array_equal(as_i16(out[f"coef[{k}]"]), coef), (name, q, ad, k)
        assert np.array_equal(out[f"var_num[{k}]"].view(np.int32), vn), (name, q, ad, k)
        err = np.abs(out[f"recon[{k}]"].view(np.float32).reshape(-1, 64).astype(np.float64) - want).max()
        print(f"round trip {name} q{q} a{ad} plane {k}: recon max err {err:.3e}")
        assert err <= TOL_FLOAT, (name, q, ad, k, err)


@layouts
@shapes
@plans
@pytest.mark.parametrize("sb", [4, 2])
def test_encode_planes(T, dm, layout, name, q, ad, sb):
    """symbols_capacity is the stream's exact total: the symbol buffer has no spare symbol."""
    import oracle as O
    plan, ref, nbs = plan_of(q, ad), oracle_case(name, q, ad), nblocks(name)
    assert plan.symbol_bytes == 2, "q50 and q90 admit 2-byte symbols"
    woff, wsym, wsym16, _, _ = streams(name, q, ad)
    total, n = int(woff[-1]), sum(nbs)
    fn = plan._L.dctq_encode_planes16 if sb == 2 else plan._L.dctq_encode_planes

    def build(P):
        ds = P.planes("pixels", SHAPES[name], pictures(name))
        keep, cp = parr([P.flat_out(f"coef[{k}]", m * 128, 16) for k, m in enumerate(nbs)])
        off, sym = P.flat_out("offsets", (n + 1) * 4, 4), P.flat_out("symbols", total * sb, 4)
        ws = P.scratch("workspace", plan._L.dctq_encode_workspace_bytes(n))
        return lambda: (keep, fn(plan._h, ds, len(nbs), cp, off, sym, total, ws, dm._stream_ptr()))[1]

    out = run_case(T, dm, layout, build)
    for k, (coef, _, _, _) in enumerate(ref):
        assert np.array_equal(as_i16(out[f"coef[{k}]"]), coef), (name, q, ad, sb, k)
    assert np.array_equal(out["offsets"].view(np.uint32), woff), (name, q, ad, sb)
    got = out["symbols"].view(np.uint16 if sb == 2 else np.uint32)
    assert np.array_equal(got, O.pack16(wsym) if sb == 2 else wsym), (name, q, ad, sb)
    assert sb == 4 or np.array_equal(got, wsym16)


@layouts
def test_forward_float(T, dm, layout):
    """The kernel reads the plan's DCT matrix only: one plan."""
    plan, px, want = plan_of(50, 0), pictures("A")[0], oracle_case("A", 50, 0)[0][2]
    nb = nblocks("A")[0]

    def build(P):
        d = P.plane("pixels", px.shape, px)
        c = P.flat_out("coef", nb * 256, 16)
        return lambda: plan._L.dctq_forward_float(plan._h, C.byref(d), c, dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    err = np.abs(out["coef"].view(np.float32).reshape(-1, 64).astype(np.float64) - want).max()
    print(f"forward_float: max err {err:.3e}")
    assert err <= TOL_FLOAT, err


@layouts
@plans
def test_inverse(T, dm, layout, q, ad):
    plan = plan_of(q, ad)
    coef, vn, want = cat("A", q, ad, 0), cat("A", q, ad, 1), cat("A", q, ad, 3)
    n = coef.shape[0]

    def build(P):
        c = P.flat_in("coef", coef, 16)
        v = P.flat_in("var_num", vn, 4) if ad else None
        r = P.flat_out("recon", n * 256, 16)
        return lambda: plan._L.dctq_inverse(plan._h, c, v, n, r, dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    err = np.abs(out["recon"].view(np.float32).reshape(n, 64).astype(np.float64) - want).max()
    print(f"inverse q{q} a{ad}: max err {err:.3e}")
    assert err <= TOL_FLOAT, (q, ad, err)


# ---- 2. the pixel decoders ------------------------------------------------------------------------------------
def var_inputs(P, name, q, ad):
    if not ad:
        return None, None
    return parr([P.flat_in(f"var_num[{k}]", r[1], 4) for k, r in enumerate(oracle_case(name, q, ad))])


@layouts
@shapes
@plans
def test_decode_planes(T, dm, layout, name, q, ad):
    plan, ref = plan_of(q, ad), oracle_case(name, q, ad)

    def build(P):
        k1, cp = parr([P.flat_in(f"coef[{k}]", r[0], 16) for k, r in enumerate(ref)])
        k2, vp = var_inputs(P, name, q, ad)
        ds = P.planes("dst", SHAPES[name])
        return lambda: (k1, k2, plan._L.dctq_decode_planes(plan._h, cp, vp, ds, len(ref), dm._stream_ptr()))[2]

    check_pixels(run_case(T, dm, layout, build), "dst", name, q, ad, "decode_planes")


@layouts
@shapes
@plans
@pytest.mark.parametrize("sb", [4, 2])
def test_decode_symbols_planes(T, dm, layout, name, q, ad, sb):
    plan = plan_of(q, ad)
    off, sym, sym16, _, _ = streams(name, q, ad)
    assert sym16 is not None

    def build(P):
        s, o = P.flat_in("symbols", sym16 if sb == 2 else sym, 4), P.flat_in("offsets", off, 4)
        keep, vp = var_inputs(P, name, q, ad)
        ds = P.planes("dst", SHAPES[name])
        return lambda: (keep, plan._L.dctq_decode_symbols_planes(plan._h, s, sb, o, vp, ds, len(SHAPES[name]),
                                                                 dm._stream_ptr()))[1]

    check_pixels(run_case(T, dm, layout, build), "dst", name, q, ad, f"decode_symbols {sb}-byte")


@layouts
@shapes
@plans
def test_decode_bits_planes(T, dm, layout, name, q, ad):
    plan = plan_of(q, ad)
    _, _, _, by, boff = streams(name, q, ad)

    def build(P):
        b, o = P.flat_in("bytes", by, 4), P.flat_in("offsets", boff, 4)
        keep, vp = var_inputs(P, name, q, ad)
        ds = P.planes("dst", SHAPES[name])
        return lambda: (keep, plan._L.dctq_decode_bits_planes(plan._h, b, o, vp, ds, len(SHAPES[name]),
                                                              dm._stream_ptr()))[1]

    check_pixels(run_case(T, dm, layout, build), "dst", name, q, ad, "decode_bits")


# ---- 3. run-length symbols and the packed stream: no plan ---------------------------------------------------
STREAM = ("A", 50, 0)


@layouts
def test_rle_count(T, dm, layout):
    L, coef, off = dm.lib(), cat(*STREAM, 0), streams(*STREAM)[0]
    n = coef.shape[0]

    def build(P):
        c, o = P.flat_in("coef", coef, 16), P.flat_out("offsets", (n + 1) * 4, 4)
        ws = P.scratch("workspace", L.dctq_rle_workspace_bytes(n))
        return lambda: L.dctq_rle_count(c, n, o, ws, dm._stream_ptr())

    assert np.array_equal(run_case(T, dm, layout, build)["offsets"].view(np.uint32), off)


@layouts
def test_rle_emit(T, dm, layout):
    L, coef, (off, sym, _, _, _) = dm.lib(), cat(*STREAM, 0), streams(*STREAM)
    n = coef.shape[0]

    def build(P):
        c, o = P.flat_in("coef", coef, 16), P.flat_in("offsets", off, 4)
        s = P.flat_out("symbols", sym.size * 4, 4)
        return lambda: L.dctq_rle_emit(c, n, o, s, dm._stream_ptr())

    assert np.array_equal(run_case(T, dm, layout, build)["symbols"].view(np.uint32), sym)


@layouts
@pytest.mark.parametrize("sb", [4, 2])
def test_rle_decode(T, dm, layout, sb):
    """dctq_rle_decode (4-byte symbols) and dctq_rle_decode16."""
    L, coef, (off, sym, sym16, _, _) = dm.lib(), cat(*STREAM, 0), streams(*STREAM)
    n = coef.shape[0]
    want = TF.rle_decode_cpu(off, sym)
    assert np.array_equal(want, coef)
    fn = L.dctq_rle_decode16 if sb == 2 else L.dctq_rle_decode

    def build(P):
        s, o = P.flat_in("symbols", sym16 if sb == 2 else sym, 4), P.flat_in("offsets", off, 4)
        c = P.flat_out("coef", n * 128, 16)
        return lambda: fn(s, o, n, c, dm._stream_ptr())

    assert np.array_equal(as_i16(run_case(T, dm, layout, build)["coef"]), want)


@layouts
@pytest.mark.parametrize("sb", [4, 2])
def test_bits_pack(T, dm, layout, sb):
    """bytes_capacity is the stream's exact size."""
    L, (off, sym, sym16, by, boff) = dm.lib(), streams(*STREAM)
    n = off.size - 1

    def build(P):
        s, so = P.flat_in("symbols", sym16 if sb == 2 else sym, 4), P.flat_in("sym_offsets", off, 4)
        o, b = P.flat_out("offsets", (n + 1) * 4, 4), P.flat_out("bytes", by.size, 4)
        ws = P.scratch("workspace", L.dctq_bits_workspace_bytes(n))
        return lambda: L.dctq_bits_pack(s, sb, so, n, o, b, by.size, ws, dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    assert np.array_equal(out["offsets"].view(np.uint32), boff) and np.array_equal(out["bytes"], by)


@layouts
def test_bits_decode(T, dm, layout):
    L, coef, (_, _, _, by, boff) = dm.lib(), cat(*STREAM, 0), streams(*STREAM)
    n = coef.shape[0]
    want = bits_ref.unpack(by, boff)
    assert np.array_equal(want, coef)

    def build(P):
        b, o = P.flat_in("bytes", by, 4), P.flat_in("offsets", boff, 4)
        c = P.flat_out("coef", n * 128, 16)
        return lambda: L.dctq_bits_decode(b, o, n, c, dm._stream_ptr())

    assert np.array_equal(as_i16(run_case(T, dm, layout, build)["coef"]), want)


# ---- 4. block lengths and offsets -------------------------------------------------------------------------------
LENGTHS = ("A", 90, 0)  # the densest of the three streams (blocks of up to 78 B); 150 lengths: a partial last group


@layouts
@pytest.mark.parametrize("lb", [1, 2])
def test_block_lengths(T, dm, layout, lb):
    L, boff = dm.lib(), streams(*LENGTHS)[4]
    n = boff.size - 1
    want = frame_ref.lengths_from_offsets(boff)

    def build(P):
        o = P.flat_in("offsets", boff, 4)
        ln, mx = P.flat_out("lengths", n * lb, 4), P.flat_out("max_length", 4, 4)
        return lambda: L.dctq_block_lengths(o, n, lb, ln, mx, dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    got = out["lengths"].view(np.uint8 if lb == 1 else np.uint16)
    assert np.array_equal(got, np.minimum(want, 255 if lb == 1 else 65535))
    assert int(out["max_length"].view(np.uint32)[0]) == int(want.max())


@layouts
@pytest.mark.parametrize("lb", [1, 2])
def test_block_offsets(T, dm, layout, lb):
    L, boff = dm.lib(), streams(*LENGTHS)[4]
    n = boff.size - 1
    ln = np.minimum(frame_ref.lengths_from_offsets(boff), 255 if lb == 1 else 65535).astype(np.uint8 if lb == 1 else np.uint16)
    want = frame_ref.offsets_from_lengths(ln)

    def build(P):
        i, o = P.flat_in("lengths", ln, 4), P.flat_out("offsets", (n + 1) * 4, 4)
        ws = P.scratch("workspace", L.dctq_block_offsets_workspace_bytes(n))
        return lambda: L.dctq_block_offsets(i, lb, n, o, ws, dm._stream_ptr())

    assert np.array_equal(run_case(T, dm, layout, build)["offsets"].view(np.uint32), want)


# ---- 5. sizes and distortion ----------------------------------------------------------------------------------
@layouts
def test_huffman_bits(T, dm, layout):
    import oracle as O
    L, coef = dm.lib(), cat(*STREAM, 0)
    n = coef.shape[0]

    def build(P):
        c, b = P.flat_in("coef", coef, 16), P.flat_out("bits", n * 4, 4)
        return lambda: L.dctq_huffman_bits(c, n, b, dm._stream_ptr())

    assert np.array_equal(run_case(T, dm, layout, build)["bits"].view(np.uint32), O.huffman_bits_plane(coef))


@layouts
@shapes
@plans
def test_huffman_bits_planes(T, dm, layout, name, q, ad):
    import oracle as O
    plan, n = plan_of(q, ad), sum(nblocks(name))

    def build(P):
        ds = P.planes("pixels", SHAPES[name], pictures(name))
        b = P.flat_out("bits", n * 4, 4)
        return lambda: plan._L.dctq_huffman_bits_planes(plan._h, ds, len(SHAPES[name]), b, dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    assert np.array_equal(out["bits"].view(np.uint32), O.huffman_bits_plane(cat(name, q, ad, 0))), (name, q, ad)


@layouts
@shapes
@plans
def test_distortion_planes(T, dm, layout, name, q, ad):
    """The yardsticks of tests/test_distortion_gpu.py: the oracle's sandwich with T = 0.5 + 1e-4, and
    equality with the composition forward_quant_planes + decode_planes on torch allocations."""
    plan, n = plan_of(q, ad), sum(nblocks(name))

    def build(P):
        ds = P.planes("pixels", SHAPES[name], pictures(name))
        s = P.flat_out("sse", n * 4, 4)
        return lambda: plan._L.dctq_distortion_planes(plan._h, ds, len(SHAPES[name]), s, dm._stream_ptr())

    sse = run_case(T, dm, layout, build)["sse"].view(np.uint32).astype(np.int64)
    lo, hi, comp = [], [], []
    for (f, h, w), px, (_, _, _, want) in zip(SHAPES[name], pictures(name), oracle_case(name, q, ad)):
        e = np.abs(px.astype(np.float64) - np.clip(TG.untile(want, f, h, w), 0.0, 255.0))
        lo.append(TD.block_sums(np.maximum(e - TD.TOL, 0.0) ** 2, f, h, w))
        hi.append(TD.block_sums((e + TD.TOL) ** 2, f, h, w))
        comp.append(TD.composition(T, plan, TG.gpu(T, px), ad).cpu().numpy())
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    assert (lo <= sse).all() and (sse <= hi).all(), (name, q, ad)
    assert np.array_equal(sse, np.concatenate(comp)), (name, q, ad)


# ---- 6. colour and the synthetic frames ---------------------------------------------------------------------------
RGB_LAYOUTS = {"rgb": (3, False), "bgrx": (4, True)}
colours = pytest.mark.parametrize("packing", list(RGB_LAYOUTS))
subs = pytest.mark.parametrize("sub", ["420", "444"])


def plane_shapes(sub):
    f, h, w = RGB_SHAPES[sub]
    s = 2 if sub == "420" else 1
    return [(f, h, w), (f, h // s, w // s), (f, h // s, w // s)]


@layouts
@colours
@subs
def test_rgb_to_ycbcr_planes(T, dm, layout, packing, sub):
    L, (step, bgr), rgb = dm.lib(), RGB_LAYOUTS[packing], rgb_picture(sub)
    want = color_ref.forward(rgb, sub)

    def build(P):
        src = P.rgb("rgb", RGB_SHAPES[sub], step, bgr, rgb)
        ds = P.planes("plane", plane_shapes(sub))
        return lambda: L.dctq_rgb_to_ycbcr_planes(C.byref(src), C.byref(ds[0]), C.byref(ds[1]), C.byref(ds[2]),
                                                  dm._stream_ptr())

    out = run_case(T, dm, layout, build)
    for k, s in enumerate(plane_shapes(sub)):
        assert np.array_equal(out[f"plane[{k}]"].reshape(s), want[k]), (packing, sub, k)


@layouts
@colours
@subs
def test_ycbcr_to_rgb_planes(T, dm, layout, packing, sub):
    L, (step, bgr) = dm.lib(), RGB_LAYOUTS[packing]
    planes = [np.ascontiguousarray(p).astype(np.uint8) for p in color_ref.forward(rgb_picture(sub), sub)]
    want = color_ref.inverse(*planes)
    f, h, w = RGB_SHAPES[sub]

    def build(P):
        ds = P.planes("plane", plane_shapes(sub), planes)
        dst = P.rgb("rgb", RGB_SHAPES[sub], step, bgr)
        return lambda: L.dctq_ycbcr_to_rgb_planes(C.byref(ds[0]), C.byref(ds[1]), C.byref(ds[2]), C.byref(dst),
                                                  dm._stream_ptr())

    mem = run_case(T, dm, layout, build)["rgb"].reshape(f, h, w, step)
    assert np.array_equal(mem[..., 2::-1] if bgr else mem[..., :3], want), (packing, sub)
    assert step == 3 or (mem[..., 3] == 255).all()


@layouts
@pytest.mark.parametrize("kind", ["uniform", "smooth", "const", "extreme"])
def test_synth(T, dm, layout, kind):
    import oracle as O
    L, (f, h, w), seed = dm.lib(), SHAPES["A"][0], 77

    def build(P):
        d = P.plane("dst", (f, h, w))
        return lambda: L.dctq_synth(seed, dm.KINDS[kind], C.byref(d), dm._stream_ptr())

    want = np.stack([O.synth_plane(seed + i, O.KINDS[kind], w, h) for i in range(f)])
    assert np.array_equal(run_case(T, dm, layout, build)["dst"].reshape(f, h, w), want), kind
