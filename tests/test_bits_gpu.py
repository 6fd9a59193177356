"""GPU: the bit-packed coefficient stream "bits v1" (dctq_bits_pack, dctq_bits_decode,
dctq_decode_bits_planes; dct_amd.bits_pack / bits_decode, Plan.decode_bits /
encode_bits_planes).

The yardstick of the format is tools/bits_ref.py, plain Python written from the
specification: the packer must reproduce its bytes and offsets bit for bit, and the
decoders its coefficients for ANY bytes.  The two contracts on top are equivalences:
bits_decode(bits_pack(S)) == rle_decode(S) for any symbols S, and decode_bits ==
decode_symbols (== bits_decode + decode_planes), bit for bit."""
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
import bits_ref  # noqa: E402

KIND_NAMES = ["uniform", "smooth", "const", "extreme"]
QUALITIES = [10, 50, 90, 100]
GEOMETRY = {  # shapes (F, H, W) of the planes of one call
    "65 blocks": [(1, 8, 520)],                                  # one full tile plus one block
    "4:2:0 x 2": [(2, 32, 48), (2, 16, 24), (2, 16, 24)],        # 48 + 12 + 12: tiles and halves straddle planes
    "1 block": [(1, 8, 8)],
}
SENTINEL = 0xA5
EINVAL = -1
DEC_STAGE, PACK_STAGE = 2560, 8192  # bits_core.h kBitsStage (per half), bits.hip kPackStage (per tile)


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


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def widths_of(plan):
    return [4, 2] if plan.symbol_bytes == 2 else [4]


def nblocks(shapes):
    return [f * (h // 8) * (w // 8) for f, h, w in shapes]


def split_planes(coef, nbs):
    out, first = [], 0
    for nb in nbs:
        out.append(coef[first:first + nb])
        first += nb
    return out


def synth_planes(dm, shapes, kind, seed=700):
    return [dm.synth(seed + k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]


def reference_stream(sym, off):
    """bits_ref.pack of a device symbol stream: (bytes u8, offsets u32)."""
    s = sym.cpu().numpy()
    return bits_ref.pack(bits_ref.blocks_of(s, u32(off)))


def assert_pack_equals_reference(T, dm, sym, off, what):
    """Pack on the GPU, compare with the reference, and close the loop through both decoders."""
    got, boff = dm.bits_pack(sym, off)
    want, woff = reference_stream(sym, off)
    assert np.array_equal(u32(boff), woff), (what, "offsets")
    assert got.dtype == T.uint8 and got.numel() == int(woff[-1]), (what, got.numel(), int(woff[-1]))
    assert np.array_equal(got.cpu().numpy(), want), (what, "bytes")
    back = dm.bits_decode(got, boff)
    assert T.equal(back, dm.rle_decode(sym, off)), (what, "bits_decode(bits_pack(S)) != rle_decode(S)")
    return got, boff


# ---- 1. pack, bit for bit, and back ---------------------------------------------------------------
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("geo", list(GEOMETRY))
def test_pack_matches_reference(T, dm, geo, q):
    shapes = GEOMETRY[geo]
    plan = dm.Plan(q, 0)
    for kind in KIND_NAMES:
        planes = synth_planes(dm, shapes, kind)
        packed = {}
        for sb in widths_of(plan):
            _, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
            packed[sb] = assert_pack_equals_reference(T, dm, sym, off, (geo, q, kind, sb))
            total = int(u32(packed[sb][1])[-1])
            print(f"{geo} q{q} {kind} {sb}-byte: {sym.numel()} symbols -> {total} B "
                  f"({total / sum(nblocks(shapes)):.1f} B/block)")
        if 2 in packed:  # the stream does not depend on the symbol format it was packed from
            assert T.equal(packed[2][0], packed[4][0]) and T.equal(packed[2][1], packed[4][1])
        coefs, boff, by = plan.encode_bits_planes(planes)
        assert T.equal(by, packed[4][0]) and T.equal(boff, packed[4][1])
        assert T.equal(dm.bits_decode(by, boff), T.cat(coefs)), (geo, q, kind, "round trip of the coefficients")


# ---- 2. symbols no encoder of ours emits ---------------------------------------------------------------
def foreign_blocks():
    rng = np.random.default_rng(11)
    blocks = [
        [(0, 64)],                                              # the all-zero block
        [],                                                     # no symbols at all
        [(32767, 0), (-32767, 0), (-32768, 0), (1, 0), (-1, 0)],
        [(-32768, 64)] * 64,                                    # the worst case: 368 B
        [(5, 63)],                                              # exactly the last position
        [(7, 65), (9, 0)],                                      # runs past the block: clamped to 64, dropped either way
        [(3, 65535)],
        [(int(v), 0) for v in rng.integers(-32768, 32768, 70)],  # 70 symbols: the last 6 are not written
        [(int(v), int(r)) for v, r in zip(rng.integers(-600, 600, 70), rng.integers(0, 3, 70))],
        [(2, 10), (-3, 100), (6, 0)],
        [(100, 0), (-50, 0), (0, 62)],
    ]
    for _ in range(64):  # past one tile; any value, runs 0..64 and 65..65535
        n = int(rng.integers(0, 20))
        runs = np.where(rng.random(n) < 0.2, rng.integers(65, 65536, n), rng.integers(0, 65, n))
        blocks.append([(int(v), int(r)) for v, r in zip(rng.integers(-32768, 32768, n), runs)])
    return blocks


def symbols_of(blocks):
    sym = np.array([(v & 0xFFFF) | (r << 16) for b in blocks for v, r in b], np.uint32)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    return sym, off


def test_foreign_symbols(T, dm):
    blocks = foreign_blocks()
    assert len(blocks) > 64
    sym, off = symbols_of(blocks)
    gs, go = gpu(T, sym.view(np.int32)), gpu(T, off.view(np.int32))
    got, boff = assert_pack_equals_reference(T, dm, gs, go, "foreign")
    sizes = np.diff(u32(boff).astype(np.int64))
    assert sizes[0] == 2 and sizes[1] == 0 and sizes[3] == 368, sizes[:8]
    want = bits_ref.unpack(got.cpu().numpy(), u32(boff))
    assert np.array_equal(dm.bits_decode(got, boff).cpu().numpy(), want)
    assert want[2, 0] == 32767 and want[2, 8] == -32768 and want[4, 63] == 5 and not want[1].any()


# ---- 3. the decoders ------------------------------------------------------------------------------------
PLANS = [(50, 0), (75, 0), (50, 1)]  # fp32 inverse, fp64 non-adaptive, fp64 adaptive


@pytest.mark.parametrize("q,ad", PLANS)
@pytest.mark.parametrize("geo", list(GEOMETRY))
def test_decode_bits_equals_decode_symbols(T, dm, geo, q, ad):
    """Into strided destinations with sentinel padding and gaps between frames."""
    shapes, pad, gap = GEOMETRY[geo], 8, 3
    nbs = nblocks(shapes)
    plan = dm.Plan(q, ad)
    planes = [dm.synth(900 + k, KIND_NAMES[k % 4], s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    vns = [T.zeros(nb, dtype=T.int32, device="cuda") for nb in nbs]
    plan.forward_quant_planes(planes, var_nums=vns)
    vns = vns if ad else None
    _, off, sym = plan.encode_planes(planes)
    by, boff = dm.bits_pack(sym, off)
    want = plan.decode_symbols(sym, off, shapes=shapes, var_nums=vns)
    bufs = [T.full((s[0], s[1] + gap, s[2] + pad), SENTINEL, dtype=T.uint8, device="cuda") for s in shapes]
    views = [b[:, :s[1], :s[2]] for b, s in zip(bufs, shapes)]
    outs = plan.decode_bits(by, boff, outs=views, var_nums=vns)
    two = plan.decode_planes(split_planes(dm.bits_decode(by, boff), nbs), shapes=shapes, var_nums=vns)
    for k, s in enumerate(shapes):
        assert outs[k].data_ptr() == bufs[k].data_ptr()
        assert T.equal(views[k], want[k]), (geo, q, ad, k, int((views[k] != want[k]).sum()))
        assert T.equal(views[k], two[k]), (geo, q, ad, k, "bits_decode + decode_planes")
        outside = bufs[k].clone()
        outside[:, :s[1], :s[2]] = SENTINEL
        assert bool((outside == SENTINEL).all()), ("bytes outside width x height were written", k, s)
    again = plan.decode_bits(by, boff, shapes=shapes, var_nums=vns)
    assert all(T.equal(a, w) for a, w in zip(again, want))


# The four stream decoders share one tile loop, one coefficient sink and one pixel sink
# (tile_decode_core.h, decode_core.h): the tail tile, the tail half and a half that straddles
# planes, through all four at once.  One-frame planes of 8-pixel-high strips, N blocks in all:
# around a half (31, 32, 33), around a tile (63, 64, 65) and past two (129); from 33 on, three
# planes with one to three blocks in the middle one, placed so that one 32-block half holds
# blocks of all three -- the first half, the second (65) or the third (129).
TAIL_SPLITS = {1: [1], 31: [31], 32: [32], 33: [29, 2, 2], 63: [28, 3, 32], 64: [30, 1, 33], 65: [59, 3, 3],
               129: [92, 3, 34]}
# fp32 inverse; fp64 adaptive, 2-byte symbols allowed; fp64, 4-byte symbols only
TAIL_PLANS = [(50, 0), (90, 1), (100, 0)]


@pytest.mark.parametrize("q,ad", TAIL_PLANS)
def test_tails_and_straddles_through_all_four_decoders(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    assert widths_of(plan) == ([4] if q == 100 else [4, 2])
    pad, gap = 8, 3
    for total, split in TAIL_SPLITS.items():
        shapes = [(1, 8, 8 * n) for n in split]
        assert sum(nblocks(shapes)) == total
        if len(split) == 3:  # some half [32i, 32i + 32) holds blocks of all three planes
            lo, hi = split[0] - 1, split[0] + split[1]  # the last block of plane 0, the first of plane 2
            assert lo // 32 == hi // 32 and 0 <= lo and hi < total, split
        planes = synth_planes(dm, shapes, "uniform", seed=1400 + total)
        vns = [T.zeros(nb, dtype=T.int32, device="cuda") for nb in split]
        plan.forward_quant_planes(planes, var_nums=vns)
        vns = vns if ad else None
        pixels = None
        for sb in widths_of(plan):
            what = (q, ad, total, sb)
            coefs, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
            forward = T.cat(coefs)
            by, boff = dm.bits_pack(sym, off)
            from_symbols, from_bits = dm.rle_decode(sym, off), dm.bits_decode(by, boff)
            assert T.equal(from_symbols, forward), (what, "rle_decode(S) != the forward's coefficients")
            assert T.equal(from_bits, forward), (what, "bits_decode(bits_pack(S)) != the forward's coefficients")
            two = plan.decode_planes(split_planes(from_symbols, split), shapes=shapes, var_nums=vns)
            for name, decode in (("decode_symbols", lambda v: plan.decode_symbols(sym, off, outs=v, var_nums=vns)),
                                 ("decode_bits", lambda v: plan.decode_bits(by, boff, outs=v, var_nums=vns))):
                bufs = [T.full((1, 8 + gap, s[2] + pad), SENTINEL, dtype=T.uint8, device="cuda") for s in shapes]
                views = [b[:, :8, :s[2]] for b, s in zip(bufs, shapes)]
                decode(views)
                for k, s in enumerate(shapes):
                    assert T.equal(views[k], two[k]), (what, name, k, int((views[k] != two[k]).sum()))
                    bufs[k][:, :8, :s[2]] = SENTINEL
                    assert bool((bufs[k] == SENTINEL).all()), (what, name, k, "bytes outside width x height written")
            if pixels is not None:  # the pixels do not depend on the symbol format
                assert all(T.equal(a, b) for a, b in zip(two, pixels)), what
            pixels = two


def test_dense_and_staged_paths(T, dm):
    """Extremes at q100: a half's bytes exceed the decoders' stage and a tile's the packer's, so
    the chunked decode and the direct emit run; smooth content at q50 is staged whole."""
    shapes = [(1, 8, 520)]
    seen = {}
    for kind, q in (("extreme", 100), ("smooth", 50)):
        plan = dm.Plan(q, 0)
        planes = synth_planes(dm, shapes, kind)
        _, off, sym = plan.encode_planes(planes)
        by, boff = assert_pack_equals_reference(T, dm, sym, off, (kind, q))
        o = u32(boff).astype(np.int64)
        seen[kind] = (int(o[32] - o[0]), int(o[64] - o[0]))
        print(f"{kind} q{q}: first half {seen[kind][0]} B, first tile {seen[kind][1]} B")
        got = plan.decode_bits(by, boff, shapes=shapes)[0]
        assert T.equal(got, plan.decode_symbols(sym, off, shapes=shapes)[0]), (kind, q)
    assert seen["extreme"][0] > DEC_STAGE, seen
    assert seen["smooth"][0] <= DEC_STAGE - 3 and seen["smooth"][1] <= PACK_STAGE - 3, seen
    # the packer's own dense path: this encoder's densest tile stays below its stage (7.8 KB
    # above), so a foreign tile of 64 random int16 per block (about 250 B per block) takes it
    rng = np.random.default_rng(3)
    sym, off = symbols_of([[(int(v), 0) for v in rng.integers(-32768, 32768, 64)] for _ in range(66)])
    gs, go = gpu(T, sym.view(np.int32)), gpu(T, off.view(np.int32))
    by, boff = assert_pack_equals_reference(T, dm, gs, go, "foreign dense tile")
    o = u32(boff).astype(np.int64)
    assert o[64] - o[0] > PACK_STAGE and o[32] - o[0] > DEC_STAGE, o[[0, 32, 64]]
    plan = dm.Plan(75, 0)
    shapes = [(1, 8, 8 * 66)]
    assert T.equal(plan.decode_bits(by, boff, shapes=shapes)[0], plan.decode_symbols(gs, go, shapes=shapes)[0])


def test_side_stream(T, dm):
    plan = dm.Plan(50, 1)
    shapes = GEOMETRY["4:2:0 x 2"]
    planes = synth_planes(dm, shapes, "uniform")
    vns = [T.zeros(nb, dtype=T.int32, device="cuda") for nb in nblocks(shapes)]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, off, sym = plan.encode_planes(planes)
    by, boff = dm.bits_pack(sym, off)
    want = plan.decode_symbols(sym, off, shapes=shapes, var_nums=vns)
    T.cuda.synchronize()
    stream = T.cuda.Stream()
    with T.cuda.stream(stream):
        by2, boff2 = dm.bits_pack(sym, off, stream=stream)
        coef = dm.bits_decode(by2, boff2, stream=stream)
        got = plan.decode_bits(by2, boff2, shapes=shapes, var_nums=vns, stream=stream)
    stream.synchronize()
    assert T.equal(by2, by) and T.equal(boff2, boff)
    assert T.equal(coef, dm.rle_decode(sym, off))
    assert all(T.equal(g, w) for g, w in zip(got, want))
    dm.stream_release(stream)


# ---- 4. any bytes are a valid input ----------------------------------------------------------------------
def test_any_bytes_decode(T, dm):
    rng = np.random.default_rng(5)
    whole, _ = bits_ref.pack([[(int(v), 0) for v in rng.integers(-300, 300, 64)]])
    noise = rng.integers(0, 256, 256).astype(np.uint8)
    cuts = [0, 3, 100, 101, 200, 256]  # 256 random bytes split into 5 blocks
    parts = [whole[:len(whole) // 2],                  # a block cut mid-code through its offsets
             np.zeros(8, np.uint8),                    # all zero: a prefix of more than 16 zero bits
             np.zeros(0, np.uint8)]                    # empty
    parts += [noise[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    parts += [whole]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint32)
    data = np.concatenate(parts)
    want = bits_ref.unpack(data, off)
    assert not want[1].any() and not want[2].any() and np.array_equal(want[-1], bits_ref.unpack(whole, [0, len(whole)])[0])
    assert np.count_nonzero(want[0]) < 64 and want[0, 0] == want[-1, 0]
    n = len(parts)
    shape = (1, 8, 8 * n)
    for lead in (0, 1):  # the stream at a 4-byte aligned address, and one byte past one
        buf = np.full(lead + len(data) + 64, SENTINEL, np.uint8)
        buf[lead:lead + len(data)] = data
        g = gpu(T, buf)
        gb, go = g[lead:lead + len(data)], gpu(T, off.view(np.int32))
        coef = dm.bits_decode(gb, go)
        assert np.array_equal(coef.cpu().numpy(), want), lead
        for q, ad in PLANS:
            plan = dm.Plan(q, ad)
            vns = [T.full((n,), 4096 * 50, dtype=T.int32, device="cuda")] if ad else None
            got = plan.decode_bits(gb, go, shapes=[shape], var_nums=vns)[0]
            assert T.equal(got, plan.decode_planes([coef], shapes=[shape], var_nums=vns)[0]), (lead, q, ad)
        assert bool((g[lead + len(data):] == SENTINEL).all()) and bool((g[:lead] == SENTINEL).all())


# ---- 5. capacity ----------------------------------------------------------------------------------------------
def raw_pack(dm, T, sym, off, buf, cap, nblk=None, sb=None, boff=None, ws="ok", symbols="ok", sym_offsets="ok"):
    """dctq_bits_pack as a C host calls it.  Returns (rc, byte offsets tensor).  ws: "ok", None (NULL) or a
    number of bytes to add to the workspace's address."""
    L = dm.lib()
    n = off.numel() - 1 if nblk is None else nblk
    if boff is None:
        boff = T.full((off.numel(),), -1, dtype=T.int32, device="cuda")
    wsp = T.empty(int(L.dctq_bits_workspace_bytes(off.numel() - 1)) // 4 + 2, dtype=T.int32, device="cuda")
    rc = L.dctq_bits_pack(C.c_void_p(sym.data_ptr()) if symbols == "ok" else symbols,
                          (2 if sym.dtype == T.int16 else 4) if sb is None else sb,
                          C.c_void_p(off.data_ptr()) if sym_offsets == "ok" else None, n,
                          C.c_void_p(boff.data_ptr()) if boff is not False else None,
                          buf if isinstance(buf, (C.c_void_p, type(None))) else C.c_void_p(buf.data_ptr()), cap,
                          None if ws is None else C.c_void_p(wsp.data_ptr() + (0 if ws == "ok" else ws)), None)
    T.cuda.synchronize()
    return rc, boff


@pytest.mark.parametrize("kind,q", [("uniform", 50), ("extreme", 100), ("foreign", None)])
def test_capacity(T, dm, kind, q):
    """65 blocks: staged tiles (uniform, extremes) and a tile the packer stores directly (foreign)."""
    if kind == "foreign":
        rng = np.random.default_rng(4)
        s, o = symbols_of([[(int(v), 0) for v in rng.integers(-32768, 32768, 64)] for _ in range(65)])
        sym, off = gpu(T, s.view(np.int32)), gpu(T, o.view(np.int32))
    else:
        _, off, sym = dm.Plan(q, 0).encode_planes(synth_planes(dm, GEOMETRY["65 blocks"], kind))
    full, boff = dm.bits_pack(sym, off)
    total = full.numel()
    o = u32(boff).astype(np.int64)
    caps = sorted({0, 1, 5, int(o[1]), int(o[1]) + 1, int(o[33]) - 2, int(o[64]) - 1, int(o[64]) + 1, total - 1,
                   total, total + 9})
    for cap in caps:
        buf = T.full((total + 64,), SENTINEL, dtype=T.uint8, device="cuda")
        rc, got_off = raw_pack(dm, T, sym, off, buf, cap)
        assert rc == 0, cap
        assert T.equal(got_off, boff), (cap, "offsets must be complete")
        k = min(cap, total)
        assert T.equal(buf[:k], full[:k]), (cap, "bytes below the capacity")
        assert bool((buf[k:] == SENTINEL).all()), (cap, "a byte at or beyond the capacity was written")
    rc, got_off = raw_pack(dm, T, sym, off, None, 1 << 20)  # bytes == NULL: the offsets only
    assert rc == 0 and T.equal(got_off, boff)
    by0, off0 = dm.bits_pack(sym, off, capacity=0)
    assert by0.numel() == 0 and T.equal(off0, boff)
    by7, _ = dm.bits_pack(sym, off, capacity=7)
    assert T.equal(by7, full[:7])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------
def test_pack_and_decode_refusals(T, dm):
    L = dm.lib()
    plan = dm.Plan(50, 0)
    _, off, sym = plan.encode_planes(synth_planes(dm, [(1, 16, 32)], "uniform"), symbol_bytes=4)
    nblk = off.numel() - 1
    full, boff = dm.bits_pack(sym, off)
    buf = T.full((full.numel() + 64,), SENTINEL, dtype=T.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    bad = {
        "NULL symbols": dict(symbols=None),
        "NULL sym_offsets": dict(sym_offsets=None),
        "NULL offsets": dict(boff=False),
        "NULL workspace": dict(ws=None),
        "symbol_bytes 3": dict(sb=3),
        "symbol_bytes 0": dict(sb=0),
        "nblocks 0": dict(nblk=0),
        "nblocks 2^26": dict(nblk=1 << 26),
        "368 * nblocks >= 2^32": dict(nblk=11671107),
        "capacity < 0": dict(cap=-1),
        "misaligned bytes": dict(buf=C.c_void_p(buf.data_ptr() + 1)),
        "workspace + 1": dict(ws=1),
        "workspace + 2": dict(ws=2),
    }
    for what, kw in bad.items():
        kw = dict(kw)
        rc, got_off = raw_pack(dm, T, sym, off, kw.pop("buf", buf), kw.pop("cap", buf.numel()), **kw)
        assert rc == EINVAL, what
        assert L.dctq_error_string(EINVAL), what
        assert got_off is False or bool((got_off == -1).all()), (what, "a refused call wrote offsets")
    assert bool((buf == SENTINEL).all()), "a refused call wrote bytes"
    rc, got_off = raw_pack(dm, T, sym, off, buf, buf.numel())  # the same call, unrefused
    assert rc == 0 and T.equal(got_off, boff) and T.equal(buf[:full.numel()], full)

    coef = T.full((nblk, 64), 0x5A5A, dtype=T.int16, device="cuda")

    def dec(bytes_="ok", offsets="ok", n=nblk, out="ok"):
        rc = L.dctq_bits_decode(C.c_void_p(full.data_ptr()) if bytes_ == "ok" else None,
                                C.c_void_p(boff.data_ptr()) if offsets == "ok" else None, n,
                                C.c_void_p(coef.data_ptr()) if out == "ok" else None, None)
        T.cuda.synchronize()
        return rc

    for what, kw in {"NULL bytes": dict(bytes_=None), "NULL offsets": dict(offsets=None), "NULL coef": dict(out=None),
                     "nblocks 0": dict(n=0), "nblocks 2^26": dict(n=1 << 26)}.items():
        assert dec(**kw) == EINVAL, what
    assert bool((coef == 0x5A5A).all()), "a refused call wrote coefficients"
    assert dec() == 0 and T.equal(coef, dm.rle_decode(sym, off))


def test_decode_bits_planes_refusals(T, dm):
    L = dm.lib()
    plans = {0: dm.Plan(50, 0), 1: dm.Plan(50, 1)}
    w, h = 32, 16
    nblk = (w // 8) * (h // 8)
    px = T.full((h * w + 64,), SENTINEL, dtype=T.uint8, device="cuda")
    by = T.zeros(4 * nblk, dtype=T.uint8, device="cuda")
    off = (4 * T.arange(nblk + 1, dtype=T.int32, device="cuda")).contiguous()
    vn = T.zeros(nblk, dtype=T.int32, device="cuda")

    def call(ad=0, plan="ok", bytes_="ok", offsets="ok", vns="ok", dst="ok", nplanes=1, **geo):
        g = dict(pixels=px.data_ptr(), stride=w, frame_stride=w * h, width=w, height=h, nframes=1, vn=vn.data_ptr())
        g.update(geo)
        n = max(nplanes, 1)
        descs = (dm._Plane * n)(*[dm._Plane(g["pixels"], g["stride"], g["frame_stride"], g["width"], g["height"],
                                            g["nframes"]) for _ in range(n)])
        vp = (C.c_void_p * n)(*[g["vn"]] * n)
        return L.dctq_decode_bits_planes(plans[ad]._h if plan == "ok" else None,
                                         C.c_void_p(by.data_ptr()) if bytes_ == "ok" else None,
                                         C.c_void_p(off.data_ptr()) if offsets == "ok" else None,
                                         C.cast(vp, C.c_void_p) if vns == "ok" else None,
                                         descs if dst == "ok" else None, nplanes, None)

    bad = {
        "NULL plan": dict(plan=None),
        "NULL bytes": dict(bytes_=None),
        "NULL offsets": dict(offsets=None),
        "NULL dst": dict(dst=None),
        "NULL dst[k].pixels": dict(pixels=None),
        "nplanes 0": dict(nplanes=0),
        "nplanes 5": dict(nplanes=5),
        "adaptive without var_num": dict(ad=1, vns=None),
        "adaptive with a NULL var_num[k]": dict(ad=1, vn=None),
        "width 12": dict(width=12),
        "height 12": dict(height=12),
        "2^26 blocks": dict(width=8 * 8192, stride=8 * 8192, height=8 * 8192),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
    T.cuda.synchronize()
    assert bool((px == SENTINEL).all()), "a refused call wrote pixels"
    assert call(vns=None) == 0  # non-adaptive plans ignore var_num
    T.cuda.synchronize()
    assert bool((px[w * h:] == SENTINEL).all())
    p = plans[0]
    for bad_call in (lambda: p.decode_bits(by, off[:-1], shapes=[(h, w)]),
                     lambda: p.decode_bits(by, off.to(T.int64), shapes=[(h, w)]),
                     lambda: p.decode_bits(by, off.cpu(), shapes=[(h, w)]),
                     lambda: p.decode_bits(by.to(T.int32), off, shapes=[(h, w)]),
                     lambda: p.decode_bits(by, off),
                     lambda: plans[1].decode_bits(by, off, shapes=[(h, w)]),
                     lambda: dm.bits_decode(by.to(T.int16), off),
                     lambda: dm.bits_decode(by, off, out=T.zeros((nblk - 1, 64), dtype=T.int16, device="cuda")),
                     lambda: dm.bits_pack(by, off),
                     lambda: dm.bits_pack(vn, off.to(T.int64)),
                     lambda: dm.bits_pack(vn, off, symbol_bytes=2)):
        with pytest.raises(dm.DctqError):
            bad_call()


# ---- 7. C host -----------------------------------------------------------------------------------------------------------
def test_frame_bits_host(T, dm):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_bits"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for (w, h, q, ad, kind) in [(640, 480, 90, 1, 1), (64, 48, 50, 0, 0), (96, 80, 100, 0, 3)]:
        r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(ROOT, "host", "frame_bits"), str(w), str(h),
                            str(q), str(ad), "12345", str(kind)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        got = dict(l.split("=", 1) for l in r.stdout.strip().splitlines())
        assert got["fused_equal"] == "1" and got["padding_intact"] == "1" and got["abi_version"] == "6", got
        assert got["guard_intact"] == "1" and int(got["bytes_total"]) > 0, got
        assert int(got["blocks"]) == (w // 8) * (h // 8) * 3 // 2, got
