"""GPU: the symbol consumers (dctq_rle_decode, dctq_rle_decode16, dctq_decode_symbols_planes,
dctq_bits_pack) on streams no encoder of ours emits, in every density path, and the coefficient
consumers (dctq_rle_count / dctq_rle_emit, dctq_huffman_bits) at the ends of int16.

Part A.  rebuild_half (rle_decode_core.h) picks one of three paths per half tile of 32 blocks by
the half's symbol count: lane (<= 240), walk (<= 1024), quad (denser).  A catalogue of foreign
blocks -- empty, all-zero, 64 symbols over the whole value range, 65..300 symbols, runs of 64 to
65535 first and in mid-block, values landing exactly at positions 63 and 64, sums of run + 1 that
wrap 8, 16 and 22 bits, and for 2-byte symbols 0x0000 in mid-block, payload 0x200 and run field
63 -- is laid out as ten tiles whose halves take every ordered pair of paths (a wave rebuilds the
two halves of a tile one after the other in the same LDS), the tenth ragged (37 blocks), with a
half exactly on each side of each threshold.  The layout is checked on the host, from the offsets
and symbols alone, before any kernel runs: every half is in the path it was built for and every
path holds every feature.  Expected coefficients: test_decode_foreign_gpu.rle_decode_cpu (an
int64 cumsum), cross-checked on the host against tools/bits_ref.py unpack(pack(blocks)); expected
bytes: bits_ref.pack.  The pixel contracts are equivalences (include/dct_amd.h): decode_symbols
and decode_bits against decode_planes fed the CPU-decoded coefficients.  Everything is exact, and
everything runs a second time in one workgroup (dct_amd.grid_limit(1)), where a wave takes two
or three of the tiles in sequence.

Part B.  Coefficient tiles of {-32768, -32767, -1, 0, 1, 32767} and of uniform int16 through
rle_encode (both emit paths of rle.hip: tiles of <= 2048 symbols and denser) and huffman_bits
(every path of classify in huffman.hip) against the oracle, which is pinned to the compiled
reference at these magnitudes by tests/golden/huffman.json's int16_range block."""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bits_ref  # noqa: E402
from test_decode_foreign_gpu import plain_var_num, rle_decode_cpu  # noqa: E402

LANE_MAX, WALK_MAX = 240, 1024  # rle_decode_core.h kDecLaneMax, kDecWalkMax (symbols of a half tile)
PACK_STAGE = 8192               # bits.hip kPackStage (bytes of a tile the emit stages)
EMIT_LANE_MAX = 2048            # rle.hip kLaneWalkMax (symbols of a tile the lane-per-block emit stages)
PATHS = ("lane", "walk", "quad")
PLANS = [(50, 0), (90, 0), (50, 1)]  # fp32 inverse, fp64 inverse, adaptive
FIRST_PLANE = 100               # blocks of the first of the two planes: the boundary is inside tile 1's second half
# symbols of the halves of each path, in the order the layout meets them; the thresholds from both sides
TARGETS = {"lane": [240, 236, 215, 239, 202, 229], "walk": [241, 1024, 701, 334, 901, 512],
           "quad": [1025, 2100, 1501, 3000, 1203, 2502]}
RAGGED = [("quad", 32, 1707), ("walk", 5, 420)]  # the tenth tile: 37 blocks


def path_of(nsym):
    return "lane" if nsym <= LANE_MAX else "walk" if nsym <= WALK_MAX else "quad"


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


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@contextlib.contextmanager
def workgroups(dm, one):
    """one: every persistent launch inside runs as ONE workgroup; yields a check of that."""
    if not one:
        yield lambda: None
        return

    def check():
        assert dm.last_grid() == 1

    with dm.grid_limit(1):
        yield check


GRIDS = [pytest.param(False, id="full grid"), pytest.param(True, id="one workgroup")]


# ---- Part A: the catalogue -----------------------------------------------------------------------
def run0(values):
    return [(int(v), 0) for v in values]


def nonzero(rng, n, narrow):
    v = rng.integers(-512, 512, n) if narrow else rng.integers(-32768, 32768, n)
    return np.where(v == 0, 1, v)


def catalogue(narrow, path, rng):
    """(name, [(value, run), ...]) of generators 1-8 of the issue, for 4-byte symbols (any int16, runs to
    65535) or 2-byte ones (10-bit values, runs 0..63, and (0, 64) = 0x0000; a zero value needs run >= 1)."""
    top, low, lowest = (511, -511, -512) if narrow else (32767, -32767, -32768)
    full = nonzero(rng, 64, narrow)
    full[[3, 17, 40]] = top, low, lowest
    cat = [
        ("empty", []),
        ("all-zero", [(0, 64)]),
        ("64 symbols", run0(full)),
        ("zeros inside", [(top, 0), (0, 1), (lowest, 0), (0, 2), (low, 0), (0, 1), (9, 3)]),
        ("65 symbols", run0(nonzero(rng, 65, narrow))),
        ("70 symbols", run0(nonzero(rng, 70, narrow))),
        ("100 symbols", run0(nonzero(rng, 100, narrow))),
        ("200 symbols", run0(nonzero(rng, 200, narrow))),
        ("lands at 63", [(7, 63)]),
        ("lands at 62, 63, then dropped", [(5, 62), (6, 0), (7, 0)]),
        ("lands at 5, 63, then dropped", [(1, 5), (2, 57), (3, 0)]),
        ("lands at 64", [(1, 0), (2, 63), (3, 0)]),
    ]
    if path != "lane":
        cat.append(("300 symbols", run0(nonzero(rng, 300, narrow))))
    if narrow:
        cat += [
            ("0x0000 first", [(0, 64), (5, 0), (6, 3)]),
            ("0x0000 in mid-block", [(1, 0), (2, 3), (0, 64), (4, 0), (5, 0)]),
            ("wraps 8 bits", [(1, 0)] + [(0, 64)] * 4 + [(3, 0)]),          # pos 261 = 256 + 5
            ("64 x run 63", [(int(v), 63) for v in nonzero(rng, 64, True)]),  # 4096 steps
            ("64 x 0x0000", [(0, 64)] * 64),
            ("0x200", [(511, 0), (-512, 5), (-511, 0), (-512, 55)]),        # lands at 0, 6, 7, 63
            ("0x200 dropped", [(-512, 10), (-512, 60)]),
        ]
    else:
        cat += [
            ("run 64 first", [(7, 64), (8, 0)]),
            ("run 65 first", [(7, 65), (8, 0), (9, 0)]),
            ("run 1000 first", [(-7, 1000), (8, 2)]),
            ("run 65535 first", [(32767, 65535), (-32768, 0), (3, 0)]),
            ("huge run in mid-block", [(1, 0), (2, 3), (3, 40000), (4, 0), (5, 0)]),
            ("wraps 8 bits", [(1, 0), (2, 255), (3, 0)]),
            ("wraps 16 bits", [(1, 0), (2, 65535), (3, 0)]),
            ("64 x run 65535", [(int(v), 65535) for v in nonzero(rng, 64, False)]),  # 2^22 steps
            ("64 x (-32768, 64)", [(-32768, 64)] * 64),
        ]
    return cat


def filler(rng, n, narrow):
    """n symbols of small runs, now and then a long one, and zero values."""
    out = []
    for _ in range(n):
        long_run = rng.random() < 0.04
        if narrow:
            r = int(rng.integers(40, 64)) if long_run else int(rng.integers(0, 3))
            v = int(rng.integers(-512, 512))
            if v == 0 and r == 0:
                r = 1
        else:
            r = int(rng.integers(64, 65536)) if long_run else int(rng.integers(0, 3))
            v = 0 if rng.random() < 0.05 else int(rng.integers(-32768, 32768))
        out.append((v, r))
    return out


def build_halves(narrow, path, halves, rng):
    """halves: [(blocks, symbols)] of one path.  The catalogue goes largest first into the half with
    the most room, random blocks fill the other slots, and one block per half -- past its end with
    its first symbol -- takes the symbols still missing, which are dropped."""
    room = [n - 1 for _, n in halves]     # one symbol and one slot are the padding block's
    slots = [nb - 1 for nb, _ in halves]
    held = [[] for _ in halves]
    for name, blk in sorted(catalogue(narrow, path, rng), key=lambda e: -len(e[1])):
        fits = [k for k in range(len(halves)) if slots[k] > 0 and room[k] >= len(blk)]
        assert fits, (path, name, "does not fit any half")
        k = max(fits, key=lambda j: (room[j], slots[j]))
        held[k].append(blk)
        room[k] -= len(blk)
        slots[k] -= 1
    size = {"lane": (0, 6), "walk": (0, 40), "quad": (30, 200)}[path]
    out = []
    for k in range(len(halves)):
        sizes = rng.integers(size[0], size[1] + 1, slots[k])
        if sizes.sum() > room[k]:
            sizes = sizes * room[k] // sizes.sum()
        blocks = held[k] + [filler(rng, int(n), narrow) for n in sizes]
        pad = room[k] - int(sizes.sum())
        blocks.append([(0, 64) if narrow else (1, 70)] + filler(rng, pad, narrow))
        order = rng.permutation(len(blocks))
        out.append([blocks[i] for i in order])
        assert len(out[-1]) == halves[k][0] and sum(len(b) for b in out[-1]) == halves[k][1]
    return out


def units_of(blocks):
    """2-byte symbols: (run & 63) << 10 | (value & 0x3FF), (0, 64) = 0x0000."""
    out = []
    for b in blocks:
        for v, r in b:
            assert (v, r) == (0, 64) or (0 <= r <= 63 and -512 <= v <= 511 and (v, r) != (0, 0)), (v, r)
            out.append(((r & 63) << 10) | (v & 0x3FF))
    return np.array(out, np.uint16)


def widen(units):
    """include/dct_amd.h: (run & 63) << 10 | (value & 0x3FF), 0x0000 = (0, 64), the value sign-extended
    from 10 bits -> the 4-byte symbol (uint16)value | run << 16."""
    u = units.astype(np.int64)
    value = u & 0x3FF
    value = np.where(value >= 0x200, value - 0x400, value)
    run = np.where(u == 0, 64, (u >> 10) & 63)
    return ((value & 0xFFFF) | (run << 16)).astype(np.uint32)


def block_features(sym, units):
    """What a block's symbols exercise, from the 4-byte symbols alone (units: the 2-byte form or None)."""
    n = len(sym)
    value = (sym & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    run = (sym >> 16).astype(np.int64)
    pos = np.cumsum(run + 1) - 1            # where each symbol lands (exact: int64)
    read = np.arange(n) < 64                # symbols a count clamp keeps
    f = {
        "no symbols": n == 0,
        "all-zero block": n == 1 and value[0] == 0 and run[0] == 64,
        "more than 64 symbols": n > 64,
        "a run >= 64": bool((run[read] >= 64).any()),
        "nothing lands": n > 1 and run[0] >= 64,
        "dropped after a long run in mid-block": bool((read & (run >= 64) & (np.arange(n) > 0)
                                                      & (np.arange(n) < n - 1)).any()) and pos[0] < 64,
        "a value lands at 63": bool((pos == 63).any()),
        "a value lands at 64": bool((pos[read] == 64).any()),
        "a value past 63": bool((pos[read] > 63).any()),
        "a zero value inside": bool(((value == 0) & (pos < 64) & (np.arange(n) < n - 1)).any()),
        "an 8-bit pos would land a value": bool((read & (pos >= 256) & (pos % 256 < 64)).any()),
        "64 symbols run 0": n == 64 and not run.any(),
    }
    if units is None:
        f["a run of 65535"] = bool((run[read] == 65535).any())
        f["a 16-bit pos would land a value"] = bool((read & (pos >= 65536) & (pos % 65536 < 64)).any())
        f["the steps add up to 2^22"] = n >= 64 and int((run[:64] + 1).sum()) == 1 << 22
        f["32767, -32767, -32768 land"] = all(bool(((value == v) & (pos < 64)).any()) for v in (32767, -32767, -32768))
    else:
        f["0x0000 not last"] = bool((units[:-1] == 0).any())
        f["0x200 lands"] = bool((((units & 0x3FF) == 0x200) & (pos < 64)).any())
        f["run field 63"] = bool(((units >> 10) == 63).any())
        f["the steps add up past 2^12"] = n >= 64 and int((run[:64] + 1).sum()) >= 1 << 12
    return f


@functools.lru_cache(maxsize=None)
def stream(narrow):
    """The ten tiles: dict(blocks, off uint32 [N + 1], sym uint32 [total] (widened by the header's definition),
    units uint16 or None, coef int16 [N, 64], bytes / boff: the packed reference)."""
    rng = np.random.default_rng(20 if narrow else 40)
    pairs = [(a, b) for a in PATHS for b in PATHS]
    plan = []   # (path, blocks, symbols) of every half, in stream order
    seen = {p: 0 for p in PATHS}
    for pair in pairs:
        for p in pair:
            plan.append((p, 32, TARGETS[p][seen[p]]))
            seen[p] += 1
    plan += RAGGED
    assert all(seen[p] == len(TARGETS[p]) for p in PATHS)
    built = {}
    for p in PATHS:
        mine = [(nb, n) for q, nb, n in plan if q == p]
        built[p] = iter(build_halves(narrow, p, mine, rng))
    blocks = [b for p, _, _ in plan for b in next(built[p])]
    nblk = len(blocks)
    assert nblk == 9 * 64 + 37
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    if narrow:
        units = units_of(blocks)
        sym = widen(units)
    else:
        units = None
        sym = np.array([(v & 0xFFFF) | (r << 16) for b in blocks for v, r in b], np.uint32)
    assert off[-1] == sym.size and (np.diff(off.astype(np.int64)) >= 0).all()
    listed = bits_ref.blocks_of(sym, off)
    assert listed == [[(int(v), int(r)) for v, r in b] for b in blocks]  # the widening gives back what was built
    if narrow:
        assert bits_ref.blocks_of(units, off) == listed

    # ---- the layout, from the offsets: every half in its path, every threshold from both sides
    o = off.astype(np.int64)
    halves = []  # (path, first block, end block)
    for h0 in range(0, nblk, 32):
        halves.append((path_of(int(o[min(h0 + 32, nblk)] - o[h0])), h0, min(h0 + 32, nblk)))
    assert [h[0] for h in halves] == [p for p, _, _ in plan]
    assert [(halves[2 * t][0], halves[2 * t + 1][0]) for t in range(9)] == pairs
    counts = {int(o[e] - o[s]) for _, s, e in halves}
    assert {LANE_MAX, LANE_MAX + 1, WALK_MAX, WALK_MAX + 1} <= counts, sorted(counts)
    assert nblk % 64 == 37 and FIRST_PLANE % 32 not in (0, 31)

    # ---- every path holds every feature
    cells = {}
    for p, s, e in halves:
        for b in range(s, e):
            f = block_features(sym[o[b]:o[b + 1]], None if units is None else units[o[b]:o[b + 1]])
            if narrow and o[b + 1] > o[b]:
                f["starts at an odd unit"] = bool(o[b] & 1)
                f["starts at an even unit"] = not o[b] & 1
            for name, has in f.items():
                cells[p, name] = cells.get((p, name), 0) + int(bool(has))
        if narrow:
            for name, has in (("half starts at an odd unit", o[s] & 1), ("half starts at an even unit", not o[s] & 1)):
                cells[p, name] = cells.get((p, name), 0) + int(bool(has))
    empty = sorted(k for k, n in cells.items() if n == 0)
    assert not empty, empty
    assert len(cells) == 3 * (20 if narrow else 16), len(cells)
    sizes = np.diff(o)
    # the sizes the issue names per path
    big = {p: {int(n) for q, s, e in halves if q == p for n in sizes[s:e] if n > 64} for p in PATHS}
    assert 200 in big["lane"] and 300 in big["walk"] and {65, 70, 100, 200} <= big["quad"], big

    # ---- expected results: two references that share nothing agree
    coef = rle_decode_cpu(off, sym)
    data, boff = bits_ref.pack(blocks)
    assert np.array_equal(bits_ref.unpack(data, boff), coef)
    tile_bytes = np.diff(boff.astype(np.int64)[np.r_[0:nblk:64, nblk]])
    for a in (off, sym, coef, data, boff) + (() if units is None else (units,)):
        a.setflags(write=False)
    return dict(blocks=blocks, off=off, sym=sym, units=units, coef=coef, bytes=data, boff=boff, halves=halves,
                tile_bytes=tile_bytes, cells=cells)


def device_symbols(T, s, width):
    """The stream's symbols on the device in the format of `width` bytes; 2-byte units in an
    allocation of whole dwords."""
    if width == 4:
        return gpu(T, s["sym"].view(np.int32))
    assert s["units"] is not None
    n = s["units"].size
    buf = np.full(n + (n & 1), 0x7FFF, np.uint16)
    buf[:n] = s["units"]
    return gpu(T, buf.view(np.int16))[:n]


STREAMS = [pytest.param(False, 4, id="any int16, 4-byte"), pytest.param(True, 4, id="10-bit, 4-byte"),
           pytest.param(True, 2, id="10-bit, 2-byte")]


def plane_shapes(nblk):
    return [(1, 8, 8 * FIRST_PLANE), (1, 8, 8 * (nblk - FIRST_PLANE))]


def test_layout_fills_every_cell():
    """Host only: the assertions inside stream() -- every half in its path, every path x feature cell
    filled, both references agreeing -- and the emit paths the tiles take."""
    for narrow in (False, True):
        s = stream(narrow)
        print(f"{'2-byte' if narrow else '4-byte'}: {s['off'].size - 1} blocks, {s['sym'].size} symbols, "
              f"{s['bytes'].size} B packed; tile bytes {s['tile_bytes'].tolist()}")
        for p in PATHS:
            print("  ", p, {name: n for (q, name), n in s["cells"].items() if q == p})
    s = stream(False)
    sizes = np.diff(s["off"].astype(np.int64))
    over = [bool((sizes[64 * t:64 * t + 64] > 64).any()) for t in range(10)]
    # both emits of bits.hip see blocks of more than 64 symbols in this stream already
    assert any(n > PACK_STAGE and o for n, o in zip(s["tile_bytes"], over))
    assert any(n + 3 <= PACK_STAGE and o for n, o in zip(s["tile_bytes"], over))


@pytest.mark.parametrize("one", GRIDS)
@pytest.mark.parametrize("narrow,width", STREAMS)
def test_coefficients(T, dm, narrow, width, one):
    s = stream(narrow)
    gs, go = device_symbols(T, s, width), gpu(T, s["off"].view(np.int32))
    with workgroups(dm, one) as check:
        got = dm.rle_decode(gs, go).cpu().numpy()
        check()
    bad = np.argwhere((got != s["coef"]).any(axis=1)).ravel()
    assert np.array_equal(got, s["coef"]), (bad[:8].tolist(), [len(s["blocks"][b]) for b in bad[:8]])


@functools.lru_cache(maxsize=None)
def split_host(narrow):
    s = stream(narrow)
    n = s["coef"].shape[0]
    vn = plain_var_num(n)
    return (s["coef"][:FIRST_PLANE], s["coef"][FIRST_PLANE:]), (vn[:FIRST_PLANE], vn[FIRST_PLANE:])


@pytest.mark.parametrize("one", GRIDS)
@pytest.mark.parametrize("narrow,width", STREAMS)
@pytest.mark.parametrize("q,ad", PLANS)
def test_pixels(T, dm, q, ad, narrow, width, one):
    """decode_symbols and decode_bits against decode_planes of the coefficients decoded on the CPU."""
    s = stream(narrow)
    shapes = plane_shapes(s["coef"].shape[0])
    coefs, vns = split_host(narrow)
    gs, go = device_symbols(T, s, width), gpu(T, s["off"].view(np.int32))
    gb, gbo = gpu(T, s["bytes"]), gpu(T, s["boff"].view(np.int32))
    with workgroups(dm, one) as check:
        plan = dm.Plan(q, ad)
        gv = [gpu(T, v) for v in vns] if ad else None
        want = plan.decode_planes([gpu(T, c) for c in coefs], shapes=shapes, var_nums=gv)
        got = plan.decode_symbols(gs, go, shapes=shapes, var_nums=gv)
        check()
        bits = plan.decode_bits(gb, gbo, shapes=shapes, var_nums=gv)
        check()
    for k in range(2):
        assert T.equal(got[k], want[k]), ("decode_symbols", k, int((got[k] != want[k]).sum()))
        assert T.equal(bits[k], want[k]), ("decode_bits", k, int((bits[k] != want[k]).sum()))
    assert int(want[0].max()) > int(want[0].min())  # pixels that depend on the coefficients


def check_pack(T, dm, gs, go, data, boff, coef, check, what):
    got, goff = dm.bits_pack(gs, go)
    check()
    assert np.array_equal(u32(goff), boff), (what, "offsets")
    assert got.dtype == T.uint8 and got.numel() == data.size, (what, got.numel(), data.size)
    assert np.array_equal(got.cpu().numpy(), data), (what, "bytes")
    back = dm.bits_decode(got, goff)
    check()
    assert np.array_equal(back.cpu().numpy(), coef), (what, "bits_decode(bits_pack(S))")
    return got, goff


@pytest.mark.parametrize("one", GRIDS)
@pytest.mark.parametrize("narrow", [False, True], ids=["any int16", "10-bit"])
def test_pack(T, dm, narrow, one):
    s = stream(narrow)
    go = gpu(T, s["off"].view(np.int32))
    with workgroups(dm, one) as check:
        packed = [check_pack(T, dm, device_symbols(T, s, w), go, s["bytes"], s["boff"], s["coef"], check, (narrow, w))
                  for w in ([4, 2] if narrow else [4])]
    if narrow:  # the stream does not depend on the symbol format it was packed from
        assert T.equal(packed[0][0], packed[1][0]) and T.equal(packed[0][1], packed[1][1])


@functools.lru_cache(maxsize=None)
def emit_tiles():
    """Two tiles for the packer's count clamp: bytes past the stage (the lanes store) and below it
    (staged), both with blocks of more than 64 symbols."""
    rng = np.random.default_rng(41)
    dense = [[(-32768, 64)] * 100 for _ in range(23)]                      # 368 B each: 8464 B
    dense += [[(-32768, 64)] * 64 + filler(rng, 30, False), run0(nonzero(rng, 200, False)), [], [(0, 64)]]
    dense += [filler(rng, int(n), False) for n in rng.integers(0, 90, 64 - len(dense))]
    staged = [run0(rng.integers(-3, 4, int(n))) for n in rng.integers(60, 130, 64)]  # about 32 B per block
    staged[5] = [(1, 0)] * 300
    staged[40] = []
    blocks = [dense[i] for i in rng.permutation(64)] + staged
    sym = np.array([(v & 0xFFFF) | (r << 16) for b in blocks for v, r in b], np.uint32)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    data, boff = bits_ref.pack(blocks)
    o = boff.astype(np.int64)
    assert o[64] - o[0] > PACK_STAGE and o[128] - o[64] + 3 <= PACK_STAGE, o[[0, 64, 128]]
    sizes = np.diff(off.astype(np.int64))
    assert (sizes[:64] > 64).sum() >= 25 and (sizes[64:] > 64).sum() >= 20
    coef = rle_decode_cpu(off, sym)
    assert np.array_equal(bits_ref.unpack(data, boff), coef)
    return sym, off, data, boff, coef


@pytest.mark.parametrize("one", GRIDS)
def test_pack_count_clamp_in_both_emits(T, dm, one):
    sym, off, data, boff, coef = emit_tiles()
    gs, go = gpu(T, sym.view(np.int32)), gpu(T, off.view(np.int32))
    with workgroups(dm, one) as check:
        check_pack(T, dm, gs, go, data, boff, coef, check, "emit tiles")
        got = dm.rle_decode(gs, go).cpu().numpy()
        check()
    assert np.array_equal(got, coef)


# ---- Part B: int16 extremes into the coefficient consumers ---------------------------------------
EXTREMES = np.array([-32768, -32767, -1, 1, 32767], np.int16)  # with 0, the six values of the issue


def sparse_blocks(rng, counts, values, last=False):
    """Block i holds counts[i] nonzeros at random places; last False keeps (7,7) zero, so that the
    block has counts[i] + 1 symbols exactly."""
    b = np.zeros((len(counts), 64), np.int16)
    for i, k in enumerate(counts):
        b[i, rng.permutation(64 if last else 63)[:k]] = values(k)
    return b


@functools.lru_cache(maxsize=None)
def rle_tiles():
    """Tiles of 64 blocks, then a ragged one: (coef, oracle offsets, oracle symbols)."""
    import oracle as O
    rng = np.random.default_rng(51)
    ext = lambda k: rng.choice(EXTREMES, k)  # noqa: E731
    uni = lambda k: np.where((v := rng.integers(-32768, 32768, k)) == 0, -32768, v)  # noqa: E731
    tiles = [
        sparse_blocks(rng, [15] * 64, ext),                      # 1024 symbols: lane per block
        sparse_blocks(rng, [31] * 64, ext),                      # 2048: the last tile of that path
        sparse_blocks(rng, [31] * 63 + [32], ext),               # 2049: wave per block
        sparse_blocks(rng, [31] * 64, uni),
        sparse_blocks(rng, [39] * 64, uni),
        sparse_blocks(rng, list(rng.integers(0, 65, 64)), ext, last=True),
        rng.choice(EXTREMES, (64, 64)).astype(np.int16),         # 64 symbols in every block
        rng.integers(-32768, 32768, (64, 64)).astype(np.int16),
        rng.choice(np.r_[EXTREMES, np.int16(0)], (64, 64)).astype(np.int16),
        sparse_blocks(rng, [1] * 64, ext, last=True),
        sparse_blocks(rng, list(rng.integers(0, 65, 29)), uni, last=True),  # ragged
    ]
    coef = np.concatenate(tiles)
    off, sym = O.rle_encode_plane(coef)
    per_tile = np.diff(off.astype(np.int64)[np.r_[0:coef.shape[0]:64, coef.shape[0]]])
    assert {1024, EMIT_LANE_MAX, EMIT_LANE_MAX + 1, 4096} <= set(per_tile.tolist()), per_tile
    assert coef.shape[0] % 64 == 29
    for v in (-32768, -32767, 32767):  # each extreme in a tile of either path
        for dense in (False, True):
            assert any((t == v).any() for t, n in zip(tiles, per_tile) if (n > EMIT_LANE_MAX) == dense), (v, dense)
    assert np.array_equal(rle_decode_cpu(off, sym), coef)  # the oracle accepts these inputs, and losslessly
    return coef, off, sym


def test_rle_encode_int16_extremes(T, dm):
    coef, woff, wsym = rle_tiles()
    g = gpu(T, coef)
    off, sym = dm.rle_encode(g)
    assert np.array_equal(u32(off), woff)
    assert np.array_equal(u32(sym), wsym)
    assert T.equal(dm.rle_decode(sym, off), g)
    packed, boff = dm.bits_pack(sym, off)
    assert T.equal(dm.bits_decode(packed, boff), g)


def few_values(rng, pool, n):
    """n coefficients drawn from two to five values of pool: leaf weights repeat and tie."""
    return rng.choice(rng.choice(pool, int(rng.integers(2, 6)), replace=False), n)


@functools.lru_cache(maxsize=None)
def huffman_tiles():
    """One tile per path of classify (huffman.hip), each checked here for the conditions of its path."""
    import oracle as O
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "huffman.json")))["blocks"]["int16_range"]
    assert sorted(set(g["coeffs"])) == [-32768, 32767]
    assert O.huffman_bits_plane(np.array([g["coeffs"]], np.int16)).tolist() == [g["bits"]]  # the compiled reference's
    rng = np.random.default_rng(61)
    tiles = {}
    # counting path: a dense tile whose every block spans fewer than 64 integers -- at both ends of int16
    # (no zeros), and around zero with vmin = -63 (the zero counter is the window's last)
    tiles["narrow top"] = np.stack([few_values(rng, np.arange(32705, 32768), 64) for _ in range(64)])
    tiles["narrow bottom"] = np.stack([few_values(rng, np.arange(-32768, -32705), 64) for _ in range(64)])
    tiles["narrow top"][0] = np.arange(32705, 32768)[rng.integers(0, 63, 64)]
    tiles["narrow top"][1, :2] = 32705, 32767
    tiles["narrow bottom"][1, :2] = -32768, -32706
    zero = np.stack([few_values(rng, np.arange(-63, 0), 64) * (rng.random(64) < 0.8) for _ in range(64)])
    zero[:, 5] = -63
    zero[::2, 63] = 0
    zero[1::2, 63] = -1
    tiles["narrow around zero"] = zero
    for name in ("narrow top", "narrow bottom", "narrow around zero"):
        t = tiles[name].astype(np.int64)
        assert (t.max(axis=1) - t.min(axis=1) <= 63).all() and (np.count_nonzero(t[:, :16], axis=1) > 7).any(), name
    assert not (tiles["narrow top"] == 0).any() and not (tiles["narrow bottom"] == 0).any()
    assert tiles["narrow top"].max() == 32767 and tiles["narrow bottom"].min() == -32768
    assert (zero.min(axis=1) == -63).all() and (zero[:, :63] == 0).any()
    # sort paths: at most 16 / at most 32 nonzeros in every block, (7,7) zero and not; denser blocks
    for name, lo, hi in (("sort 16", 0, 16), ("sort 32", 10, 32), ("sort 64", 33, 64)):
        t = np.zeros((64, 64), np.int64)
        for r in range(64):
            k = int(rng.integers(lo, hi))
            t[r, rng.choice(63, k, replace=False)] = few_values(rng, EXTREMES, k)
        t[2::2, 63] = rng.choice(EXTREMES, 31)  # (7,7) zero in the odd blocks, an extreme in the even ones
        t[0] = 0
        t[0, :hi] = np.resize(EXTREMES, hi)     # the densest block the path takes, every extreme in it
        if name == "sort 64":
            t[1:, 1], t[1:, 2] = -32768, 32767
        nz = np.count_nonzero(t, axis=1)
        assert nz.max() == hi and (nz[1:] >= lo).all(), name
        tiles[name] = t
    assert (tiles["sort 64"].max(axis=1) - tiles["sort 64"].min(axis=1) >= 64).all()
    tiles["uniform"] = rng.integers(-32768, 32768, (64, 64))
    tiles["six values"] = rng.choice(np.r_[EXTREMES.astype(np.int64), 0], (64, 64))
    tiles["ragged"] = np.concatenate([tiles["sort 64"][:20], tiles["narrow bottom"][:17]])
    coef = np.concatenate(list(tiles.values())).astype(np.int16)
    assert coef.shape[0] % 64 == 37
    return coef, O.huffman_bits_plane(coef), list(tiles)


def test_huffman_bits_int16_extremes(T, dm):
    coef, want, names = huffman_tiles()
    got = u32(dm.huffman_bits(gpu(T, coef)))
    bad = np.argwhere(got != want).ravel()
    assert np.array_equal(got, want), [(names[b // 64], int(b % 64), int(got[b]), int(want[b])) for b in bad[:8]]
