"""GPU: address arithmetic past 2 GiB and 4 GiB -- byte offsets inside image planes, uint32
symbol / byte offsets inside streams, and the running totals of the three scans.

Everything wide lives inside ONE uint8 device tensor of 8 GiB + 64 MiB (`big`; the module
skips when the device has less than that plus 4 GiB free).  Compact copies, stream offsets and
the outputs of calls whose *input* is the wide side are ordinary small allocations.  A case is
laid out so that the two likely wrong addresses -- the correct offset truncated to 32 bits, and
its low 32 bits sign-extended -- fall inside the allocation, hold OTHER random bytes (readers:
asserted on the device's own contents before the call, block by block) or the sentinel
(writers: the whole allocation is swept afterwards), so that a bug fails an assertion.

Expected values come from the CPU oracle, tools/bits_ref.py, tools/color_ref.py,
tools/frame_ref.py, tools/scaled_ref.py, tools/window_ref.py, tools/extract_ref.py, or from the
same library call on a compact copy of the same data (the path the rest of the suite pins to
the oracle); never from the call under test.  Every comparison is byte equality.

1. Planes (every entry point that takes a dctq_plane), strided views that start 2 GiB (+ 1 MiB
   per geometry) into `big`:
     a  2 frames, frame 1 past 2 GiB (span < 4 GiB: descriptor path, offsets with bit 31 set)
     b  2 frames, frame 1 past 4 GiB (span == 0: 64-bit pointer path)
     c  1 frame, the row stride carries block rows 5.. past 2 GiB (block row 5 straddles)
     d  1 frame, the row stride carries block rows 4.. past 2 GiB and 8.. past 4 GiB (block row
        8 straddles the 2^32 line: seven rows below, one above)
   readers  forward_quant (+ oracle), forward_float, round_trip_planes, encode_planes (4- and
            2-byte), huffman_bits_planes, distortion_planes; one mixed four-plane launch
            (compact, a, b, d) of every *_planes entry point
   writers  decode_planes, decode_symbols (4- and 2-byte), decode_bits, the mixed launch, and
            dctq_synth into b and d
   windows  Plan.decode_bits_window into a-d and the mixed launch: the stored planes are larger
            than the window in every dimension (three frames with the window on frames 1..,
            a block origin away from 0 in rows and columns, var_nums of the whole stored
            plane), so the window's first block, its var_num index and a run's distance from
            it are all non-zero; expected: the slice of Plan.decode_bits into compact planes
   scaled   Plan.decode_bits_scaled at 1/2, 1/4 and 1/8 into a-d and the mixed launch: the
            REDUCED picture is the geometry, so a window row is 18, 36 or 72 blocks (at 1/8 a
            run of 64 and one of 8).  decode_scaled.hip has a store tail of its own: a and c
            take its descriptor path with bit 31 set in the offset, b and d its 64-bit path,
            the mixed launch both in one grid.  In c the 2^31 line and in d the 2^32 line
            fall between the two pixel rows one lane stores (n = 4), between the two
            half-waves (n = 2) and between two block rows (n = 1).  Plans q100 and adaptive
            q50 over blocks of random levels plus noise: the expected picture (scaled_ref on
            the coefficients bits_decode returns) spans more than 64 levels at every scale
   colour   rgb_to_ycbcr / ycbcr_to_rgb, 4:2:0 and 4:4:4, interleaved and planar, picture and
            planes both wide ("frames": like b, Cb like a; "rows": like d)
   Both aliases of every byte of these cases lie inside the allocation.
2. Stream consumers (rle_decode, bits_decode, Plan.decode_symbols, Plan.decode_bits, bits_pack
   reading symbols, block_lengths) with offsets base + cumsum:
     4-byte symbols  base 2^30 - k (the byte offset crosses 2^32), 2^31 - k (the index crosses
                     bit 31)
     2-byte symbols  base 2^31 - k, and 2^32 - total - 1 / - 2
     packed bytes    base 2^31 - k, and 2^32 - total - 1 / - 2
   k puts the crossing inside block 101 (tile 1, second half); two k of different parity.
   Aliases that LEAVE the allocation (a bug of that kind could fault instead of failing):
   only the sign-extended 4-byte symbol INDEX at base 2^31 - k (8 GiB below the base pointer).
   The issue's "2^32 - total" for packed bytes puts the END offset at 2^32, which a uint32
   holds as 0 -- a decreasing offset, outside the format (include/dct_amd.h: non-decreasing
   offsets).  The top-of-range byte stream here ends at 2^32 - 1 (and 2^32 - 2).
   At the four packed-byte placements also the consumers that take windows,
   Plan.decode_bits_window, Plan.decode_bits_scaled (2, 4, 8) and bits_window (against
   tools/extract_ref.py on the host stream: bytes, offsets and var_nums), over two window sets:
   one with block 101 inside a run of 64 and not as its first block, so the run's first offset
   is below the crossing and its end above it, and one whose runs all start above it.  The
   second numbers the same 279 blocks as ONE plane 2 232 pixels wide (the two planes side by
   side; expected pictures and var_nums concatenated): over the two planes themselves every
   window set has a run in plane 0, all of whose blocks lie below the crossing.
3. Stream producers whose totals pass 2^31: dctq_rle_count over ~37 M blocks (4.4 GiB of
   coefficients in `big`), bits_pack over ~8.3 M blocks (offsets only, capacity one byte short
   of a tile boundary past 2^31, the whole stream; then bits_decode and Plan.decode_bits on
   that stream), block_offsets / block_lengths at the API's maximum of 11 671 106 blocks.
   The packed stream is written 4 GiB into `big`: a sign-extended offset lands 2 GiB below,
   in sentinel bytes that are swept.
   dctq_bits_window_offsets / dctq_bits_window_gather on a window whose OWN payload passes
   2^31: a stream of 7 981 frames of one block row of 1 021 blocks (8.1 M blocks, 2 GiB + 2.3
   MiB, tiled from a palette and not packed) and the window of its frames 1.., which drops
   under 300 KB.  Source (2 GiB + 16 MiB into `big`) and destination (6 GiB + 32 MiB) both
   have offsets with bit 31 set; the sign-extended alias of every such source offset holds
   other bytes, that of every destination offset sentinel behind the source's end.  Offsets
   and var_nums against the source's own, the payload against the source's suffix, a capacity
   one byte short of a run boundary past 2^31, sweeps around both, the source unchanged; then
   the window decoder on the last two frames of both streams and the scaled decoder on the
   source's, against a compact copy's decode_bits and scaled_ref on the palette's coefficients.

Left out, known: rle_emit / encode_planes WRITING symbols past index 2^31 (the symbol buffer
alone would take 4-9 GiB on top of 4.6 GiB of coefficients).  A window total or a gather
destination past 2^32 (outside the format: offsets are uint32).  The window consumers of 2.
with a run in which bit 31 is set in every offset of plane 0 at base 2^31 - k (see there), and
frame_window / frame_concat / decompress(region=, scale=) past 2 GiB: they are Python over the
entry points above and torch copies, and a container of that size needs 4 GiB more."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bits_ref  # noqa: E402
import color_ref  # noqa: E402
import extract_ref  # noqa: E402
import frame_ref  # noqa: E402
import scaled_ref  # noqa: E402
import window_ref  # noqa: E402

MiB, GiB = 1 << 20, 1 << 30
L30, L31, L32, M32 = 1 << 30, 1 << 31, 1 << 32, (1 << 32) - 1
BIG = 8 * GiB + 64 * MiB
ROOM = 4 * GiB
CHUNK = 256 * MiB
SENT = 0xA5
SENT64 = int.from_bytes(bytes([SENT]) * 8, "little", signed=True)
PLANS = [(50, 0), (75, 0), (90, 1)]  # fp32 inverse; fp64 inverse; adaptive
MAX_BLOCKS = 11_671_106

_state = {"readers": None}  # what test_plane_readers laid out in `big`, while nothing overwrote it


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


@pytest.fixture(scope="module")
def big(T):
    free, _ = T.cuda.mem_get_info()
    if free < BIG + ROOM:
        pytest.skip(f"{free} B of device memory free, {BIG + ROOM} B needed ({BIG} B in one tensor + {ROOM} B of room)")
    t0 = time.time()
    buf = T.empty(BIG, dtype=T.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    yield buf
    T.cuda.synchronize()
    print(f"\ntest_wide_offsets_gpu: {time.time() - t0:.1f} s with the {BIG} B tensor alive")
    _state["readers"] = None
    del buf
    T.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def plan_of(q, ad):
    import dct_amd
    return dct_amd.Plan(q, ad)


@functools.lru_cache(maxsize=None)
def table(q, ad):
    """The plan's quantization table, as tools/scaled_ref.py takes it."""
    import dct_amd
    return dct_amd.debug_tables(q, ad)[3].reshape(8, 8)


def gpu(T, a):
    return T.from_numpy(np.array(a)).cuda()  # a copy: cached host arrays are read-only


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def sext32(x):
    x = x & M32
    return np.where(x >= L31, x - L32, x)


def widths_of(plan):
    return [4, 2] if plan.symbol_bytes == 2 else [4]


# ---- 0. the big tensor: sentinel, sweep, scattered writes and reads ---------------------------------
def fill_sentinel(big, lo=0, hi=BIG):
    for a in range(lo, hi, CHUNK):
        big[a:min(a + CHUNK, hi)].fill_(SENT)


def first_dirty(T, big, lo=0, hi=BIG):
    """The address of the first byte of big[lo:hi) that is not the sentinel, or None; on the
    device, 256 MiB at a time."""
    lo8, hi8 = min(-(-lo // 8) * 8, hi), max(hi // 8 * 8, lo)
    spans = [(lo, lo8), (hi8, hi)] if lo8 <= hi8 else [(lo, hi)]
    flags = [(a, b, (big[a:b] != SENT).any()) for a, b in spans if b > a]
    if lo8 < hi8:
        flags += [(a, min(a + CHUNK, hi8), (big[a:min(a + CHUNK, hi8)].view(T.int64) != SENT64).any())
                  for a in range(lo8, hi8, CHUNK)]
    if not flags:
        return None
    bad = T.stack([f for _, _, f in flags]).cpu().numpy()
    for (a, b, _), f in sorted(zip(flags, bad), key=lambda x: x[0][0]):
        if f:
            return a + int((big[a:b] != SENT).nonzero()[0])
    return None


def test_sweep_sees_a_single_byte(T, big):
    _state["readers"] = None
    fill_sentinel(big)
    assert first_dirty(T, big) is None
    for at in (0, 2 * GiB - 1, 5 * GiB + 3, BIG - 1):
        big[at] = SENT ^ 1
        assert first_dirty(T, big) == at and first_dirty(T, big, at, at + 1) == at
        assert first_dirty(T, big, at + 1, BIG) is None and first_dirty(T, big, 0, at) is None
        big[at] = SENT


def runs_of(addr):
    """addr int64 [n] -> [(j0, j1, addr[j0])]: the maximal runs of consecutive addresses."""
    cut = np.flatnonzero(np.diff(addr) != 1) + 1
    j0, j1 = np.concatenate([[0], cut]), np.concatenate([cut, [addr.size]])
    return [(int(a), int(b), int(addr[a])) for a, b in zip(j0, j1)]


def write(T, big, addr, data):
    """big[addr[j]] = data[j] (u8), run by run."""
    dev = gpu(T, data) if isinstance(data, np.ndarray) else data
    for j0, j1, a in runs_of(addr):
        assert 0 <= a and a + j1 - j0 <= BIG, (a, j1 - j0)
        big[a:a + j1 - j0].copy_(dev[j0:j1])


def erase(T, big, addr):
    for j0, j1, a in runs_of(addr):
        big[a:a + j1 - j0].fill_(SENT)


def read(T, big, addr):
    return T.cat([big[a:a + j1 - j0] for j0, j1, a in runs_of(addr)])


def lay(T, big, items, seed, what):
    """items: dicts with true (int64 address of every byte), data (u8), aliases {name: int64
    addresses}, unit_of (the block of every byte).  Writes other random bytes at every alias that
    differs from the true address and lies inside `big`, then the data, reads both back and
    asserts: the data is there, and every block differs from the bytes at its aliased address.
    Returns {name: number of blocks whose alias leaves the allocation}."""
    rng = np.random.default_rng(seed)
    sel = []
    for it in items:
        other = rng.integers(0, 256, it["data"].size, dtype=np.uint8)
        for name, al in it["aliases"].items():
            differs, inside = al != it["true"], (al >= 0) & (al < BIG)
            idx = np.flatnonzero(differs & inside)
            sel.append((it, name, idx, np.unique(it["unit_of"][differs & ~inside]).size))
            if idx.size:
                write(T, big, al[idx], other[idx])
    for it in items:
        write(T, big, it["true"], it["data"])
    outside = {}
    for it in items:
        assert np.array_equal(read(T, big, it["true"]).cpu().numpy(), it["data"]), (what, "layouts overlap")
    for it, name, idx, out in sel:
        outside[name] = outside.get(name, 0) + out
        if idx.size == 0:
            continue
        there = read(T, big, it["aliases"][name][idx]).cpu().numpy()
        units = it["unit_of"][idx]
        n = int(it["unit_of"].max()) + 1
        diff = np.bincount(units, weights=there != it["data"][idx], minlength=n)
        has = np.bincount(units, minlength=n) > 0
        assert (diff[has] > 0).all(), (what, name, "a block equals the bytes at its aliased address",
                                       np.flatnonzero(has & (diff == 0))[:8])
    return outside


# ---- 1. planes ----------------------------------------------------------------------------------------
GEOS = {
    "a": dict(start=2 * GiB, F=2, H=64, W=72, S=88, FS=L31 + 4104),
    "b": dict(start=2 * GiB + MiB, F=2, H=64, W=72, S=88, FS=L32 + 4104),
    "c": dict(start=2 * GiB + 2 * MiB, F=1, H=64, W=72, S=48258064, FS=64 * 48258064),
    "d": dict(start=2 * GiB + 3 * MiB, F=1, H=80, W=72, S=60921664, FS=80 * 60921664),
}


def plane_item(g, data):
    """The layout item of a u8 plane stack data [F, H, W] at geometry g (start, S, FS)."""
    F, H, W = data.shape
    f, r, x = np.meshgrid(np.arange(F, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64),
                          indexing="ij")
    off = (f * g["FS"] + r * g["S"] + x).ravel()
    return dict(true=g["start"] + off, data=data.ravel(),
                aliases={"truncated": g["start"] + (off & M32), "sign-extended": g["start"] + sext32(off)},
                unit_of=((f * (H // 8) + r // 8) * (W // 8) + x // 8).ravel(), off=off)


def plane_view(big, g, shape=None):
    F, H, W = shape or (g["F"], g["H"], g["W"])
    return big.as_strided((F, H, W), (g["FS"], g["S"], 1), g["start"])


@functools.lru_cache(maxsize=None)
def geo_pixels(name):
    g = GEOS[name]
    px = np.random.default_rng(100 + ord(name)).integers(0, 256, (g["F"], g["H"], g["W"]), dtype=np.uint8)
    px.setflags(write=False)
    return px


LINES = {"a": [L31], "b": [L31, L32], "c": [L31], "d": [L31, L32]}  # the lines a geometry's pixels lie on both sides of


def rows_around(g, line):
    """(the last pixel row of frame 0 that ends below `line`, the first that starts at or past it)."""
    first = np.arange(g["H"], dtype=np.int64) * g["S"]
    return int(np.flatnonzero(first + g["W"] - 1 < line).max()), int(np.flatnonzero(first >= line).min())


def test_geometries_are_what_the_cases_need():
    for name, g in GEOS.items():
        F, H, W, S, FS = g["F"], g["H"], g["W"], g["S"], g["FS"]
        assert W % 8 == 0 and W >= 72 and (W // 8) & (W // 8 - 1) and (F * (H // 8) * (W // 8)) % 64
        assert S % 8 == 0 and S & (S - 1) and FS % 8 == 0 and FS & (FS - 1) and g["start"] % 8 == 0
        span = (F - 1) * FS + (H - 1) * S + W
        assert g["start"] + span <= BIG and span < 4.5 * GiB
        first = np.array([f * FS + by * 8 * S for f in range(F) for by in range(H // 8)])  # each block row
        last = first + 7 * S + W - 1
        for line in LINES[name]:
            assert (last < line).any() and (first >= line).any(), (name, line)
        assert (span < M32) == (name in "ac") and span > L31
        if name == "d":
            assert ((first < L32) & (first + 7 * S >= L32)).any(), "no block straddles the 2^32 line"
        # no alias of any byte leaves the allocation: the aliases depend on F, H, W, S and FS only, so this
        # holds for every writer into these views, the window and the scaled decoder included
        it = plane_item(g, geo_pixels(name))
        for al in it["aliases"].values():
            assert int(al.min()) >= 0 and int(al.max()) < BIG, name
        # the scaled decoder writes n = 8 / scale pixel rows a block row, whatever n: single pixel rows
        # (the unit of n = 1) lie on both sides of every line
        row = np.array([f * FS + r * S for f in range(F) for r in range(H)])
        for line in LINES[name]:
            assert (row + W - 1 < line).any() and (row >= line).any(), (name, line)
    # where the lines fall among the n-row block rows of the scaled decoder (decode_scaled.hip: lane
    # (hh, j) stores rows 2 hh and 2 hh + 1 of its block for n = 4, row hh for n = 2)
    for name, line, pair in (("c", L31, (44, 45)), ("d", L32, (70, 71))):
        lo, hi = rows_around(GEOS[name], line)
        assert (lo, hi) == pair, (name, lo, hi)
        assert lo // 4 == hi // 4 and (lo % 4) // 2 == (hi % 4) // 2 and hi % 2 == 1  # n = 4: one lane's two rows
        assert lo // 2 == hi // 2 and (lo % 2, hi % 2) == (0, 1)                      # n = 2: across the half-waves
        assert lo > 0 and hi < GEOS[name]["H"] - 1                                    # n = 1: rows on both sides
    assert rows_around(GEOS["d"], L31) == (35, 36)  # between two block rows for n = 4 and n = 2


def readers_layout(T, big):
    """All four geometries in `big` at once, with their aliases: {name: (view, compact)}."""
    if _state["readers"] is None:
        items = [plane_item(GEOS[n], geo_pixels(n)) for n in GEOS]
        outside = lay(T, big, items, 1, "planes a-d")
        assert not any(outside.values()), outside
        _state["readers"] = {n: (plane_view(big, GEOS[n]), gpu(T, geo_pixels(n))) for n in GEOS}
    return _state["readers"]


def nblocks(p):
    f, h, w = (1, *p.shape) if p.dim() == 2 else p.shape
    return f * (h // 8) * (w // 8)


def run_reader(T, plan, name, planes):
    """The entry point `name` on the planes (one launch where the entry point takes several)."""
    nbs = [nblocks(p) for p in planes]
    vns = [T.full((nb,), -1, dtype=T.int32, device="cuda") for nb in nbs]
    if name == "forward_quant":
        if len(planes) == 1:
            return [plan.forward_quant(planes[0], var_num=vns[0])] + vns
        return plan.forward_quant_planes(planes, var_nums=vns) + vns
    if name == "forward_float":
        return [plan.forward_float(p) for p in planes]
    if name == "round_trip_planes":
        coefs, recons = plan.round_trip_planes(planes, var_nums=vns)
        return coefs + recons + vns
    if name == "encode_planes":
        out = []
        for sb in widths_of(plan):
            coefs, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
            out += coefs + [off, sym]
        return out
    if name == "huffman_bits_planes":
        return [plan.huffman_bits_planes(planes)]
    assert name == "distortion_planes"
    return [plan.distortion_planes(planes)]


READERS = ["forward_quant", "forward_float", "round_trip_planes", "encode_planes", "huffman_bits_planes",
           "distortion_planes"]


def assert_same(T, got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        same = T.equal(g.view(T.uint8) if g.dtype == T.float32 else g, w.view(T.uint8) if w.dtype == T.float32 else w)
        assert same, (what, "output", k, int((g != w).sum()), "elements differ")


@functools.lru_cache(maxsize=None)
def oracle_forward(name, q, ad):
    import oracle as O
    px = geo_pixels(name)
    coef = np.concatenate([O.forward_plane(p, q, ad) for p in px])
    vn = np.concatenate([O.plane_variance(p) for p in px]) * 4096.0
    assert np.array_equal(vn, np.round(vn))
    return coef, vn.astype(np.int32)


@pytest.mark.parametrize("q,ad", PLANS)
@pytest.mark.parametrize("entry", READERS)
@pytest.mark.parametrize("geo", list(GEOS))
def test_plane_readers(T, dm, big, geo, entry, q, ad):
    view, compact = readers_layout(T, big)[geo]
    plan = plan_of(q, ad)
    d = dm.plane_desc(view)
    assert (d.stride, d.nframes) == (GEOS[geo]["S"], GEOS[geo]["F"]) and (d.nframes == 1 or d.frame_stride == GEOS[geo]["FS"])
    want = run_reader(T, plan, entry, [compact])
    got = run_reader(T, plan, entry, [view])
    assert_same(T, got, want, (geo, entry, q, ad))
    if entry == "forward_quant":
        coef, vn = oracle_forward(geo, q, ad)
        assert np.array_equal(got[0].cpu().numpy(), coef), (geo, q, ad, "forward_quant != the oracle's forward")
        assert np.array_equal(got[1].cpu().numpy(), vn), (geo, q, ad, "var_num != the oracle's variance")


MIXED = ["c", "a", "b", "d"]  # plane 0 is the compact copy of c


@pytest.mark.parametrize("q,ad", PLANS)
@pytest.mark.parametrize("entry", [e for e in READERS if e != "forward_float"])
def test_plane_readers_mixed_launch(T, dm, big, entry, q, ad):
    lay_ = readers_layout(T, big)
    plan = plan_of(q, ad)
    compact = [lay_[n][1] for n in MIXED]
    planes = [compact[0]] + [lay_[n][0] for n in MIXED[1:]]
    assert_same(T, run_reader(T, plan, entry, planes), run_reader(T, plan, entry, compact), ("mixed", entry, q, ad))


@functools.lru_cache(maxsize=None)
def writer_inputs(names, q, ad):
    """What the decoders read, made on the compact path: {"coefs", "vns", 4: (sym, off), 2: ..,
    "bits": (bytes, offsets)} for the planes `names` in one call."""
    import torch as T
    import dct_amd as dm
    plan = plan_of(q, ad)
    compact = [gpu(T, geo_pixels(n)) for n in names]
    vns = [T.zeros(nblocks(p), dtype=T.int32, device="cuda") for p in compact]
    inp = {"coefs": plan.forward_quant_planes(compact, var_nums=vns), "vns": vns if ad else None}
    for sb in widths_of(plan):
        _, off, sym = plan.encode_planes(compact, symbol_bytes=sb)
        inp[sb] = (sym, off)
    inp["bits"] = dm.bits_pack(*inp[4])
    return inp


def run_writer(plan, name, inp, **where):
    """[(label, pixels)] of the writer `name`, into where = shapes=... or outs=..."""
    if name == "decode_planes":
        return [(name, plan.decode_planes(inp["coefs"], var_nums=inp["vns"], **where))]
    if name == "decode_bits":
        return [(name, plan.decode_bits(*inp["bits"], var_nums=inp["vns"], **where))]
    assert name == "decode_symbols"
    return [(f"{name} {sb}-byte", plan.decode_symbols(*inp[sb], var_nums=inp["vns"], **where)) for sb in widths_of(plan)]


WRITERS = ["decode_planes", "decode_symbols", "decode_bits"]


def check_written(T, big, items, wants, what):
    """The wide destinations hold `wants`; then, with them erased, the whole tensor is sentinel."""
    for k, (it, want) in enumerate(zip(items, wants)):
        got = read(T, big, it["true"])
        assert T.equal(got, want.reshape(-1)), (what, "plane", k, int((got != want.reshape(-1)).sum()), "bytes differ")
        erase(T, big, it["true"])
    at = first_dirty(T, big)
    assert at is None, (what, f"a store landed at byte {at} of the allocation, outside the destination")


@pytest.mark.parametrize("q,ad", PLANS)
@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("geo", list(GEOS) + ["mixed"])
def test_plane_writers(T, dm, big, geo, writer, q, ad):
    names = tuple(MIXED) if geo == "mixed" else (geo,)
    plan = plan_of(q, ad)
    inp = writer_inputs(names, q, ad)
    shapes = [geo_pixels(n).shape for n in names]
    wide = [n for n in names if not (geo == "mixed" and n == MIXED[0])]
    items = [plane_item(GEOS[n], geo_pixels(n)) for n in wide]
    _state["readers"] = None
    fill_sentinel(big)
    for pos, (label, want) in enumerate(run_writer(plan, writer, inp, shapes=shapes)):
        assert all(T.equal(a, b) for a, b in zip(want, plan.decode_planes(inp["coefs"], shapes=shapes, var_nums=inp["vns"])))
        outs = [plane_view(big, GEOS[n]) for n in names]
        if geo == "mixed":
            outs[0] = T.full(shapes[0], SENT, dtype=T.uint8, device="cuda")
        got = run_writer(plan, writer, inp, outs=outs)[pos][1]
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
        if geo == "mixed":
            assert T.equal(outs[0], want[0]), (geo, label, q, ad, "the compact plane")
        check_written(T, big, items, want[len(names) - len(wide):], (geo, label, q, ad))


# ---- windows of a stream into wide planes: the window decoder and the scaled decoder -------------------
def stored_geometry(name, scale=1):
    """(stored shape, window) of a stream whose window fills geometry `name` at 1 / scale: the
    window's extent is (F, H scale, W scale); the stored plane has three frames with the window
    on frames 1.., one block row above and below it, two block columns left and one right of it."""
    g = GEOS[name]
    h, w = g["H"] * scale, g["W"] * scale
    return (3, h + 16, w + 24), ((1, 1 + g["F"]), (8, 8 + h), (16, 16 + w))


@functools.lru_cache(maxsize=None)
def levels_and_noise(shape, seed):
    """u8 pixels [F, H, W]: every 8 x 8 block has a level of its own in 24..231, plus noise of up to
    24 either way, so a reduced picture spans the range at every scale (at 1/8 it is the levels)."""
    rng = np.random.default_rng(seed)
    f, h, w = shape
    level = rng.integers(24, 232, (f, h // 8, w // 8)).repeat(8, 1).repeat(8, 2)
    px = (level + rng.integers(-24, 25, shape)).astype(np.uint8)
    px.setflags(write=False)
    return px


def window_inputs(T, names, scale, q, ad):
    """The packed stream of the stored planes around the windows of `names`, made on the compact
    path: (bytes, offsets, var_nums or None, stored shapes, windows)."""
    plan = plan_of(q, ad)
    geo = [stored_geometry(n, scale) for n in names]
    shapes, windows = [s for s, _ in geo], [w for _, w in geo]
    for (f, h, w), ((f0, f1), (y0, y1), (x0, x1)) in zip(shapes, windows):  # first, var_first and rel are non-trivial
        assert 0 < f0 < f1 <= f and 0 < y0 < y1 < h and 0 < x0 < x1 < w
    planes = [gpu(T, levels_and_noise(s, 40 + k)) for k, s in enumerate(shapes)]
    vns = [T.zeros(nblocks(p), dtype=T.int32, device="cuda") for p in planes]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, boff, by = plan.encode_bits_planes(planes)
    return by, boff, (vns if ad else None), shapes, windows


def wide_outs(T, big, names, mixed):
    """(outs, items of the wide ones): the views of `names` in `big`; mixed: plane 0 is compact."""
    outs = [plane_view(big, GEOS[n]) for n in names]
    if mixed:
        outs[0] = T.full(geo_pixels(names[0]).shape, SENT, dtype=T.uint8, device="cuda")
    return outs, [plane_item(GEOS[n], geo_pixels(n)) for n in names[1 if mixed else 0:]]


@pytest.mark.parametrize("q,ad", PLANS)
@pytest.mark.parametrize("geo", list(GEOS) + ["mixed"])
def test_window_decoder_into_wide_planes(T, dm, big, geo, q, ad):
    """Plan.decode_bits_window into a-d and the mixed launch: the slice of Plan.decode_bits of the same
    stream into compact full planes, and not a byte anywhere else in the allocation."""
    mixed = geo == "mixed"
    names = tuple(MIXED) if mixed else (geo,)
    plan = plan_of(q, ad)
    by, boff, vns, shapes, windows = window_inputs(T, names, 1, q, ad)
    full = plan.decode_bits(by, boff, shapes=shapes, var_nums=vns)
    want = [p[f0:f1, y0:y1, x0:x1].contiguous() for p, ((f0, f1), (y0, y1), (x0, x1)) in zip(full, windows)]
    _state["readers"] = None
    fill_sentinel(big)
    outs, items = wide_outs(T, big, names, mixed)
    got = plan.decode_bits_window(by, boff, shapes, windows, outs=outs, var_nums=vns)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    if mixed:
        assert T.equal(outs[0], want[0]), (geo, q, ad, "the compact plane")
    check_written(T, big, items, want[len(names) - len(items):], ("decode_bits_window", geo, q, ad))


SCALED_PLANS = [(100, 0), (50, 1)]  # the plans whose pictures show where a block landed (tests/test_window_gpu.py)


@pytest.mark.parametrize("q,ad", SCALED_PLANS)
@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("geo", list(GEOS) + ["mixed"])
def test_scaled_decoder_into_wide_planes(T, dm, big, geo, scale, q, ad):
    """Plan.decode_bits_scaled into a-d and the mixed launch, whose reduced pictures are the geometries:
    tools/scaled_ref.py on the coefficients bits_decode returns, cut to the windows.  a and c take the
    descriptor path (offsets with bit 31 set), b and d the 64-bit path, the mixed launch both."""
    mixed = geo == "mixed"
    names = tuple(MIXED) if mixed else (geo,)
    plan = plan_of(q, ad)
    by, boff, vns, shapes, windows = window_inputs(T, names, scale, q, ad)
    nbs = sorted(set(window_ref.runs(shapes, windows)[:, 1].tolist()))
    assert nbs == {2: [18], 4: [36], 8: [8, 64]}[scale], nbs
    coef = dm.bits_decode(by, boff).cpu().numpy()
    host_vns = [v.cpu().numpy() for v in vns] if ad else None
    want = scaled_ref.planes(coef, shapes, table(q, ad), scale, ad, host_vns, windows)
    spans = [int(p.max()) - int(p.min()) for p in want]
    assert min(spans) > 64, (geo, scale, q, ad, spans)  # a misplaced block shows
    _state["readers"] = None
    fill_sentinel(big)
    outs, items = wide_outs(T, big, names, mixed)
    for n, o, it in zip(names[len(names) - len(items):], outs[len(names) - len(items):], items):
        d = dm.plane_desc(o)
        span = (d.nframes - 1) * d.frame_stride + (d.height - 1) * d.stride + d.width
        assert (span < M32) == (n in "ac") and span == int(it["off"].max()) + 1, (n, span)
        for line in LINES[n]:  # pixel rows on both sides of every line the geometry is meant to cross
            assert (it["off"] < line).any() and (it["off"] >= line).any(), (n, line)
    got = plan.decode_bits_scaled(by, boff, shapes, scale, windows, outs=outs, var_nums=vns)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    if mixed:
        assert np.array_equal(outs[0].cpu().numpy(), want[0]), (geo, scale, q, ad, "the compact plane")
    check_written(T, big, items, [gpu(T, w) for w in want[len(names) - len(items):]], ("decode_bits_scaled", geo, scale, q, ad))


@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("geo", ["b", "d"])
def test_synth_into_wide_planes(T, dm, big, geo, kind):
    import oracle as O
    g = GEOS[geo]
    want = np.stack([O.synth_plane(31 + f, O.KINDS[kind], g["W"], g["H"]) for f in range(g["F"])])
    _state["readers"] = None
    fill_sentinel(big)
    dm.synth(31, kind, g["W"], g["H"], g["F"], out=plane_view(big, g))
    check_written(T, big, [plane_item(g, want)], [gpu(T, want)], ("synth", geo, kind))


# ---- colour ---------------------------------------------------------------------------------------------
CS_WIDE = GiB + 1028
COLOUR = {  # picture: (S, FS, channel stride of the planar layout); planes: {sub: [(S, FS)] * 3}
    "frames": dict(F=2, H=32, W=48, rgb=(152, L32 + 4104), planar=(56, L32 + 4104, CS_WIDE),
                   planes={"420": [(56, L32 + 8216), (56, L31 + 6168), (56, L32 + 12000)],
                           "444": [(56, L32 + 8216), (56, L31 + 6168), (56, L32 + 12000)]}),
    "rows": dict(F=1, H=80, W=48, rgb=(60921664, 0), planar=(60921664, 0, 4160),
                 planes={"420": [(60921672, 0), (120985136, 0), (120985144, 0)],
                         "444": [(60921672, 0), (60921680, 0), (60921688, 0)]}),
}
COLOUR_START = [2 * GiB + (8 + k) * MiB for k in range(4)]  # the picture, Y, Cb, Cr


def rgb_item(start, S, FS, step, CS, data):
    """The layout item of a picture data [F, H, W, 3]: interleaved (pixel step `step`, CS 1) or
    planar (step 1, channel stride CS)."""
    F, H, W, _ = data.shape
    f, r, x, c = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in (F, H, W, 3)], indexing="ij")
    off = (f * FS + r * S + x * step + c * CS).ravel()
    return dict(true=start + off, data=data.ravel(),
                aliases={"truncated": start + (off & M32), "sign-extended": start + sext32(off)},
                unit_of=((f * H + r) * (W // 8) + x // 8).ravel())


def colour_case(big, geo, layout, sub, rgb, planes):
    """(picture item, picture view, plane items, plane views) of host data rgb / planes."""
    c = COLOUR[geo]
    F, H, W = c["F"], c["H"], c["W"]
    if layout == "interleaved":
        S, FS = c["rgb"]
        step, CS = 3, 1
    else:
        S, FS, CS = c["planar"]
        step = 1
    FS = FS or S * H
    pic = rgb_item(COLOUR_START[0], S, FS, step, CS, rgb)
    pic_view = big.as_strided((F, H, W, 3), (FS, S, step, CS), COLOUR_START[0])
    items, views = [], []
    for k, (p, (s, fs)) in enumerate(zip(planes, c["planes"][sub])):
        g = dict(start=COLOUR_START[1 + k], S=s, FS=fs or s * p.shape[1])
        assert s % 8 == 0 and s & (s - 1) and g["FS"] % 8 == 0
        items.append(plane_item(g, p))
        views.append(plane_view(big, g, p.shape))
    for it in [pic] + items:
        assert int(it["true"].max()) < BIG and int(it["true"].max() - it["true"].min()) >= L31
    return pic, pic_view, items, views


@functools.lru_cache(maxsize=None)
def colour_data(geo, sub):
    c = COLOUR[geo]
    F, H, W = c["F"], c["H"], c["W"]
    rng = np.random.default_rng(F * 1000 + H + (sub == "420"))
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    s = 2 if sub == "420" else 1
    planes = [rng.integers(0, 256, shp, dtype=np.uint8) for shp in ((F, H, W), (F, H // s, W // s), (F, H // s, W // s))]
    return rgb, [np.ascontiguousarray(p) for p in color_ref.forward(rgb, sub)], planes, color_ref.inverse(*planes)


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("geo", list(COLOUR))
@pytest.mark.parametrize("direction", ["rgb_to_ycbcr", "ycbcr_to_rgb"])
def test_colour_wide(T, dm, big, direction, geo, layout, sub):
    rgb, want_planes, planes, want_rgb = colour_data(geo, sub)
    what = (direction, geo, layout, sub)
    _state["readers"] = None
    fill_sentinel(big)
    if direction == "rgb_to_ycbcr":
        pic, pic_view, items, views = colour_case(big, geo, layout, sub, rgb, want_planes)
        sources, written, wants = [pic], items, want_planes
    else:
        pic, pic_view, items, views = colour_case(big, geo, layout, sub, want_rgb, planes)
        sources, written, wants = items, [pic], [want_rgb]
    outside = lay(T, big, sources, 5, what)
    assert not any(outside.values()), (what, outside)
    if direction == "rgb_to_ycbcr":
        d = dm.rgb_desc(pic_view)
        assert d.pixel_step == (3 if layout == "interleaved" else 1)
        dm.rgb_to_ycbcr(pic_view, sub, outs=views)
    else:
        dm.ycbcr_to_rgb(*views, out=pic_view)
    for it in sources:  # the inputs are as they were, then leave with their aliases
        assert np.array_equal(read(T, big, it["true"]).cpu().numpy(), it["data"]), (what, "an input was written")
        for addr in [it["true"]] + list(it["aliases"].values()):
            erase(T, big, addr[(addr >= 0) & (addr < BIG)])
    check_written(T, big, written, [gpu(T, w) for w in wants], what)


# ---- 2. stream consumers: offsets that start high -------------------------------------------------------
STREAM_SHAPES = [(1, 8, 8 * 100), (1, 8, 8 * 179)]  # the plane boundary falls inside tile 1's second half
CROSS_BLOCK = 64 + 37


@functools.lru_cache(maxsize=None)
def stream_blocks():
    """279 blocks of (value, run), values in [-511, 511] \\ {0} and runs <= 2 so both symbol widths
    hold them: a sparse tile with empty blocks (lane path), a medium one (walk), a dense one
    (quad; its halves' bytes need several chunks of the bit source), a mixed one, 23 more."""
    rng = np.random.default_rng(77)

    def blk(n, dense=False):
        v = rng.integers(1, 512, n) * rng.choice([-1, 1], n)
        r = np.zeros(n, np.int64) if dense else rng.integers(0, 3, n)
        return [(int(a), int(b)) for a, b in zip(v, r)]

    blocks = [blk(int(rng.integers(0, 7))) if b % 5 else [] for b in range(64)]
    blocks += [blk(int(rng.integers(15, 26))) for _ in range(64)]
    blocks += [blk(64, dense=True) for _ in range(64)]
    blocks += [blk(int(rng.integers(0, 5))) if b % 3 else [] for b in range(32)] + [blk(64, dense=True) for _ in range(32)]
    blocks += [blk(int(rng.integers(10, 31))) if b != 7 else [] for b in range(23)]
    return blocks


@functools.lru_cache(maxsize=None)
def stream_host():
    """{4: uint32 symbols, 2: uint16 symbols, "off": symbol offsets, 1: packed bytes, "boff": byte offsets}"""
    blocks = stream_blocks()
    v = np.array([s[0] for b in blocks for s in b], np.int64)
    r = np.array([s[1] for b in blocks for s in b], np.int64)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.int64)
    by, boff = bits_ref.pack(blocks)
    halves = [int(off[min(a + 32, len(blocks))] - off[a]) for a in range(0, len(blocks), 32)]
    bhalves = [int(boff[min(a + 32, len(blocks))]) - int(boff[a]) for a in range(0, len(blocks), 32)]
    assert len(blocks) % 64 and any(not b for b in blocks)
    assert any(h <= 240 for h in halves) and any(240 < h <= 1024 for h in halves) and any(h > 1024 for h in halves)
    assert any(0 < h <= 2560 - 3 for h in bhalves) and any(h > 2560 for h in bhalves)
    return {4: ((v & 0xFFFF) | (r << 16)).astype(np.uint32), 2: ((r << 10) | (v & 0x3FF)).astype(np.uint16),
            "off": off, 1: by, "boff": boff.astype(np.int64)}


@functools.lru_cache(maxsize=None)
def stream_base0():
    """Every consumer on the stream at base 0 in ordinary allocations: the expected values."""
    import torch as T
    import dct_amd as dm
    h = stream_host()
    off, boff = gpu(T, h["off"].astype(np.uint32).view(np.int32)), gpu(T, h["boff"].astype(np.uint32).view(np.int32))
    sym = {4: gpu(T, h[4].view(np.int32)), 2: gpu(T, h[2].view(np.int16))}
    by = gpu(T, h[1])
    n = len(stream_blocks())
    vns = list(T.split(gpu(T, (np.random.default_rng(3).integers(0, 2000, n) * 4096).astype(np.int32)), [100, 179]))
    want = {"coef": dm.rle_decode(sym[4], off), "vns": vns, "lengths": dm.block_lengths(off), "blengths": dm.block_lengths(boff)}
    assert T.equal(dm.rle_decode(sym[2], off), want["coef"]) and T.equal(dm.bits_decode(by, boff), want["coef"])
    assert np.array_equal(want["coef"].cpu().numpy(), bits_ref.unpack(h[1], h["boff"]))
    packed, poff = dm.bits_pack(sym[4], off)
    assert T.equal(packed, by) and T.equal(poff, boff), "bits_pack at base 0 != tools/bits_ref.py"
    for q, ad in ((50, 0), (90, 1)):
        v = vns if ad else None
        want[q, ad] = plan_of(q, ad).decode_symbols(sym[4], off, shapes=STREAM_SHAPES, var_nums=v)
        for other in (plan_of(q, ad).decode_symbols(sym[2], off, shapes=STREAM_SHAPES, var_nums=v),
                      plan_of(q, ad).decode_bits(by, boff, shapes=STREAM_SHAPES, var_nums=v)):
            assert all(T.equal(a, b) for a, b in zip(other, want[q, ad]))
    want["bytes"], want["boff"] = by, boff
    return want


def placements():
    """{id: (element width, base, base pointer inside big)}"""
    h = stream_host()
    out = {}
    for par in (0, 1):  # two k of different parity
        ks = int(h["off"][CROSS_BLOCK]) + 1 + par   # the crossing falls inside block 101
        kb = int(h["boff"][CROSS_BLOCK]) + 1 + par
        assert h["off"][CROSS_BLOCK] < ks < h["off"][CROSS_BLOCK + 1] and h["boff"][CROSS_BLOCK] < kb < h["boff"][CROSS_BLOCK + 1]
        tag = "odd" if (ks & 1) else "even"
        out[f"sym4 at 2^30-k {tag}"] = (4, L30 - ks, GiB)
        out[f"sym4 at 2^31-k {tag}"] = (4, L31 - ks, 32 * MiB)
        out[f"sym2 at 2^31-k {tag}"] = (2, L31 - ks, 4 * GiB)
        out[f"sym2 at 2^32-total-{1 + par}"] = (2, L32 - int(h["off"][-1]) - 1 - par, 32 * MiB)
        tag = "odd" if (kb & 1) else "even"
        out[f"bytes at 2^31-k {tag}"] = (1, L31 - kb, 4 * GiB)
        out[f"bytes at 2^32-total-{1 + par}"] = (1, L32 - int(h["boff"][-1]) - 1 - par, 4 * GiB)
    return out


PLACEMENTS = placements()

# Windows for the three consumers that take one (packed bytes only).  The second set numbers the same
# 279 blocks as ONE plane, the two planes of STREAM_SHAPES side by side: over STREAM_SHAPES itself
# every window set has a run in plane 0, whose 100 blocks all lie below the crossing.
STREAM_ROW = [(1, 8, 8 * 279)]
WINDOW_SETS = {
    "the crossing inside a run": (STREAM_SHAPES, [((0, 1), (0, 8), (8 * 90, 8 * 100)), ((0, 1), (0, 8), (0, 8 * 70))]),
    "every run above the crossing": (STREAM_ROW, [((0, 1), (0, 8), (8 * 104, 8 * 188))]),
}


def test_window_sets_are_what_the_cases_need():
    boff = stream_host()["boff"]
    crossings = [int(boff[CROSS_BLOCK]) + 1 + par for par in (0, 1)]  # kb of placements(): base + kb is 2^31
    runs = {name: window_ref.runs(*ws) for name, ws in WINDOW_SETS.items()}
    inside = [(s0, nb) for s0, nb in runs["the crossing inside a run"].tolist() if s0 < CROSS_BLOCK < s0 + nb]
    assert len(inside) == 1  # ... and not as the run's first block: its first offset is below, its end above
    assert all(boff[s0] < kb <= boff[CROSS_BLOCK + 1] <= boff[s0 + nb] for s0, nb in inside for kb in crossings)
    assert all(s0 > CROSS_BLOCK and boff[s0] > max(crossings) for s0, _ in runs["every run above the crossing"].tolist())
    for name, r in runs.items():
        assert 64 in r[:, 1] and r[:, 1].min() < 32, (name, r[:, 1].tolist())
    assert sum(f * (h // 8) * (w // 8) for f, h, w in STREAM_ROW) == len(stream_blocks())


def window_consumers_at_high_offsets(T, dm, src, high, where):
    """Plan.decode_bits_window, Plan.decode_bits_scaled and bits_window on packed bytes at `high`
    offsets: slices of the base-0 pictures, tools/scaled_ref.py on the base-0 coefficients, and
    tools/extract_ref.py on the host stream."""
    h, want = stream_host(), stream_base0()
    coef = want["coef"].cpu().numpy()
    for name, (shapes, windows) in WINDOW_SETS.items():
        one = len(shapes) == 1
        vns = [T.cat(want["vns"])] if one else want["vns"]
        host_vns = [v.cpu().numpy() for v in vns]
        wb, wo, wv = extract_ref.window_stream(h[1], h["boff"], shapes, windows, host_vns)
        gb, go, gv = dm.bits_window(src, high, shapes, windows, var_nums=vns)
        assert np.array_equal(u32(go), wo), (where, name, "bits_window: offsets")
        assert gb.numel() == len(wb) and np.array_equal(gb.cpu().numpy(), wb), (where, name, "bits_window: bytes")
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(gv, wv)), (where, name, "bits_window: var_nums")
        for q, ad in ((50, 0), (90, 1)):
            plan, v = plan_of(q, ad), vns if ad else None
            full = [T.cat(want[q, ad], 2)] if one else want[q, ad]
            got = plan.decode_bits_window(src, high, shapes, windows, var_nums=v)
            for g, p, ((f0, f1), (y0, y1), (x0, x1)) in zip(got, full, windows):
                assert T.equal(g, p[f0:f1, y0:y1, x0:x1]), (where, name, q, ad, "decode_bits_window")
            for scale in (2, 4, 8):
                ref = scaled_ref.planes(coef, shapes, table(q, ad), scale, ad, host_vns if ad else None, windows)
                got = plan.decode_bits_scaled(src, high, shapes, scale, windows, var_nums=v)
                assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got, ref)), (where, name, q, ad, scale)


@pytest.mark.parametrize("where", list(PLACEMENTS))
def test_stream_consumers_at_high_offsets(T, dm, big, where):
    wd, base, ptr = PLACEMENTS[where]
    h, want = stream_host(), stream_base0()
    off0 = h["boff"] if wd == 1 else h["off"]
    data = np.ascontiguousarray(h[wd]).view(np.uint8)
    j = np.arange(data.size, dtype=np.int64)
    e, sub = base + j // wd, j % wd
    assert base + int(off0[-1]) <= M32 and (base + int(off0[-1])) * wd >= L31 and ptr % 4 == 0
    item = dict(true=ptr + e * wd + sub, data=data, unit_of=np.searchsorted(off0, j // wd, side="right") - 1,
                aliases={"byte offset truncated": ptr + ((e * wd) & M32) + sub,
                         "byte offset sign-extended": ptr + sext32(e * wd) + sub,
                         "index sign-extended": ptr + sext32(e) * wd + sub})
    _state["readers"] = None
    outside = lay(T, big, [item], 9, where)
    leaves = {k for k, v in outside.items() if v}
    assert leaves == ({"index sign-extended"} if where.startswith("sym4 at 2^31") else set()), (where, outside)
    high = gpu(T, ((base + off0) & M32).astype(np.uint32).view(np.int32))
    assert int(u32(high).max()) * wd >= L31  # the offset itself, or (4-byte symbols at 2^30) its byte offset
    lengths, lb = dm.block_lengths(high)
    wl, wlb = want["blengths" if wd == 1 else "lengths"]
    assert lb == wlb and T.equal(lengths, wl), (where, "block_lengths")
    if wd == 1:
        src = big[ptr:]
        assert T.equal(dm.bits_decode(src, high), want["coef"]), (where, "bits_decode")
    else:
        src = big[ptr:].view(T.int32 if wd == 4 else T.int16)
        assert T.equal(dm.rle_decode(src, high), want["coef"]), (where, "rle_decode")
        packed, poff = dm.bits_pack(src, high)
        assert T.equal(poff, want["boff"]) and int(u32(poff)[0]) == 0, (where, "bits_pack: byte offsets")
        assert T.equal(packed, want["bytes"]), (where, "bits_pack: bytes")
    for q, ad in ((50, 0), (90, 1)):
        v = want["vns"] if ad else None
        decode = plan_of(q, ad).decode_bits if wd == 1 else plan_of(q, ad).decode_symbols
        got = decode(src, high, shapes=STREAM_SHAPES, var_nums=v)
        assert all(T.equal(a, b) for a, b in zip(got, want[q, ad])), (where, q, ad, decode.__name__)
    if wd == 1:
        window_consumers_at_high_offsets(T, dm, src, high, where)


# ---- 3. stream producers: running totals that pass 2^31 --------------------------------------------------
PALETTE = 61


def tile_into(T, big, at, period, n_periods_total, tail):
    """big[at ..] = `period` (a u8 device tensor) repeated n times, then its first `tail` bytes:
    broadcasting copies of at most 128 MiB."""
    p = period.numel()
    step = max(1, (128 * MiB) // p)
    for k in range(0, n_periods_total, step):
        m = min(step, n_periods_total - k)
        big[at + k * p:at + (k + m) * p].view(m, p).copy_(period.view(1, p).expand(m, p))
    if tail:
        big[at + n_periods_total * p:at + n_periods_total * p + tail].copy_(period[:tail])


def equals_tiled(T, got, period):
    """got (1-D) == period repeated (and cut), compared 64 MiB at a time: the index of the first
    chunk that differs, or None."""
    p = period.numel()
    reps = max(1, (64 * MiB) // (p * period.element_size()))
    tile = period.repeat(reps)
    flags = [(got[a:a + tile.numel()] == tile[:min(tile.numel(), got.numel() - a)]).all()
             for a in range(0, got.numel(), tile.numel())]
    ok = T.stack(flags).cpu().numpy()
    return None if ok.all() else int(np.flatnonzero(~ok)[0])


def expected_offsets(T, per_block, n):
    """Exclusive prefix sums of per_block (int64 [P]) tiled over n blocks: int64 [n + 1] on the device."""
    tiled = gpu(T, per_block.astype(np.int64)).repeat(-(-n // per_block.size))[:n]
    return T.cat([T.zeros(1, dtype=T.int64, device="cuda"), T.cumsum(tiled, 0)])


def low32(T, t):
    return t.to(T.int64) & M32


def test_rle_count_total_past_2_31(T, dm, big):
    import oracle as O
    rng = np.random.default_rng(21)
    pal = rng.integers(1, 400, (PALETTE, 64)).astype(np.int16) * rng.choice([-1, 1], (PALETTE, 64)).astype(np.int16)
    for b in range(0, PALETTE, 10):  # a few sparse blocks, one of them all zero
        pal[b] = 0
        pal[b, rng.integers(0, 64, b // 10)] = 7
    off, _ = O.rle_encode_plane(pal)
    counts = np.diff(off.astype(np.int64))
    assert counts.min() == 1 and np.median(counts) == 64
    n = ((L31 + 10 ** 6) // int(counts.sum()) + 1) * PALETTE + 17
    n += n % 64 == 0  # a ragged last tile
    assert n < 1 << 26 and n % 64 and n % PALETTE and n * 128 <= BIG
    _state["readers"] = None
    tile_into(T, big, 0, gpu(T, pal).view(T.uint8).reshape(-1), n // PALETTE, (n % PALETTE) * 128)
    want = expected_offsets(T, counts, n)
    assert int(want[-1]) > L31 + 10 ** 6 and int(want[-1]) < L32
    guard = 64
    got = T.full((n + 1 + guard,), -1, dtype=T.int32, device="cuda")
    ws = T.empty(int(dm.lib().dctq_rle_workspace_bytes(n)) // 4 + 1, dtype=T.int32, device="cuda")
    rc = dm.lib().dctq_rle_count(C.c_void_p(big.data_ptr()), n, C.c_void_p(got.data_ptr()), C.c_void_p(ws.data_ptr()),
                                 C.c_void_p(T.cuda.current_stream().cuda_stream))
    assert rc == 0, dm.lib().dctq_error_string(rc)
    wrong = (low32(T, got[:n + 1]) != want).nonzero()
    assert wrong.numel() == 0, (f"{wrong.numel()} offsets differ, the first at block {int(wrong[0])}",
                                int(got[int(wrong[0])]) & M32, int(want[int(wrong[0])]))
    assert bool((got[n + 1:] == -1).all()), "written past offsets[n]"


@functools.lru_cache(maxsize=None)
def long_palette():
    """61 blocks of 64 long-coded 4-byte symbols: (symbols uint32 [61 * 64], bytes, byte offsets, coefficients)."""
    rng = np.random.default_rng(22)
    v = rng.integers(16384, 32768, (PALETTE, 64)) * rng.choice([-1, 1], (PALETTE, 64))  # codes of 31 and 33 bits
    r = np.where(rng.random((PALETTE, 64)) < 0.1, rng.integers(1, 70, (PALETTE, 64)), 0)
    blocks = [[(int(a), int(b)) for a, b in zip(vb, rb)] for vb, rb in zip(v, r)]
    by, boff = bits_ref.pack(blocks)
    return ((v & 0xFFFF) | (r << 16)).astype(np.uint32).ravel(), by, boff.astype(np.int64), bits_ref.unpack(by, boff)


def test_bits_pack_total_past_2_31(T, dm, big):
    sym, pby, pboff, pcoef = long_palette()
    lens, per, bw = np.diff(pboff), int(pboff[-1]), 1021
    rows = -(-((L31 + 10 ** 6) * PALETTE // per + PALETTE) // bw)
    while (rows * bw) % 64 == 0:
        rows += 1
    n = rows * bw
    assert 368 * n < L32 and n * 256 < 2 * GiB
    out_at = 4 * GiB  # the stream's base pointer: a sign-extended offset lands 2 GiB below it, in sentinel
    _state["readers"] = None
    tile_into(T, big, 0, gpu(T, sym).view(T.uint8), n // PALETTE, (n % PALETTE) * 256)
    fill_sentinel(big, n * 256, BIG)
    symv = big[:n * 256].view(T.int32)
    soff = (64 * T.arange(n + 1, dtype=T.int64, device="cuda")).to(T.int32)
    want = expected_offsets(T, lens, n)
    total = int(want[-1])
    assert L31 + 10 ** 6 < total < L32 and out_at + total + 64 <= BIG
    # offsets only
    empty, boff = dm.bits_pack(symv, soff, capacity=0)
    wrong = (low32(T, boff) != want).nonzero()
    assert empty.numel() == 0 and wrong.numel() == 0, (f"{wrong.numel()} offsets differ, the first at block {int(wrong[0])}",)
    assert first_dirty(T, big, n * 256, BIG) is None, "capacity 0 wrote bytes"
    period = gpu(T, pby)
    L = dm.lib()
    ws = T.empty(int(L.dctq_bits_workspace_bytes(n)) // 4 + 1, dtype=T.int32, device="cuda")
    tile = int((want[::64] > L31).nonzero()[0]) + 3
    short = int(want[64 * tile]) - 1  # one byte short of a tile boundary beyond 2^31
    assert L31 < short < total
    for cap in (short, total):
        off2 = T.full((n + 1,), -1, dtype=T.int32, device="cuda")
        rc = L.dctq_bits_pack(C.c_void_p(symv.data_ptr()), 4, C.c_void_p(soff.data_ptr()), n, C.c_void_p(off2.data_ptr()),
                              C.c_void_p(big.data_ptr() + out_at), cap, C.c_void_p(ws.data_ptr()),
                              C.c_void_p(T.cuda.current_stream().cuda_stream))
        assert rc == 0, L.dctq_error_string(rc)
        assert T.equal(off2, boff), (cap, "offsets must be complete")
        bad = equals_tiled(T, big[out_at:out_at + cap], period)
        assert bad is None, (cap, f"the stream differs from the palette's bytes in its 64 MiB chunk {bad}")
        at = first_dirty(T, big, out_at + cap, BIG)
        assert at is None, (cap, f"byte {at - out_at} of the stream, at or past the capacity, was written")
        at = first_dirty(T, big, n * 256, out_at)
        assert at is None, (cap, f"a store landed {out_at - at} bytes below the stream")
    # the byte consumers at offsets the packer reached by itself
    stream = big[out_at:out_at + total]
    coef = dm.bits_decode(stream, boff)
    bad = equals_tiled(T, coef.reshape(-1), gpu(T, pcoef).reshape(-1))
    assert bad is None, f"bits_decode differs from the palette's coefficients in chunk {bad}"
    plan, shape = plan_of(50, 0), (1, 8 * rows, 8 * bw)
    got = plan.decode_bits(stream, boff, shapes=[shape])[0]
    assert T.equal(got, plan.decode_planes([coef], shapes=[shape])[0]), "decode_bits != decode_planes(bits_decode)"


def as_i32(T, t):
    """int64 values below 2^32 as the int32 tensor that holds their uint32 bit patterns."""
    return (((t + L31) & M32) - L31).to(T.int32)


def same_bytes(T, a, b):
    """Two equally long u8 device tensors compared 256 MiB at a time: the first chunk that differs, or None."""
    flags = [T.equal(a[k:k + CHUNK], b[k:k + CHUNK]) for k in range(0, a.numel(), CHUNK)]
    return None if all(flags) else flags.index(False)


def test_window_payload_past_2_31(T, dm, big):
    """dctq_bits_window_offsets and dctq_bits_window_gather on a window whose own payload passes 2^31:
    a stream of the long palette (made by tiling, not by bits_pack) of F frames of one block row of
    1 021 blocks, and the window of its frames 1..F.  Source and destination both lie in `big`; the
    sign-extended alias of every source offset holds other bytes, that of every destination offset
    sentinel.  Then the window and the scaled decoder on the source's last two frames."""
    _, pby, pboff, pcoef = long_palette()
    lens, per, bw = np.diff(pboff), int(pboff[-1]), 1021
    F = -(-((L31 + 2 * 10 ** 6) * PALETTE // per + PALETTE) // bw) + 1
    while (F * bw) % 64 == 0 or (F * bw) % PALETTE == 0:
        F += 1
    n, nw = F * bw, (F - 1) * bw
    want = expected_offsets(T, lens, n)
    total, drop = int(want[-1]), int(want[bw])
    wtotal = total - drop
    assert L31 + 2 * 10 ** 6 < total < L32 and drop < 300_000 and wtotal > L31 + 10 ** 6 and n < 1 << 26
    # the layout: [a_lo, a_hi) and [d_lo, d_hi) are where sign-extended source and destination offsets land
    SRC, DST = 2 * GiB + 16 * MiB, 6 * GiB + 32 * MiB
    a_lo, a_hi = SRC + L31 - L32, SRC + total - L32
    d_lo, d_hi = DST + L31 - L32, DST + wtotal - L32
    assert 0 <= a_lo < a_hi <= SRC and SRC + total <= d_lo < d_hi <= DST and DST + wtotal + 64 <= BIG
    _state["readers"] = None
    fill_sentinel(big)
    period = gpu(T, pby)
    tile_into(T, big, SRC, period, n // PALETTE, int(pboff[n % PALETTE]))
    source = big[SRC:SRC + total]
    other = source[L31:] ^ 0x5A
    big[a_lo:a_hi].copy_(other)
    assert bool((big[a_lo:a_hi] != source[L31:]).all()) and equals_tiled(T, source, period) is None
    soff = as_i32(T, want)
    assert int(u32(soff[-1:])[0]) == total and int((soff < 0).sum()) > 1021
    var = T.arange(n, dtype=T.int32, device="cuda")

    shapes, windows = [(F, 8, 8 * bw)], [((1, F), (0, 8), (0, 8 * bw))]
    wins, wshapes, _ = dm._stored_windows(shapes, windows)
    assert wshapes == [(F - 1, 8, 8 * bw)]
    exts = (dm._Extent * 1)(dm._Extent(8 * bw, 8, F - 1))
    L, s = dm.lib(), C.c_void_p(T.cuda.current_stream().cuda_stream)
    ws = T.empty(int(L.dctq_bits_window_workspace_bytes(nw)) // 4 + 1, dtype=T.int32, device="cuda")
    guard = 64
    woff = T.full((nw + 1 + guard,), -1, dtype=T.int32, device="cuda")
    wvar = T.full((nw + guard,), -1, dtype=T.int32, device="cuda")
    vp = (C.c_void_p * 1)(var.data_ptr())
    rc = L.dctq_bits_window_offsets(soff.data_ptr(), vp, wins, exts, 1, woff.data_ptr(), wvar.data_ptr(), ws.data_ptr(), s)
    assert rc == 0, L.dctq_error_string(rc)
    wwant = want[bw:] - drop  # the source's offsets, rebased
    wrong = (low32(T, woff[:nw + 1]) != wwant).nonzero()
    assert wrong.numel() == 0, (f"{wrong.numel()} offsets differ, the first at block {int(wrong[0])}",
                                int(woff[int(wrong[0])]) & M32, int(wwant[int(wrong[0])]))
    assert T.equal(wvar[:nw], var[bw:]), "win_var_num != var_num from block 1021 on"
    assert bool((woff[nw + 1:] == -1).all()) and bool((wvar[nw:] == -1).all()), "written past the outputs"

    assert [192, 64] in window_ref.runs([(1, 8, 8 * bw)], [((0, 1), (0, 8), (0, 8 * bw))]).tolist()  # the runs of a row
    row = int((wwant[::bw] > L31).nonzero()[0]) + 1
    short = int(wwant[row * bw + 192]) - 1  # one byte short of a run boundary beyond 2^31
    assert L31 < short < wtotal - 64 * 368
    suffix = source[drop:]
    for cap in (short, wtotal):
        rc = L.dctq_bits_window_gather(source.data_ptr(), soff.data_ptr(), wins, exts, 1, woff.data_ptr(),
                                       big.data_ptr() + DST, cap, s)
        assert rc == 0, L.dctq_error_string(rc)
        bad = same_bytes(T, big[DST:DST + cap], suffix[:cap])
        assert bad is None, (cap, f"the payload differs from the source's suffix in its 256 MiB chunk {bad}")
        at = first_dirty(T, big, DST + cap, BIG)
        assert at is None, (cap, f"byte {at - DST} of the window's stream, at or past the capacity, was written")
        at = first_dirty(T, big, SRC + total, DST)  # the aliases of the destination offsets lie here
        assert at is None, (cap, f"a store landed {DST - at} bytes below the window's stream")
        for lo, hi in ((0, a_lo), (a_hi, SRC)):
            at = first_dirty(T, big, lo, hi)
            assert at is None, (cap, f"a store landed at byte {at}, below the source")
        assert T.equal(big[a_lo:a_hi], other), (cap, "the bytes at the source's aliases were written")
        assert equals_tiled(T, source, period) is None, (cap, "the source was written")

    # the consumers at offsets the source reached by itself: its last two frames
    b0 = (F - 2) * bw
    at0 = int(want[b0])
    assert at0 > L31
    compact, coff = source[at0:].clone(), as_i32(T, want[b0:] - at0)
    last = [((F - 2, F), (0, 8), (0, 8 * bw))]
    coef = pcoef[np.arange(b0, n) % PALETTE].astype(np.int16)
    wstream = big[DST:DST + wtotal]
    wlast = [((F - 3, F - 1), (0, 8), (0, 8 * bw))]
    for q, ad in ((50, 0), (90, 1)):
        plan = plan_of(q, ad)
        ref = plan.decode_bits(compact, coff, shapes=[(2, 8, 8 * bw)], var_nums=[var[b0:]] if ad else None)[0]
        got = plan.decode_bits_window(source, soff, shapes, last, var_nums=[var] if ad else None)[0]
        assert T.equal(got, ref), (q, ad, "decode_bits_window on the source != decode_bits of a compact copy")
        got = plan.decode_bits_window(wstream, woff[:nw + 1], wshapes, wlast, var_nums=[wvar[:nw]] if ad else None)[0]
        assert T.equal(got, ref), (q, ad, "decode_bits_window on the window's stream != decode_bits of a compact copy")
        host_vns = [var[b0:].cpu().numpy()] if ad else None
        for scale in (2, 4, 8):
            ref = scaled_ref.planes(coef, [(2, 8, 8 * bw)], table(q, ad), scale, ad, host_vns)[0]
            got = plan.decode_bits_scaled(source, soff, shapes, scale, last, var_nums=[var] if ad else None)[0]
            assert np.array_equal(got.cpu().numpy(), ref), (q, ad, scale, "decode_bits_scaled != tools/scaled_ref.py")


def test_block_offsets_at_the_maximum(T, dm):
    n = MAX_BLOCKS
    assert 368 * n < L32 <= 368 * (n + 1)
    clamp = T.full((n,), 1000, dtype=T.int16, device="cuda")  # every length above the clamp of 368
    off = dm.block_offsets(clamp)
    want = 368 * T.arange(n + 1, dtype=T.int64, device="cuda")
    assert int(want[-1]) == L32 - 288 and T.equal(low32(T, off), want)
    back, lb = dm.block_lengths(off, length_bytes=2)
    assert lb == 2 and bool((back == 368).all())
    rng = np.random.default_rng(8)
    for lb, dt, lo, top in ((1, np.uint8, 128, 256), (2, np.uint16, 100, 369)):  # both totals pass 2^31
        lengths = rng.integers(lo, top, n).astype(dt)
        ref = frame_ref.offsets_from_lengths(lengths)
        assert L31 + 10 ** 6 < int(ref[-1]) < L32
        dev = gpu(T, lengths.view(np.int16) if lb == 2 else lengths)
        off = dm.block_offsets(dev)
        assert np.array_equal(u32(off), np.asarray(ref).astype(np.uint32)), lb
        back, got_lb = dm.block_lengths(off, length_bytes=lb)
        assert got_lb == lb and T.equal(back, dev), lb
    one_more = T.zeros(n + 1, dtype=T.uint8, device="cuda")
    with pytest.raises(dm.DctqError):
        dm.block_offsets(one_more)
    with pytest.raises(dm.DctqError):
        dm.block_lengths(T.zeros(n + 2, dtype=T.int32, device="cuda"), length_bytes=1)
