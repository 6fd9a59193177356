"""GPU: the stream paste (dctq_bits_paste_offsets, dctq_bits_paste_copy; bits_paste) against
tools/paste_ref.py, byte for byte: every geometry of the definition, every pair of source and
destination alignment for both sources, guard bytes and short capacities, grid-stride loops that run
more than once, var_num merged, source offsets with bit 31 set and result offsets past 2^31.  Then
the containers: frame_paste inverts frame_window, equals compress of the edited picture and
decompresses to the edited picture; frame_tile equals compress of the joined picture, for a grid and
for the band shards of dct_amd/shard.py; and every refusal comes before anything is launched."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import paste_ref  # noqa: E402
import window_ref  # noqa: E402

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 40, 368)
SENTINEL = 0xA5
GUARD = 64


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


def nblocks(shapes):
    return [f * (h // 8) * (w // 8) for f, h, w in shapes]


def blk(f, y, x):
    """A window from block coordinates."""
    return (f, (8 * y[0], 8 * y[1]), (8 * x[0], 8 * x[1]))


def whole(shapes):
    return [((0, f), (0, h), (0, w)) for f, h, w in shapes]


def last_block(shapes):
    wins = [((0, 1), (0, 8), (0, 8)) for _ in shapes]
    f, h, w = shapes[-1]
    wins[-1] = ((f - 1, f), (h - 8, h), (w - 8, w))
    return wins


THREE = [(2, 32, 48), (2, 16, 24), (2, 16, 24)]
FOUR = [(1, 16, 16), (2, 8, 24), (1, 24, 8), (3, 8, 8)]
WIDE = [(2, 32, 1056), (2, 16, 528), (2, 16, 528)]     # 1584 blocks: 25 tiles
CASES = {
    "a one block": ([(1, 16, 24)], [blk((0, 1), (1, 2), (1, 2))]),
    "b bw 3, a column over rows and frames": ([(4, 40, 24)], [blk((1, 3), (1, 4), (1, 2))]),
    "c 70 of 130 columns": ([(1, 16, 1040)], [blk((0, 1), (0, 2), (30, 100))]),
    "d three planes": (THREE, [blk((0, 2), (1, 3), (2, 5)), blk((1, 2), (0, 1), (1, 3)), blk((0, 1), (1, 2), (0, 1))]),
    "e four planes": (FOUR, [blk((0, 1), (1, 2), (0, 2)), blk((1, 2), (0, 1), (1, 2)), blk((0, 1), (1, 3), (0, 1)),
                             blk((2, 3), (0, 1), (0, 1))]),
    "f whole, one plane": ([(4, 40, 24)], whole([(4, 40, 24)])),
    "f whole, three planes": (THREE, whole(THREE)),
    "g last block, one plane": ([(1, 16, 1040)], last_block([(1, 16, 1040)])),
    "g last block of the last plane": (THREE, [blk((0, 1), (0, 1), (0, 1)), blk((0, 1), (0, 1), (0, 1)),
                                              blk((1, 2), (1, 2), (2, 3))]),
    "wide": (WIDE, [blk((0, 2), (1, 3), (3, 131)), blk((1, 2), (0, 2), (0, 66)), blk((0, 1), (1, 2), (65, 66))]),
}


def test_case_g_takes_the_last_block_only():
    for name in ("g last block, one plane",):
        shapes, windows = CASES[name]
        assert window_ref.blocks(shapes, windows)[-1].reshape(-1).tolist() == [sum(nblocks(shapes)) - 1]
    shapes, windows = CASES["g last block of the last plane"]
    assert window_ref.blocks(shapes, windows)[-1].reshape(-1).tolist() == [sum(nblocks(shapes)) - 1]


def random_stream(rng, n):
    ln = rng.choice(LENGTHS, n)
    ln[:min(n, len(LENGTHS))] = LENGTHS[::-1][:min(n, len(LENGTHS))]     # every length, the longest first
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(shapes, windows, base (data, off, var), patch (data, off, var), want (bytes, offsets, var))."""
    shapes, windows = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    nbs = nblocks(shapes)
    wnbs = [b.size for b in window_ref.blocks(shapes, windows)]
    data, off = random_stream(rng, sum(nbs))
    pdata, poff = random_stream(rng, sum(wnbs))
    var = [rng.integers(-5, 1 << 24, n).astype(np.int32) for n in nbs]
    pvar = [rng.integers(-(1 << 24), -5, n).astype(np.int32) for n in wnbs]
    want = paste_ref.paste_stream(data, off, shapes, windows, pdata, poff, var, pvar)
    return shapes, windows, (data, off, var), (pdata, poff, pvar), want


def shifted(T, data, k, room=3):
    """The host bytes on the device as a view k bytes into its allocation."""
    buf = T.empty(len(data) + room + 4, dtype=T.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    buf[k:k + len(data)].copy_(T.from_numpy(np.ascontiguousarray(data)))
    return buf[k:k + len(data)]


def dev_i32(T, a):
    return T.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


# ---- 1. equality with the definition, through the package ---------------------------------------------------
@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_bits_paste_equals_the_definition(T, dm, name, adaptive):
    shapes, windows, (data, off, var), (pdata, poff, pvar), (wb, wo, wv) = host_case(name)
    kw = {}
    if adaptive:
        kw = dict(var_nums=[dev_i32(T, v) for v in var], patch_var_nums=[dev_i32(T, v) for v in pvar])
    gb, go, gv = dm.bits_paste(shifted(T, data, 1), dev_i32(T, off), shapes, windows, shifted(T, pdata, 2),
                               dev_i32(T, poff), **kw)
    assert gb.dtype == T.uint8 and go.dtype == T.int32 and gb.is_contiguous()
    assert np.array_equal(u32(go), wo), (name, "offsets differ")
    assert gb.numel() == len(wb) and np.array_equal(gb.cpu().numpy(), wb), (name, "bytes differ")
    if adaptive:
        assert len(gv) == len(wv) and all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(gv, wv)), (name, "var_nums")
    else:
        assert gv is None


@pytest.mark.parametrize("name", ["b bw 3, a column over rows and frames", "d three planes", "wide"])
def test_paste_inverts_bits_window(T, dm, name):
    shapes, windows, (data, off, var), _, _ = host_case(name)
    by, boff, vns = shifted(T, data, 3), dev_i32(T, off), [dev_i32(T, v) for v in var]
    wb, wo, wv = dm.bits_window(by, boff, shapes, windows, var_nums=vns)
    gb, go, gv = dm.bits_paste(by, boff, shapes, windows, wb, wo, vns, wv)
    assert T.equal(gb, by) and T.equal(go, boff) and all(T.equal(a, b) for a, b in zip(gv, vns))


# ---- 2. the write contract and alignment, through the C entry points ------------------------------------------
def raw_paste(dm, T, by, boff, pby, pboff, shapes, windows, vns=None, pvns=None, out=None, ooff=None, ovar=None,
              capacity=None, payload=None, patch_payload=None):
    """The two C calls on caller-placed buffers -> (out, ooff, ovar, total, grids)."""
    wins, wshapes, nbs = dm._stored_windows(shapes, windows)
    n, nblk = len(wshapes), sum(nbs)
    exts = (dm._Extent * n)(*[dm._Extent(w, h, f) for f, h, w in wshapes])
    L = dm.lib()
    ws = T.empty(int(L.dctq_bits_paste_workspace_bytes(nblk)) // 4 + 1, dtype=T.int32, device="cuda")
    ooff = T.empty(nblk + 1, dtype=T.int32, device="cuda") if ooff is None else ooff
    if vns is not None and ovar is None:
        ovar = T.empty(nblk, dtype=T.int32, device="cuda")
    vp = None if vns is None else (C.c_void_p * n)(*[v.data_ptr() for v in vns])
    pvp = None if pvns is None else (C.c_void_p * n)(*[v.data_ptr() for v in pvns])
    s = dm._stream_ptr()
    rc = L.dctq_bits_paste_offsets(boff.data_ptr(), vp, pboff.data_ptr(), pvp,
                                   by.numel() if payload is None else payload,
                                   pby.numel() if patch_payload is None else patch_payload, wins, exts, n,
                                   ooff.data_ptr(), None if vns is None else ovar.data_ptr(), ws.data_ptr(), s)
    assert rc == 0, L.dctq_error_string(rc)
    grids = [dm.last_grid()]
    total = int(u32(ooff[nblk:nblk + 1])[0])
    out = T.empty(max(total, 1), dtype=T.uint8, device="cuda") if out is None else out
    rc = L.dctq_bits_paste_copy(by.data_ptr(), boff.data_ptr(), pby.data_ptr(), pboff.data_ptr(), wins, exts, n,
                                ooff.data_ptr(), out.data_ptr(), total if capacity is None else capacity, s)
    assert rc == 0, L.dctq_error_string(rc)
    grids.append(dm.last_grid())
    T.cuda.synchronize()
    return out, ooff, ovar, total, grids


def segments(shapes, windows, off, poff, new):
    """The copy's segments on the host: (from patch, source byte, destination byte, bytes), tile by
    tile of 64 result blocks, split where the source changes or stops being consecutive."""
    n = sum(nblocks(shapes))
    src = np.full(n, -1, np.int64)
    src[np.concatenate([b.reshape(-1) for b in window_ref.blocks(shapes, windows)])] = np.arange(len(poff) - 1)
    out, s = [], 0
    while s < n:
        e = s + 1
        while e < n and e % 64 and (src[e] >= 0) == (src[s] >= 0) and (src[e] == src[e - 1] + 1 if src[s] >= 0 else True):
            e += 1
        a = int(poff[src[s]]) if src[s] >= 0 else int(off[s])
        out.append((bool(src[s] >= 0), a, int(new[s]), int(new[e]) - int(new[s])))
        s = e
    return out


def test_all_sixteen_alignment_pairs_for_each_source(T, dm):
    """Base, patch and output pointers 0..3 bytes into their allocations: every (source mod 4,
    destination mod 4) occurs for segments from the base and for segments from the patch, and the
    result is the definition's each time, with the guard bytes around the output intact."""
    shapes, windows, (data, off, _), (pdata, poff, _), (wb, wo, _) = host_case("wide")
    boff, pboff = dev_i32(T, off), dev_i32(T, poff)
    segs = [s for s in segments(shapes, windows, off, poff, wo) if s[3] >= 12]
    seen = {False: set(), True: set()}
    total = len(wb)
    for ks, ko in itertools.product(range(4), range(4)):
        by, pby = shifted(T, data, ks), shifted(T, pdata, (ks + 1) % 4)
        big = T.full((GUARD + ko + total + GUARD,), SENTINEL, dtype=T.uint8, device="cuda")
        out = big[GUARD + ko:GUARD + ko + total]
        raw_paste(dm, T, by, boff, pby, pboff, shapes, windows, out=out)
        got = big.cpu().numpy()
        assert np.array_equal(got[GUARD + ko:GUARD + ko + total], wb), (ks, ko)
        assert (got[:GUARD + ko] == SENTINEL).all() and (got[GUARD + ko + total:] == SENTINEL).all(), (ks, ko)
        for patch, a, d, _ in segs:
            base = pby.data_ptr() if patch else by.data_ptr()
            seen[patch].add(((base + a) % 4, (out.data_ptr() + d) % 4))
    every = set(itertools.product(range(4), range(4)))
    assert seen[False] == every and seen[True] == every, (every - seen[False], every - seen[True])


@pytest.mark.parametrize("name", ["d three planes", "c 70 of 130 columns", "wide"])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_guard_bytes_and_short_capacity(T, dm, name, lead):
    """64 guard bytes before and after the bytes, the offsets and var_num as views inside sentinel-
    filled allocations: every sentinel survives; a short capacity leaves every byte at or past it."""
    shapes, windows, (data, off, var), (pdata, poff, pvar), (wb, wo, wv) = host_case(name)
    by, pby = shifted(T, data, 1), shifted(T, pdata, 3)
    boff, pboff = dev_i32(T, off), dev_i32(T, poff)
    vns, pvns = [dev_i32(T, v) for v in var], [dev_i32(T, v) for v in pvar]
    n, total = len(wo) - 1, len(wb)
    big = T.full((GUARD + lead + total + GUARD,), SENTINEL, dtype=T.uint8, device="cuda")
    obuf = T.full((n + 1 + 8,), 0x5A5A5A5A, dtype=T.int32, device="cuda")
    vbuf = T.full((n + 8,), 0x5A5A5A5A, dtype=T.int32, device="cuda")
    a = GUARD + lead
    out, ooff, ovar = big[a:a + total], obuf[3:3 + n + 1], vbuf[5:5 + n]
    raw_paste(dm, T, by, boff, pby, pboff, shapes, windows, vns, pvns, out, ooff, ovar)
    assert np.array_equal(u32(ooff), wo) and np.array_equal(out.cpu().numpy(), wb)
    assert np.array_equal(ovar.cpu().numpy(), np.concatenate(wv))
    for buf, lo, hi, s in ((big, a, a + total, SENTINEL), (obuf, 3, 3 + n + 1, 0x5A5A5A5A), (vbuf, 5, 5 + n, 0x5A5A5A5A)):
        assert bool((buf[:lo] == s).all()) and bool((buf[hi:] == s).all()), (name, lead, "a sentinel was overwritten")
    first_tile = int(wo[min(64, n)])
    for cap in sorted({1, 2, 3, first_tile // 2 + 1, total // 2 + 1, total // 2 + 2, total - 1}):
        big.fill_(SENTINEL)
        raw_paste(dm, T, by, boff, pby, pboff, shapes, windows, vns, pvns, out, ooff, ovar, capacity=cap)
        got = big.cpu().numpy()
        assert np.array_equal(got[a:a + cap], wb[:cap]), (name, lead, cap)
        assert (got[:a] == SENTINEL).all() and (got[a + cap:] == SENTINEL).all(), (name, lead, cap)


# ---- 3. the grid-stride loops run more than once -----------------------------------------------------------------
def test_under_a_grid_limit(T, dm):
    shapes, windows, (data, off, var), (pdata, poff, pvar), (wb, wo, wv) = host_case("wide")
    assert sum(nblocks(shapes)) > 1024
    by, pby = shifted(T, data, 3), shifted(T, pdata, 0)
    boff, pboff = dev_i32(T, off), dev_i32(T, poff)
    vns, pvns = [dev_i32(T, v) for v in var], [dev_i32(T, v) for v in pvar]
    for limit in (1, 3):
        with dm.grid_limit(limit):
            out, ooff, ovar, total, grids = raw_paste(dm, T, by, boff, pby, pboff, shapes, windows, vns, pvns)
            assert grids == [limit, limit] and -(-(len(wo) - 1) // 64) > 4 * limit     # every wave loops
            assert total == len(wb) and np.array_equal(u32(ooff), wo)
            assert np.array_equal(out[:total].cpu().numpy(), wb)
            assert np.array_equal(ovar.cpu().numpy(), np.concatenate(wv))
            gb, go, gv = dm.bits_paste(by, boff, shapes, windows, pby, pboff, vns, pvns)
            assert dm.last_grid() == limit
            assert np.array_equal(gb.cpu().numpy(), wb) and np.array_equal(u32(go), wo)


# ---- 4. offsets with bit 31 set --------------------------------------------------------------------------------
def test_source_offsets_with_bit_31_set(T, dm):
    """Both payloads lie past 2^31 in one uninitialised tensor, so every source offset has bit 31
    set; the payload sizes handed to the offsets call are the streams' own."""
    shapes, windows, (data, off, _), (pdata, poff, _), (wb, wo, _) = host_case("d three planes")
    base_at, patch_at = (1 << 31) + 5, (1 << 31) + (1 << 20) + 2
    big = T.empty((1 << 31) + (2 << 20), dtype=T.uint8, device="cuda")
    big[base_at:base_at + len(data)].copy_(T.from_numpy(data))
    big[patch_at:patch_at + len(pdata)].copy_(T.from_numpy(pdata))
    hoff, hpoff = (off.astype(np.int64) + base_at).astype(np.uint32), (poff.astype(np.int64) + patch_at).astype(np.uint32)
    assert (hoff >> 31).all() and (hpoff >> 31).all()
    out, ooff, _, total, _ = raw_paste(dm, T, big, dev_i32(T, hoff), big, dev_i32(T, hpoff), shapes, windows,
                                       payload=len(data), patch_payload=len(pdata))
    assert total == len(wb) and np.array_equal(u32(ooff), wo) and np.array_equal(out[:total].cpu().numpy(), wb)
    del big
    T.cuda.empty_cache()


def test_result_offsets_past_2_31(T, dm):
    """6 000 000 blocks of 368 B: the result's offsets are arange * 368 and pass 2^31 inside the
    window; bytes are compared on tiles around the window, around 2^31 and at both ends."""
    bw, bh, size = 3000, 2000, 368
    n = bw * bh
    shapes = [(1, 8 * bh, 8 * bw)]
    cross = (1 << 31) // size                      # the block that holds byte 2^31
    row, col = divmod(cross, bw)
    windows = [blk((0, 1), (row - 5, row + 5), (col - 70, col + 70))]
    wblocks = T.from_numpy(window_ref.blocks(shapes, windows)[0].reshape(-1)).cuda()
    assert cross in wblocks.tolist() and col - 70 >= 0 and col + 70 <= bw
    nw = wblocks.numel()
    g = T.Generator(device="cuda").manual_seed(5)
    base = T.randint(0, 256, (n * size,), dtype=T.uint8, device="cuda", generator=g)
    patch = T.randint(0, 256, (nw * size,), dtype=T.uint8, device="cuda", generator=g)
    steps = T.arange(n + 1, dtype=T.int64, device="cuda") * size
    boff = T.where(steps >= 1 << 31, steps - (1 << 32), steps).to(T.int32)
    pboff = (T.arange(nw + 1, dtype=T.int64, device="cuda") * size).to(T.int32)
    gb, go, _ = dm.bits_paste(base, boff, shapes, windows, patch, pboff)
    assert gb.numel() == n * size and T.equal(go, boff)
    got, b2, p2 = gb.view(n, size), base.view(n, size), patch.view(nw, size)
    assert T.equal(got[wblocks], p2), "the window's blocks are not the patch's"
    lo, hi = (row - 6) * bw, (row + 6) * bw
    for a, b in ((0, 4096), (lo, hi), (cross - 128, cross + 128), (n - 4096, n)):
        want = b2[a:b].clone()
        inside = (wblocks >= a) & (wblocks < b)
        want[wblocks[inside] - a] = p2[inside]
        assert T.equal(got[a:b], want), (a, b)
    del base, patch, gb, got, b2
    T.cuda.empty_cache()


def test_payloads_of_2_32_together_are_refused_before_a_launch(T, dm):
    shapes, windows = CASES["a one block"]
    big = T.empty((1 << 32) - 8, dtype=T.uint8, device="cuda")
    off = T.zeros(7, dtype=T.int32, device="cuda")
    poff = T.zeros(2, dtype=T.int32, device="cuda")
    with dm.grid_limit(5):
        marker(T, dm)
        with pytest.raises(dm.DctqError, match="2\\^32"):
            dm.bits_paste(big, off, shapes, windows, T.empty(8, dtype=T.uint8, device="cuda"), poff)
        assert dm.last_grid() == 3
        gb, go, _ = dm.bits_paste(big, off, shapes, windows, T.empty(7, dtype=T.uint8, device="cuda"), poff)
        assert gb.numel() == 0 and not go.any()
    del big
    T.cuda.empty_cache()


def marker(T, dm):
    """A launch whose grid (3 workgroups under grid_limit(5)) no refused call could leave behind:
    the containers of these tests give every launch one workgroup."""
    shapes = [(1, 8, 8 * 700)]
    off = T.zeros(701, dtype=T.int32, device="cuda")
    dm.bits_window(T.zeros(4, dtype=T.uint8, device="cuda"), off, shapes, whole(shapes))
    assert dm.last_grid() == 3


# ---- 5. containers -------------------------------------------------------------------------------------------------
def picture(T, shape, seed):
    """Noise over a ramp, so blocks differ in size and neighbours in content."""
    g = T.Generator(device="cpu").manual_seed(seed)
    ramp = T.arange(shape[-2 if len(shape) == 4 else -1]).remainder(200).to(T.int32)
    ramp = ramp.view(-1, 1) if len(shape) == 4 else ramp
    x = T.randint(0, 96, shape, generator=g, dtype=T.int32) + ramp
    return x.clamp(0, 255).to(T.uint8).cuda()


# name: (kind, shape(s), subsampling, [(at, patch size (h, w), frame, patch frames)]): the first patch ends on the
# true picture's edge, which is off the block grid; the second lies inside
SOURCES = {
    "rgb 420": ("rgb", (3, 70, 94, 3), "420", [((48, 64), (22, 30), 1, 2), ((16, 32), (32, 16), 0, 1)]),
    "rgb 444": ("rgb", (2, 38, 46, 3), "444", [((24, 32), (14, 14), 0, 2), ((8, 8), (16, 24), 1, 1)]),
    "planes": ("planes", [(2, 38, 46), (2, 27, 20)], None,
               [([(32, 40), (16, 8)], [(6, 6), (11, 12)], 1, 1), ([(8, 16), (0, 8)], [(24, 8), (16, 8)], 0, 2)]),
}


@functools.lru_cache(maxsize=None)
def source(name):
    import torch
    kind, shape, _, _ = SOURCES[name]
    if kind == "rgb":
        return picture(torch, shape, 3)
    return [picture(torch, s, 4 + k) for k, s in enumerate(shape)]


def compress(dm, name, x, q, adaptive):
    sub = SOURCES[name][2]
    return dm.compress(x, q, bool(adaptive), **({"subsampling": sub} if sub else {}))


def patch_of(T, name, size, frames, seed):
    if SOURCES[name][0] == "rgb":
        return picture(T, (frames, size[0], size[1], 3), seed)
    return [picture(T, (frames, h, w), seed + k) for k, (h, w) in enumerate(size)]


def written(name, x, p, at, frame):
    """x with p written in at `at` from frame `frame`."""
    if SOURCES[name][0] == "rgb":
        y = x.clone()
        y[frame:frame + p.shape[0], at[0]:at[0] + p.shape[1], at[1]:at[1] + p.shape[2]] = p
        return y
    out = []
    for xp, pp, (ay, ax) in zip(x, p, at):
        y = xp.clone()
        y[frame:frame + pp.shape[0], ay:ay + pp.shape[1], ax:ax + pp.shape[2]] = pp
        out.append(y)
    return out


def region_of(name, at, size):
    if SOURCES[name][0] == "rgb":
        return ((at[0], at[0] + size[0]), (at[1], at[1] + size[1]))
    return [((ay, ay + h), (ax, ax + w)) for (ay, ax), (h, w) in zip(at, size)]


def same(T, a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(T, x, y) for x, y in zip(a, b))
    return a.shape == b.shape and T.equal(a, b)


@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("name", list(SOURCES))
def test_frame_paste(T, dm, name, adaptive):
    x = source(name)
    buf = compress(dm, name, x, 50, adaptive)
    for i, (at, size, frame, pf) in enumerate(SOURCES[name][3]):
        what = (name, adaptive, at, size, frame)
        # the window pasted back is the identity
        w = dm.frame_window(buf, region=region_of(name, at, size), frames=(frame, frame + pf))
        got = dm.frame_paste(buf, w, at=at, frame=frame)
        assert got.dtype == T.uint8 and got.shape == buf.shape and T.equal(got, buf), what
        # a new patch: compress of the edited picture, and its decompress is the edited decompress
        p = patch_of(T, name, size, pf, 50 + i)
        cp = compress(dm, name, p, 50, adaptive)
        got = dm.frame_paste(buf, cp, at=at, frame=frame)
        want = compress(dm, name, written(name, x, p, at, frame), 50, adaptive)
        assert got.shape == want.shape and T.equal(got, want), what + ("compress of the edited picture",)
        assert same(T, dm.decompress(got), written(name, dm.decompress(buf), dm.decompress(cp), at, frame)), \
            what + ("decompress",)


@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("name", list(SOURCES))
def test_frame_tile_of_a_2_by_3_grid(T, dm, name, adaptive):
    """Rows of 16 and the rest, three columns of m, m and the rest: the last row and column end off-grid."""
    x = source(name)
    ys, xs = [0, 16, None], [0, 16, 32, None] if SOURCES[name][0] == "rgb" else [0, 8, 16, None]

    def cut(t, r, c):
        return t[:, ys[r]:ys[r + 1], xs[c]:xs[c + 1]].contiguous()

    grid = [[compress(dm, name, cut(x, r, c) if SOURCES[name][0] == "rgb" else [cut(p, r, c) for p in x], 50, adaptive)
             for c in range(3)] for r in range(2)]
    got = dm.frame_tile(grid)
    want = compress(dm, name, x, 50, adaptive)
    assert got.shape == want.shape and T.equal(got, want), (name, adaptive)


@pytest.mark.parametrize("adaptive", [0, 1])
def test_frame_tile_of_band_shards(T, dm, adaptive):
    """Each rank compresses the band dct_amd/shard.py cuts for it; the bands tiled are the whole."""
    from dct_amd import shard
    plane = picture(T, (2, 88, 48), 9)
    world = 3
    bands = [shard.band_shard(plane, world, r)[0].contiguous() for r in range(world)]
    assert [b.shape[1] for b in bands] == [32, 32, 24]
    got = dm.frame_tile([[dm.compress([b], 50, bool(adaptive))] for b in bands])
    want = dm.compress([plane], 50, bool(adaptive))
    assert got.shape == want.shape and T.equal(got, want)


def test_frame_blank_decodes_to_grey(T, dm):
    for adaptive in (False, True):
        b = dm.frame_blank([(2, 16, 24), (2, 8, 8)], 50, adaptive, crops=[(3, 0), (0, 1)])
        assert bytes(b.cpu().numpy()) == paste_ref.frame_blank([(2, 16, 24), (2, 8, 8)], 50, adaptive, crops=[(3, 0), (0, 1)])
        a, c = dm.decompress(b)
        assert tuple(a.shape) == (2, 13, 24) and tuple(c.shape) == (2, 8, 7) and bool((a == 128).all()) and bool((c == 128).all())


def test_refusals_launch_nothing(T, dm):
    """Every refusal of frame_paste and frame_tile is raised with nothing launched: the grid of the
    last launch is still the marker's."""
    x = picture(T, (2, 38, 46), 1)                    # true 38 x 46, stored 40 x 48
    rgb = picture(T, (2, 38, 62, 3), 2)
    tile = picture(T, (1, 16, 16), 3)
    with dm.grid_limit(5):
        base = dm.compress([x], 50)
        col = dm.compress(rgb, 50)                    # 4:2:0
        c = lambda p, **kw: dm.compress(p, **{"quality": 50, **kw})   # noqa: E731
        bad = [
            (base, c([tile], quality=60), dict(at=(8, 16))),
            (base, c([tile], adaptive=True), dict(at=(8, 16))),
            (base, c([tile, tile]), dict(at=(8, 16))),
            (base, c(picture(T, (1, 16, 16, 3), 4)), dict(at=(0, 0))),
            (col, c(picture(T, (1, 16, 16, 3), 4), subsampling="444"), dict(at=(16, 16))),
            (col, c(picture(T, (1, 16, 16, 3), 4)), dict(at=(8, 16))),
            (base, c([tile]), dict(at=(4, 16))),
            (base, c([tile]), dict(at=(8, 12))),
            (base, c([tile]), dict(at=(-8, 16))),
            (base, c([tile]), dict(at=(8, 16), frame=2)),
            (base, c([tile]), dict(at=(8, 16), frame=-1)),
            (base, c([picture(T, (3, 16, 16), 5)]), dict(at=(8, 16))),
            (base, c([tile]), dict(at=(24, 16))),                           # rows 24..40 leave the 38
            (base, c([tile]), dict(at=(8, 32))),                            # columns 32..48 leave the 46
            (base, c([picture(T, (1, 14, 16), 6)]), dict(at=(8, 16))),      # a crop that ends inside
            (base, c([picture(T, (1, 13, 16), 6)]), dict(at=(24, 16))),     # true rows end at 37
            (base, c([tile]), dict(at=[(8, 16), (8, 16)])),
        ]
        tiles = [[c([picture(T, (1, 16, 16), 7)]), c([picture(T, (1, 16, 13), 8)])],
                 [c([picture(T, (1, 11, 16), 9)]), c([picture(T, (1, 11, 13), 10)])]]
        grids = [
            [tiles[0], tiles[1][:1]],
            [tiles[1], tiles[0]],                                          # a bottom crop that is not last
            [[row[1], row[0]] for row in tiles],                           # a right crop that is not last
            [[tiles[0][0], tiles[1][0]]],                                  # heights differ along a row
            [[tiles[0][0]], [tiles[0][1]]],                                # widths differ along a column
            [[tiles[0][0], c([picture(T, (1, 16, 16), 7)], quality=51)]],
            [[tiles[0][0], c([picture(T, (2, 16, 16), 7)])]],
        ]
        marker(T, dm)
        for buf, patch, kw in bad:
            with pytest.raises(dm.DctqError):
                dm.frame_paste(buf, patch, **kw)
            assert dm.last_grid() == 3, kw
        for g in grids:
            with pytest.raises(dm.DctqError):
                dm.frame_tile(g)
            assert dm.last_grid() == 3
        # and the accepted neighbours of those refusals do launch
        dm.frame_paste(base, c([picture(T, (1, 14, 16), 6)]), at=(24, 16))
        assert dm.last_grid() != 3
        assert T.equal(dm.frame_tile(tiles), c([T.cat([T.cat([picture(T, (1, 16, 16), 7), picture(T, (1, 16, 13), 8)], 2),
                                                        T.cat([picture(T, (1, 11, 16), 9), picture(T, (1, 11, 13), 10)], 2)], 1)]))
