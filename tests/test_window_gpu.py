"""GPU: random access into a "bits v1" stream -- dctq_decode_bits_window_planes,
Plan.decode_bits_window and decompress(region=, frames=).

The yardstick is always the full Plan.decode_bits (pinned to tools/bits_ref.py and the oracle by
the rest of the suite), sliced: a window must equal that slice bit for bit, for any bytes.  Two
more properties catch a wrong block mapping that an equal result could hide: payload bytes of
every block that tools/window_ref.py puts in no run may be overwritten without changing the
window (only the window is read), and every byte of a strided destination outside the window's
pixels keeps its sentinel.

Stored picture set: 4:2:0 planes (2, 32, 1056) + 2 x (2, 16, 528): 132 x 4 and 66 x 2 blocks per
frame, 1 584 in all.  The most runs one call over this set can have is 40 (the whole planes: 3
runs per luma row, 2 per chroma row), so the grid-limit case uses the whole planes: 40 runs
over the 4 waves of one workgroup and the 12 of three are at least 3 runs per wave in both.

What a case can show depends on its plan.  The non-adaptive inverse multiplies a coefficient by
1 / Q, as the reference's dequantization does, so below q100 its pictures stay within a level or
two of 128 and say little about WHERE a block landed; at q100 (Q = 1) and on adaptive plans
(which multiply by Q) the decoded pictures span the whole range.  The sweep keeps every plan
the issue lists, asserts that range where it exists, and the poison, sentinel and grid-limit
cases use such plans."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import window_ref  # noqa: E402

SHAPES = [(2, 32, 1056), (2, 16, 528), (2, 16, 528)]
NBS = [f * (h // 8) * (w // 8) for f, h, w in SHAPES]
SENTINEL = 0xA5
STAGE = 2560  # bits_core.h kBitsStage: a half of 32 blocks beyond it takes several chunks
ALL = [((0, f), (0, h), (0, w)) for f, h, w in SHAPES]


def blk(f, y, x):
    """Block ranges -> a window in frames and pixels."""
    return (f, (8 * y[0], 8 * y[1]), (8 * x[0], 8 * x[1]))


WINDOWS = {
    "whole": ALL,
    "last block": [blk((1, 2), (3, 4), (131, 132)), blk((1, 2), (1, 2), (65, 66)), blk((1, 2), (1, 2), (65, 66))],
    "first block": [blk((0, 1), (0, 1), (0, 1))] * 3,
    "65 from 1": [blk((0, 2), (0, 4), (1, 66)), blk((0, 2), (0, 2), (1, 66)), blk((0, 2), (0, 2), (1, 66))],
    "31 wide": [blk((0, 2), (0, 4), (2, 33)), blk((0, 2), (0, 2), (2, 33)), blk((0, 2), (0, 2), (2, 33))],
    "32 wide": [blk((0, 2), (0, 4), (2, 34)), blk((0, 2), (0, 2), (2, 34)), blk((0, 2), (0, 2), (2, 34))],
    "33 wide": [blk((0, 2), (0, 4), (2, 35)), blk((0, 2), (0, 2), (2, 35)), blk((0, 2), (0, 2), (2, 35))],
    "frame 1": [((1, 2), (0, h), (0, w)) for _, h, w in SHAPES],
    "rows 1..3": [blk((0, 2), (1, 4), (0, 132)), blk((0, 2), (1, 2), (0, 66)), blk((0, 2), (1, 2), (0, 66))],
    "unrelated": [blk((1, 2), (1, 4), (1, 66)), blk((1, 2), (0, 2), (0, 33)), blk((0, 1), (1, 2), (65, 66))],
}


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
def stream_of(kind, q, adaptive):
    """The stored set's packed stream, its var_nums, and the full decode: (bytes, offsets, var_nums, full)."""
    import dct_amd
    import torch
    plan = plan_of(q, adaptive)
    planes = [dct_amd.synth(900 + k, kind, s[2], s[1], s[0]) for k, s in enumerate(SHAPES)]
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in NBS]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, boff, by = plan.encode_bits_planes(planes)
    vns = vns if adaptive else None
    full = plan.decode_bits(by, boff, shapes=SHAPES, var_nums=vns)
    torch.cuda.synchronize()
    return by, boff, vns, full


def cut(full, windows):
    return [p[f0:f1, y0:y1, x0:x1] for p, ((f0, f1), (y0, y1), (x0, x1)) in zip(full, windows)]


def assert_windows_equal(T, got, full, windows, what):
    for k, (g, w) in enumerate(zip(got, cut(full, windows))):
        assert g.dtype == T.uint8 and tuple(g.shape) == tuple(w.shape), (what, k, tuple(g.shape), tuple(w.shape))
        assert T.equal(g, w), (what, f"plane {k}", int((g != w).sum()), "pixels differ")


# ---- 1. every window, content and plan ----------------------------------------------------------------
def test_the_plans_cover_both_inverses(dm):
    admitted = {q: dm.inverse_bound(q, False)[1] for q in (10, 50, 100)}
    assert set(admitted.values()) == {True, False}, admitted  # the fp32 and the fp64 inverse both run below


def test_dense_halves_exceed_the_stage(T, dm):
    """At q100 a 32-block half of noise is beyond the 2 560 B stage, so the chunk loop runs, and in
    the windows that start at block column 1 or 2 from a start that is no tile's."""
    s0 = window_ref.runs(SHAPES, WINDOWS["65 from 1"])[0][0]
    for kind in ("uniform", "extreme", "smooth"):
        off = u32(stream_of(kind, 100, 0)[1]).astype(np.int64)
        print(f"{kind} q100: the first half of the run at block {s0} is {off[s0 + 32] - off[s0]} B")
    off = u32(stream_of("uniform", 100, 0)[1]).astype(np.int64)
    assert s0 % 64 and off[s0 + 32] - off[s0] > STAGE, off[s0 + 32] - off[s0]


@pytest.mark.parametrize("adaptive", [0, 1])
@pytest.mark.parametrize("q", [10, 50, 100])
@pytest.mark.parametrize("kind", ["smooth", "uniform", "extreme"])
def test_window_equals_slice(T, dm, kind, q, adaptive):
    by, boff, vns, full = stream_of(kind, q, adaptive)
    plan = plan_of(q, adaptive)
    if adaptive or q == 100:  # a picture in which a misplaced block shows
        assert all(int(p.max()) - int(p.min()) > 128 for p in full), [(int(p.min()), int(p.max())) for p in full]
    for name, windows in WINDOWS.items():
        got = plan.decode_bits_window(by, boff, SHAPES, windows, var_nums=vns)
        assert_windows_equal(T, got, full, windows, (kind, q, adaptive, name))
    whole = plan.decode_bits_window(by, boff, SHAPES, ALL, var_nums=vns)
    assert all(T.equal(a, b) for a, b in zip(whole, full))


def test_runs_never_start_on_a_tile(dm):
    r = window_ref.runs(SHAPES, WINDOWS["65 from 1"])
    assert sorted(set(r[:, 1].tolist())) == [1, 64] and all(s0 % 64 for s0 in r[:, 0]), r.tolist()


# ---- 2. any bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [0, 1])
def test_foreign_bytes(T, dm, adaptive):
    """Random payload behind random non-decreasing offsets: lengths 0..400, so empty blocks and
    blocks above the format's 368 B both occur."""
    rng = np.random.default_rng(17 + adaptive)
    n = sum(NBS)
    lengths = rng.integers(0, 401, n)
    lengths[rng.integers(0, n, 40)] = 0
    assert (lengths > 368).any() and (lengths == 0).any()
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    by = T.from_numpy(rng.integers(0, 256, int(off[-1]), dtype=np.uint8)).cuda()
    boff = T.from_numpy(off.view(np.int32)).cuda()
    vns = stream_of("uniform", 50, 1)[2] if adaptive else None
    plan = plan_of(50, adaptive)
    full = plan.decode_bits(by, boff, shapes=SHAPES, var_nums=vns)
    assert any(int(p.min()) != int(p.max()) for p in full)
    for name, windows in WINDOWS.items():
        got = plan.decode_bits_window(by, boff, SHAPES, windows, var_nums=vns)
        assert_windows_equal(T, got, full, windows, ("foreign", adaptive, name))


# ---- 3. only the window is read ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,q,adaptive", [("smooth", 50, 1), ("uniform", 100, 0), ("extreme", 10, 1)])
def test_only_the_window_is_read(T, dm, kind, q, adaptive):
    """The payload of every block that window_ref puts in no run is overwritten (offsets
    unchanged): the window is what it was, and the full decode is not."""
    by, boff, vns, full = stream_of(kind, q, adaptive)
    plan = plan_of(q, adaptive)
    off = u32(boff).astype(np.int64)
    host = by.cpu().numpy()
    for name, windows in WINDOWS.items():
        if name == "whole":
            continue
        out = window_ref.outside(SHAPES, windows)
        keep = np.ones(host.size, dtype=bool)
        for b in out:
            keep[off[b]:off[b + 1]] = False
        inside = np.concatenate([b.ravel() for b in window_ref.blocks(SHAPES, windows)])
        assert len(out) + len(inside) == sum(NBS) and all(keep[off[b]:off[b + 1]].all() for b in inside)
        poisoned = T.from_numpy(np.where(keep, host, host ^ 0xFF)).cuda()
        got = plan.decode_bits_window(poisoned, boff, SHAPES, windows, var_nums=vns)
        assert_windows_equal(T, got, full, windows, (kind, q, name, "poisoned outside"))
        spoiled = plan.decode_bits(poisoned, boff, shapes=SHAPES, var_nums=vns)
        assert any(not T.equal(a, b) for a, b in zip(spoiled, full)), (name, "the poison changed nothing")


# ---- 4. destinations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65 from 1", "33 wide", "unrelated", "last block"])
def test_strided_outs_keep_their_padding(T, dm, name):
    by, boff, vns, full = stream_of("uniform", 50, 1)
    windows = WINDOWS[name]
    bufs, outs = [], []
    for (f0, f1), (y0, y1), (x0, x1) in windows:
        b = T.full((f1 - f0, y1 - y0 + 3, x1 - x0 + 24), SENTINEL, dtype=T.uint8, device="cuda")
        bufs.append(b)
        outs.append(b[:, :y1 - y0, :x1 - x0])
    got = plan_of(50, 1).decode_bits_window(by, boff, SHAPES, windows, outs=outs, var_nums=vns)
    assert all(g is o for g, o in zip(got, outs))
    assert_windows_equal(T, got, full, windows, (name, "strided"))
    for b, ((f0, f1), (y0, y1), (x0, x1)) in zip(bufs, windows):
        assert bool((b[:, y1 - y0:, :] == SENTINEL).all()) and bool((b[:, :, x1 - x0:] == SENTINEL).all()), name


def test_side_stream(T, dm):
    by, boff, _, full = stream_of("smooth", 100, 0)
    windows = WINDOWS["unrelated"]
    assert all(int(p.max()) - int(p.min()) > 128 for p in cut(full, windows)[:2])
    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    outs = [T.zeros((f1 - f0, y1 - y0, x1 - x0), dtype=T.uint8, device="cuda")
            for (f0, f1), (y0, y1), (x0, x1) in windows]
    T.cuda.synchronize()
    got = plan_of(100, 0).decode_bits_window(by, boff, SHAPES, windows, outs=outs, stream=s)
    s.synchronize()
    dm.stream_release(s)
    assert_windows_equal(T, got, full, windows, "side stream")


@pytest.mark.parametrize("q,adaptive", [(100, 0), (50, 1)])
def test_grid_limits(T, dm, q, adaptive):
    """Every wave takes several runs: 40 runs over 4 and over 12 waves."""
    by, boff, vns, full = stream_of("uniform", q, adaptive)
    nruns = len(window_ref.runs(SHAPES, ALL))
    assert nruns == 40 and nruns // 4 >= 3 and nruns // 12 >= 3
    for name in ("whole", "65 from 1"):
        windows = WINDOWS[name]
        want = plan_of(q, adaptive).decode_bits_window(by, boff, SHAPES, windows, var_nums=vns)
        for limit in (1, 3):
            T.cuda.synchronize()
            with dm.grid_limit(limit):
                got = dm.Plan(q, adaptive).decode_bits_window(by, boff, SHAPES, windows, var_nums=vns)
                grid = dm.last_grid()
            T.cuda.synchronize()
            assert grid == limit, (name, limit, grid, "the limit did not reach the launch")
            assert all(T.equal(g, w) for g, w in zip(got, want)), (name, limit)
            assert_windows_equal(T, got, full, windows, (name, "limit", limit))


# ---- 5. what the wrapper and the library refuse ----------------------------------------------------------
def test_refusals(T, dm):
    by, boff, vns, _ = stream_of("uniform", 50, 1)
    plan, aplan = plan_of(50, 0), plan_of(50, 1)
    ok = WINDOWS["unrelated"]
    bad = [
        [((0, 3), (0, 32), (0, 1056))] + ok[1:],      # a frame range that leaves the stored frames
        [((1, 1), (0, 32), (0, 1056))] + ok[1:],      # empty
        [((0, 1), (0, 40), (0, 1056))] + ok[1:],      # leaves the plane
        [((0, 1), (0, 32), (8, 1064))] + ok[1:],
        [((0, 1), (4, 12), (0, 8))] + ok[1:],         # not whole blocks
        [((0, 1), (0, 8), (-8, 8))] + ok[1:],
        ok[:2],                                        # one window short
    ]
    for windows in bad:
        with pytest.raises(dm.DctqError):
            plan.decode_bits_window(by, boff, SHAPES, windows)
    with pytest.raises(dm.DctqError):
        aplan.decode_bits_window(by, boff, SHAPES, ok)  # adaptive without var_nums
    with pytest.raises(dm.DctqError):
        plan.decode_bits_window(by, boff[:-1], SHAPES, ok)
    with pytest.raises(dm.DctqError):
        plan.decode_bits_window(by, boff, SHAPES, ok, outs=[T.empty((1, 8, 8), dtype=T.uint8, device="cuda")] * 3)
    # the library itself: a missing var_num on an adaptive plan is refused before any launch
    import ctypes as C
    outs = [T.full((f1 - f0, y1 - y0, x1 - x0), SENTINEL, dtype=T.uint8, device="cuda")
            for (f0, f1), (y0, y1), (x0, x1) in ok]
    descs = (dm._Plane * 3)(*[dm.plane_desc(o) for o in outs])
    wins = (dm._Window * 3)(*[dm._Window(w, h, f, x0, y0, f0)
                              for (f, h, w), ((f0, _), (y0, _), (x0, _)) in zip(SHAPES, ok)])
    L = dm.lib()
    ptrs = (C.c_void_p * 3)(vns[0].data_ptr(), None, vns[2].data_ptr())
    for vp in (None, C.cast(ptrs, C.c_void_p)):
        rc = L.dctq_decode_bits_window_planes(aplan._h, C.c_void_p(by.data_ptr()), C.c_void_p(boff.data_ptr()), vp,
                                              wins, descs, 3, None)
        assert rc == -1, rc
    T.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)


# ---- 6. decompress(region=, frames=) ---------------------------------------------------------------------------
def rgb_picture(T, dm, f, h, w, kind="smooth"):
    """An RGB stack [f, h, w, 3] of synthetic content."""
    p = dm.synth(4242, kind, -(-3 * w // 4) * 4, h, f)   # synth takes widths that are multiples of 4
    return p[:, :, :3 * w].reshape(f, h, w, 3).contiguous()


@functools.lru_cache(maxsize=None)
def container(case):
    import dct_amd as dm
    import torch as T
    if case == "420":
        buf = dm.compress(rgb_picture(T, dm, 2, 64, 1056), 100)
    elif case == "444":
        buf = dm.compress(rgb_picture(T, dm, 2, 40, 136, "uniform"), 100, subsampling="444")
    elif case == "c1":
        buf = dm.compress(rgb_picture(T, dm, 2, 70, 1050), 100)
    elif case == "adaptive":
        buf = dm.compress(rgb_picture(T, dm, 2, 70, 1050, "uniform"), 50, adaptive=True)
    elif case == "planes":
        buf = dm.compress([dm.synth(5, "smooth", 1056, 32, 2), dm.synth(6, "uniform", 100, 27, 2)], 100)
    elif case == "planes one size":
        buf = dm.compress([dm.synth(7, "smooth", 204, 45, 3)[:, :, :203], dm.synth(8, "uniform", 204, 45, 3)[:, :, :203]],
                          75, adaptive=True)
    whole = dm.decompress(buf)
    T.cuda.synchronize()
    # q100 or adaptive (see the module's docstring): pictures in which a misplaced block shows
    assert all(int(p.max()) - int(p.min()) > 128 for p in (whole if isinstance(whole, list) else [whole]))
    return buf, whole


PICTURES = {
    "420": (2, 64, 1056), "444": (2, 40, 136), "c1": (2, 70, 1050), "adaptive": (2, 70, 1050),
}


def regions_of(h, w):
    return [((0, h), (0, w)), ((16, 32), (32, 96)), ((h - 9, h), (w - 13, w)), ((3, 38), (5, 122)),
            ((1, 2), (7, 8)), ((0, 17), (w - 1, w))]


@pytest.mark.parametrize("case", list(PICTURES))
def test_decompress_region_of_a_picture(T, dm, case):
    buf, whole = container(case)
    f, h, w = PICTURES[case]
    assert tuple(whole.shape) == (f, h, w, 3)
    for region in regions_of(h, w):
        (y0, y1), (x0, x1) = region
        for frames in (None, (1, 2), (0, 1)):
            f0, f1 = frames or (0, f)
            got = dm.decompress(buf, region=region, frames=frames)
            assert T.equal(got, whole[f0:f1, y0:y1, x0:x1]), (case, region, frames)
    assert T.equal(dm.decompress(buf, frames=(1, 2)), whole[1:2])
    got = dm.decompress(buf, channels=4, bgr=True, region=((3, 38), (5, 122)))
    assert T.equal(got, dm.decompress(buf, channels=4, bgr=True)[:, 3:38, 5:122])
    got = dm.decompress(buf, planar=True, region=((3, 38), (5, 122)), frames=(1, 2))
    assert T.equal(got, whole[1:2, 3:38, 5:122])


def test_decompress_regions_of_plain_planes(T, dm):
    buf, whole = container("planes")
    regions = [((9, 30), (100, 1001)), ((0, 27), (93, 100))]
    got = dm.decompress(buf, region=regions, frames=(1, 2))
    for g, p, ((y0, y1), (x0, x1)) in zip(got, whole, regions):
        assert T.equal(g, p[1:2, y0:y1, x0:x1])
    got = dm.decompress(buf, frames=(0, 1))
    assert all(T.equal(g, p[0:1]) for g, p in zip(got, whole))
    with pytest.raises(dm.DctqError):
        dm.decompress(buf, region=((0, 8), (0, 8)))   # the planes differ in size: one region says too little
    with pytest.raises(dm.DctqError):
        dm.decompress(buf, region=regions[:1])
    buf, whole = container("planes one size")
    got = dm.decompress(buf, region=((44, 45), (1, 203)), frames=(2, 3))
    assert all(T.equal(g, p[2:3, 44:45, 1:203]) for g, p in zip(got, whole))


def test_decompress_refusals_decode_nothing(T, dm, monkeypatch):
    buf, whole = container("c1")
    calls = []
    for name in ("decode_bits", "decode_bits_window"):
        monkeypatch.setattr(dm.Plan, name, lambda self, *a, **k: calls.append(1))
    for kw in ({"region": ((0, 71), (0, 8))}, {"region": ((0, 8), (0, 1051))}, {"region": ((5, 5), (0, 8))},
               {"region": ((-1, 8), (0, 8))}, {"frames": (0, 3)}, {"frames": (1, 1)}, {"region": ((0, 8),)},
               {"region": [((0, 8), (0, 8))] * 3}, {"region": 7}):
        with pytest.raises(dm.DctqError):
            dm.decompress(buf, **kw)
    bad = buf.clone()
    bad[0] = 0
    with pytest.raises(dm.DctqError):
        dm.decompress(bad, region=((0, 8), (0, 8)))
    assert not calls
