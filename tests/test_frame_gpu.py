"""GPU: the container "frame v1" (dct_amd.frame_pack / frame_unpack / compress / decompress) and
the two conversions under it (dctq_block_lengths, dctq_block_offsets).

The yardsticks: numpy for the conversions (tools/frame_ref.py lengths_from_offsets /
offsets_from_lengths), tools/frame_ref.py pack / parse for the container byte for byte, and the
uncontained decode -- Plan.decode_bits (+ ycbcr_to_rgb) of the stream with its true offsets and
var_nums -- for the pixels, bit for bit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frame_ref  # noqa: E402

SENTINEL = 0xA5
EINVAL = -1
MAX_BLOCKS = 11_671_106
# tile (64 blocks) and 8192-tile scan-segment boundaries
NBLOCKS = [1, 63, 64, 65, 8191 * 64 + 1, 524288, 524289, 1048577]


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


@functools.lru_cache(maxsize=None)
def random_lengths(n, width):
    """Mostly what a stream holds (0..368), some above the clamp; the last block never empty."""
    rng = np.random.default_rng(1000 * width + n % 997)
    ln = rng.integers(0, 256 if width == 1 else 369, n)
    if width == 2:
        big = rng.integers(0, n, max(1, n // 50))
        ln[big] = rng.integers(369, 65536, big.size)
    ln[-1] = max(int(ln[-1]), 1)
    return ln


# ---- 1. lengths -> offsets ------------------------------------------------------------------------------------
def raw_offsets(dm, T, lengths, lb, n=None, out="ok", ws="ok", lengths_ptr="ok"):
    """dctq_block_offsets as a C host calls it.  Returns (rc, offsets tensor with two sentinels after).  ws: "ok",
    None (NULL) or a number of bytes to add to the workspace's address."""
    L = dm.lib()
    n = lengths.numel() if n is None else n
    off = T.full((lengths.numel() + 3,), -1, dtype=T.int32, device="cuda")
    wsp = T.empty(int(L.dctq_block_offsets_workspace_bytes(lengths.numel())) // 4 + 2, dtype=T.int32, device="cuda")
    rc = L.dctq_block_offsets(C.c_void_p(lengths.data_ptr()) if lengths_ptr == "ok" else None, lb, n,
                              C.c_void_p(off.data_ptr()) if out == "ok" else None,
                              None if ws is None else C.c_void_p(wsp.data_ptr() + (0 if ws == "ok" else ws)), None)
    T.cuda.synchronize()
    return rc, off


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("n", NBLOCKS)
def test_block_offsets_against_numpy(T, dm, n, width):
    ln = random_lengths(n, width)
    want = frame_ref.offsets_from_lengths(ln)
    g = gpu(T, ln.astype(np.uint8 if width == 1 else np.uint16).view(np.uint8 if width == 1 else np.int16))
    rc, off = raw_offsets(dm, T, g, width)
    assert rc == 0
    got = u32(off)
    assert np.array_equal(got[:n + 1], want), np.flatnonzero(got[:n + 1] != want)[:8]
    assert (got[n + 1:] == 0xFFFFFFFF).all(), "written past offsets[nblocks]"
    assert np.array_equal(u32(dm.block_offsets(g)), want)
    if width == 2 and hasattr(T, "uint16"):
        assert np.array_equal(u32(dm.block_offsets(g.view(T.uint16))), want)


def test_block_offsets_clamps_every_length(T, dm):
    n = NBLOCKS[-1]
    got = u32(dm.block_offsets(T.full((n,), -1, dtype=T.int16, device="cuda")))  # 65535 everywhere
    assert np.array_equal(got, 368 * np.arange(n + 1, dtype=np.uint32)) and int(got[-1]) == 368 * n


# ---- 2. offsets -> lengths ------------------------------------------------------------------------------------
def raw_lengths(dm, T, off, lb, n=None, out="ok", mx="ok", offsets="ok"):
    """dctq_block_lengths as a C host calls it.  Returns (rc, the length bytes with 16 sentinel bytes after the
    last entry, max_length)."""
    L = dm.lib()
    nn = off.numel() - 1
    n = nn if n is None else n
    buf = T.full((nn * lb + 16,), SENTINEL, dtype=T.uint8, device="cuda")
    m = T.full((1,), 0x5A5A5A5A, dtype=T.int32, device="cuda")  # no initialisation needed
    rc = L.dctq_block_lengths(C.c_void_p(off.data_ptr()) if offsets == "ok" else None, n, lb,
                              C.c_void_p(buf.data_ptr()) if out == "ok" else None,
                              C.c_void_p(m.data_ptr()) if mx == "ok" else None, None)
    T.cuda.synchronize()
    return rc, buf, int(m.item()) & 0xFFFFFFFF


def check_lengths(dm, T, off_np, lb):
    """One call on offsets off_np (uint32 [N + 1]) against numpy: entries, maximum, nothing written after."""
    n = len(off_np) - 1
    want = frame_ref.lengths_from_offsets(off_np)
    rc, buf, mx = raw_lengths(dm, T, gpu(T, off_np.view(np.int32)), lb)
    assert rc == 0
    raw = buf.cpu().numpy()
    got = raw[:n * lb].view(np.uint8 if lb == 1 else np.uint16)
    sat = np.minimum(want, 255 if lb == 1 else 65535)
    assert np.array_equal(got, sat), np.flatnonzero(got != sat)[:8]
    assert mx == int(want.max()), (mx, int(want.max()))
    assert (raw[n * lb:] == SENTINEL).all(), "a byte after the last length was written"
    return want


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("n", NBLOCKS)
def test_block_lengths_against_numpy(T, dm, n, width):
    """Width 1 on lengths up to 368: u8 saturates at 255, max_length is the true maximum."""
    ln = np.minimum(random_lengths(n, 2), 368)
    off = frame_ref.offsets_from_lengths(ln)
    want = check_lengths(dm, T, off, width)
    assert np.array_equal(want, ln)
    if width == 2:  # max <= 368: the two conversions are inverses, and the wrapper picks the width
        g = gpu(T, off.view(np.int32))
        lengths, lb = dm.block_lengths(g)
        assert lb == (1 if ln.max() <= 255 else 2) and lengths.dtype == (T.uint8 if lb == 1 else T.int16)
        assert T.equal(dm.block_offsets(lengths), g)
        if ln.max() > 255:
            with pytest.raises(dm.DctqError):
                dm.block_lengths(g, 1)


@pytest.mark.parametrize("n", [5, 65, 130])
def test_block_lengths_saturation(T, dm, n):
    rng = np.random.default_rng(n)
    ln = rng.integers(0, 300, n)
    ln[n // 2] = 70000  # above u16
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    for lb in (1, 2):
        check_lengths(dm, T, off, lb)
    with pytest.raises(dm.DctqError):
        dm.block_lengths(gpu(T, off.view(np.int32)))
    # a decreasing pair: the difference mod 2^32 saturates, and the maximum says so
    ln[0], ln[n // 2] = 10, 7
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    off[n // 2 + 1] = off[n // 2] - 1
    want = frame_ref.lengths_from_offsets(off)
    assert want.max() == 2 ** 32 - 1
    for lb in (1, 2):
        check_lengths(dm, T, off, lb)
    with pytest.raises(dm.DctqError):
        dm.block_lengths(gpu(T, off.view(np.int32)))
    with pytest.raises(dm.DctqError):
        dm.block_lengths(gpu(T, off.view(np.int32)), 2)


def test_refusals_of_the_c_entry_points(T, dm):
    off = gpu(T, frame_ref.offsets_from_lengths(np.arange(1, 70)).view(np.int32))
    n = off.numel() - 1
    bad = {"NULL offsets": dict(offsets=None), "NULL lengths": dict(out=None), "NULL max_length": dict(mx=None),
           "nblocks 0": dict(n=0), "nblocks -1": dict(n=-1), "nblocks past the limit": dict(n=MAX_BLOCKS + 1)}
    for what, kw in bad.items():
        rc, buf, _ = raw_lengths(dm, T, off, 1, **kw)
        assert rc == EINVAL, what
        assert bool((buf == SENTINEL).all()), what
    for lb in (0, 3, 4, -1):
        L = dm.lib()
        m = T.zeros(1, dtype=T.int32, device="cuda")
        buf = T.full((n * 4,), SENTINEL, dtype=T.uint8, device="cuda")
        assert L.dctq_block_lengths(C.c_void_p(off.data_ptr()), n, lb, C.c_void_p(buf.data_ptr()),
                                    C.c_void_p(m.data_ptr()), None) == EINVAL, lb
        T.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), lb
    lengths = T.ones(n, dtype=T.uint8, device="cuda")
    bad = {"NULL lengths": dict(lengths_ptr=None), "NULL offsets": dict(out=None), "NULL workspace": dict(ws=None),
           "workspace + 1": dict(ws=1), "workspace + 2": dict(ws=2),
           "nblocks 0": dict(n=0), "nblocks past the limit": dict(n=MAX_BLOCKS + 1)}
    for what, kw in bad.items():
        rc, o = raw_offsets(dm, T, lengths, 1, **kw)
        assert rc == EINVAL, what
        assert bool((o == -1).all()), what
    for lb in (0, 3, 4):
        rc, o = raw_offsets(dm, T, lengths, lb)
        assert rc == EINVAL and bool((o == -1).all()), lb


# ---- 3. the container, round trips ------------------------------------------------------------------------
F, H, W = 2, 64, 80  # 4:2:0: Y 160 blocks, Cb and Cr 40 each: 240, more than three tiles' worth of lanes
PLANS = [(50, False), (50, True), (95, False)]


def picture(T, dm):
    """Frame 0 smooth, frame 1 noise, the channels different."""
    rgb = T.stack([T.stack([dm.synth(11 + c, "smooth", W, H)[0] for c in range(3)], -1),
                   T.stack([dm.synth(21 + c, "uniform", W, H)[0] for c in range(3)], -1)])
    assert rgb.shape == (F, H, W, 3)
    return rgb.contiguous()


def uncontained(T, dm, planes, q, adaptive):
    """The stream of `planes` as the library's users held it before: (bytes, offsets, var_nums, decoded planes)."""
    plan = dm.Plan(q, adaptive)
    vns = None
    if adaptive:
        nbs = [p.shape[0] * (p.shape[1] // 8) * (p.shape[2] // 8) for p in planes]
        vns = [T.empty(n, dtype=T.int32, device="cuda") for n in nbs]
        coefs = plan.forward_quant_planes(planes, var_nums=vns)
        off, sym = dm.rle_encode(T.cat(coefs))
        by, boff = dm.bits_pack(sym, off)
    else:
        _, boff, by = plan.encode_bits_planes(planes)
    dec = plan.decode_bits(by, boff, shapes=[tuple(p.shape) for p in planes], var_nums=vns)
    return by, boff, vns, dec


def host_bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("q,adaptive", PLANS)
def test_round_trip_rgb(T, dm, q, adaptive):
    rgb = picture(T, dm)
    planes = list(dm.rgb_to_ycbcr(rgb, "420"))
    shapes = [tuple(p.shape) for p in planes]
    assert [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes] == [160, 40, 40]
    by, boff, vns, dec = uncontained(T, dm, planes, q, adaptive)
    want = dm.ycbcr_to_rgb(*dec)
    box = dm.compress(rgb, q, adaptive)
    assert box.dtype == T.uint8 and box.is_cuda and box.dim() == 1
    ref = frame_ref.pack(by.cpu().numpy(), u32(boff), shapes, q, adaptive,
                         None if vns is None else [v.cpu().numpy() for v in vns], colour=True)
    print(f"q{q} a{int(adaptive)}: container {len(ref)} B, payload {by.numel()} B, N {boff.numel() - 1}")
    assert host_bytes(box) == ref, "the container differs from tools/frame_ref.py pack"
    assert T.equal(dm.decompress(host_bytes(box)), want)      # from the host, nothing else remembered
    assert T.equal(dm.decompress(box), want)                  # from the device
    assert T.equal(dm.decompress(bytearray(ref)), want)       # a container packed on the host
    assert T.equal(dm.decompress(np.frombuffer(ref, np.uint8)), want)
    got4 = dm.decompress(box, channels=4, bgr=True)
    assert T.equal(got4[..., :3].flip(-1), want) and bool((got4[..., 3] == 255).all())
    d = dm.frame_unpack(box)
    assert (d["quality"], d["adaptive"], d["colour"], d["shapes"]) == (q, adaptive, True, shapes)
    assert T.equal(d["offsets"], boff) and T.equal(d["bytes"], by)
    assert (d["var_nums"] is None) if not adaptive else all(T.equal(a, b) for a, b in zip(d["var_nums"], vns))
    assert d["bytes"].data_ptr() >= box.data_ptr() and d["bytes"].data_ptr() < box.data_ptr() + box.numel(), "a view"


@pytest.mark.parametrize("q,adaptive", PLANS)
def test_round_trip_plain_planes(T, dm, q, adaptive):
    planes = [dm.synth(5, "smooth", 40, 24, 2), dm.synth(6, "uniform", 72, 16, 1)]  # 30 + 18 blocks
    shapes = [tuple(p.shape) for p in planes]
    by, boff, vns, dec = uncontained(T, dm, planes, q, adaptive)
    box = dm.compress(planes, q, adaptive)
    ref = frame_ref.pack(by.cpu().numpy(), u32(boff), shapes, q, adaptive,
                         None if vns is None else [v.cpu().numpy() for v in vns])
    assert host_bytes(box) == ref
    for source in (host_bytes(box), box, ref):
        got = dm.decompress(source)
        assert isinstance(got, list) and len(got) == 2
        assert all(T.equal(a, b) for a, b in zip(got, dec))
    assert not dm.frame_unpack(box)["colour"]


def test_444_and_clamped_quality(T, dm):
    rgb = picture(T, dm)
    box = dm.compress(rgb, 1000, subsampling="444")
    d = dm.frame_unpack(box)
    assert d["quality"] == 100 and d["shapes"] == [(F, H, W)] * 3 and d["colour"]
    planes = list(dm.rgb_to_ycbcr(rgb, "444"))
    _, _, _, dec = uncontained(T, dm, planes, 100, False)
    assert T.equal(dm.decompress(box), dm.ycbcr_to_rgb(*dec))


# ---- 4. two bytes of length -------------------------------------------------------------------------------
def test_width_two_through_the_whole_path(T, dm):
    """A foreign symbol stream whose blocks exceed 255 B: (-32768, 64) x 64 packs to 368 B."""
    rng = np.random.default_rng(3)
    blocks = [[(-32768, 64)] * 64 if b % 3 == 0 else [(int(rng.integers(-9, 10)), 0)] * int(rng.integers(1, 64))
              for b in range(70)]
    sym = np.array([(v & 0xFFFF) | (r << 16) for b in blocks for v, r in b], np.uint32)
    off = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    by, boff = dm.bits_pack(gpu(T, sym.view(np.int32)), gpu(T, off.view(np.int32)))
    sizes = np.diff(u32(boff).astype(np.int64))
    assert sizes.max() == 368 and sizes.min() < 255
    shapes = [(1, 8, 8 * 70)]
    box = dm.frame_pack(by, boff, shapes, 50)
    assert host_bytes(box) == frame_ref.pack(by.cpu().numpy(), u32(boff), shapes, 50)
    d = dm.frame_unpack(box)
    assert d["length_bytes"] == 2 and frame_ref.parse(host_bytes(box))["length_bytes"] == 2
    assert T.equal(d["offsets"], boff) and T.equal(d["bytes"], by)
    plan = dm.Plan(50, False)
    assert T.equal(dm.decompress(box)[0], plan.decode_bits(by, boff, shapes=shapes)[0])


# ---- 5. hostile input -----------------------------------------------------------------------------------------
def test_every_refusal(T, dm):
    planes = [dm.synth(5, "smooth", 40, 24, 2)]
    for adaptive in (False, True):
        good = host_bytes(dm.compress(planes, 50, adaptive))
        assert frame_ref.parse(good)["length_bytes"] == 1
        dm.frame_unpack(good)
        for rule, bad in frame_ref.refusal_cases(good):
            with pytest.raises(frame_ref.FrameError):
                frame_ref.parse(bad)
            with pytest.raises(dm.DctqError):
                dm.frame_unpack(bad)
                pytest.fail(f"frame_unpack accepted: {rule}")
            with pytest.raises(dm.DctqError):
                dm.frame_unpack(gpu(T, np.frombuffer(bad, np.uint8).copy()))
                pytest.fail(f"frame_unpack accepted on the device: {rule}")
    # colour claimed for planes that are no Y, Cb, Cr
    two = bytearray(host_bytes(dm.compress([planes[0], planes[0]], 50)))
    two[16] = 1
    with pytest.raises(dm.DctqError):
        dm.frame_unpack(two)
    with pytest.raises(dm.DctqError):
        dm.frame_unpack(T.zeros(100, dtype=T.uint8))  # a host tensor is no device tensor


def test_nothing_is_decoded_from_a_refused_container(T, dm):
    rgb = picture(T, dm)
    box = dm.compress(rgb, 50)
    good = host_bytes(box)
    out = dm.decompress(good)
    d = dm.frame_unpack(box)
    keep = out.clone()
    bad = bytearray(good)
    at = frame_ref.align16(48 + 16 * 3) + 100  # one length, one more
    assert bad[at] < 255
    bad[at] += 1
    with pytest.raises(dm.DctqError, match="sum"):
        dm.decompress(bad)
    with pytest.raises(dm.DctqError, match="sum"):
        dm.decompress(gpu(T, np.frombuffer(bytes(bad), np.uint8).copy()))
    T.cuda.synchronize()
    assert T.equal(out, keep) and T.equal(d["bytes"], dm.frame_unpack(good)["bytes"])
    bad[at] -= 2  # ... and one less
    with pytest.raises(dm.DctqError, match="sum"):
        dm.decompress(bad)


def test_misaligned_device_views(T, dm):
    rgb = picture(T, dm)
    for q, adaptive in PLANS[:2]:
        box = dm.compress(rgb, q, adaptive)
        want = dm.decompress(box)
        for lead in (1, 2, 4, 8, 15):
            padded = T.full((lead + box.numel() + 16,), SENTINEL, dtype=T.uint8, device="cuda")
            padded[lead:lead + box.numel()] = box
            view = padded[lead:lead + box.numel()]
            assert view.data_ptr() % 16 == lead
            assert T.equal(dm.decompress(view), want), lead
            assert T.equal(dm.decompress(padded[lead:]), want), lead  # bytes after the container are not its own
            assert T.equal(padded[lead:lead + box.numel()], box)


# ---- 6. the measuring tool -----------------------------------------------------------------------------------
def test_frame_ab_tool_runs(T):
    """tools/frame_ab.py gates on equality; here on two small frames (profiles/r13/frame_ab.log: the bench step's)."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "frame_ab.py"), "--frames", "2", "--width", "256",
                          "--height", "144", "--rounds", "1", "--launches", "1"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "equality in every pass: PASS" in out.stdout and out.stdout.count("every pixel equal: True") == 3
