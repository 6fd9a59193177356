"""GPU: exact rounding ties at AC coefficients and adaptive divisors (tools/pixel_families.py)
through every kernel that resolves ties, bit-exact against the oracle.

At a true tie (the real quotient is exactly k + 0.5) the reference's own fp64 noise decides the
side -- against round-half-away for 80 % of the ties built here -- so only there do the exact
paths' summation order, row/column roles and divisor formula show.  The DC, where every tie of
the older tests sits, has equal DCT rows, keeps Q under adaptive plans and is one flag slot;
these planes tie at (0,4), (4,0), (4,4) too, up to four entries per lane, and their transposes
swap the roles of rows and columns.  tests/test_pixel_families_cpu.py checks the planes hold
what is claimed here."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pixel_families as PF  # noqa: E402

EDGE_QUALITIES = (1, 10, 50, 90, 100)


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


def gpu_px(T, px):
    return T.from_numpy(np.ascontiguousarray(px)).cuda()


def first_bad(got, want):
    """'' or the first mismatches as (block, coefficient index, got, want)."""
    bad = np.argwhere(got != want)
    return "" if bad.size == 0 else "%d mismatches, first (block, coefficient, got, want) %s" % (
        len(bad), [(int(b), int(c), int(got[b, c]), int(want[b, c])) for b, c in bad[:6]])


def sym32(sym):
    import oracle as O
    a = sym.cpu().numpy()
    return O.unpack16(a.view(np.uint16)) if a.dtype == np.int16 else a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(key, q, ad):
    """(plane u8 [H, W], oracle coefficients, var_num int32) of a named plane, computed once."""
    import oracle as O
    name, tr = key
    if name == "sweep":
        blocks = PF.sweep_blocks(q, ad)[0]
    elif name == "batched":
        blocks = PF.batched_blocks(q, ad)[0]
    elif name == "edges":
        blocks = PF.pad(np.concatenate([PF.variance_edges()[0], PF.range_edge()]))
    else:
        blocks = PF.near_flat()[0]
    px = PF.plane(PF.transposed(blocks) if tr else blocks)
    want = O.forward_plane(px, q, ad)
    vn = (O.plane_variance(px) * 4096.0).astype(np.int32)
    for a in (px, want, vn):
        a.setflags(write=False)
    return px, want, vn


# ---- forward sweep: every quality, both modes ---------------------------------------------------
@pytest.mark.parametrize("q0", range(1, 101, 10))
def test_forward_sweep_every_plan(T, dm, q0):
    """forward_quant on the rational + textured plane of each plan, plain and transposed."""
    for q in range(q0, q0 + 10):
        for ad in (0, 1):
            plan = dm.Plan(q, ad)
            for tr in (False, True):
                px, want, _ = reference(("sweep", tr), q, ad)
                got = plan.forward_quant(gpu_px(T, px)).cpu().numpy()
                assert np.array_equal(got, want), (q, ad, "transposed" if tr else "plain", first_bad(got, want))


# ---- every exact implementation -----------------------------------------------------------------
def check_everything(T, dm, q, ad, px, want, vn, entries=None):
    """Every entry point that resolves ties, on one plane."""
    import oracle as O
    g = gpu_px(T, px)
    nb = want.shape[0]
    tag = (q, ad)
    plan = dm.Plan(q, ad)
    got = plan.forward_quant(g).cpu().numpy()  # no extras: the wide rounds (2 lanes per entry for 9..32)
    assert np.array_equal(got, want), (tag, "forward_quant", first_bad(got, want))
    v = T.zeros(nb, dtype=T.int32, device="cuda")
    got = plan.forward_quant(g, var_num=v).cpu().numpy()
    assert np.array_equal(got, want), (tag, "forward_quant + var_num", first_bad(got, want))
    assert np.array_equal(v.cpu().numpy(), vn), (tag, "var_num")
    counts = {}
    for variant in (None, 4):  # with the counter: one entry per lane above 8 entries
        p = dm.Plan(q, ad, variant=variant)
        cnt = T.zeros(1, dtype=T.int64, device="cuda")
        p.set_fallback_counter(cnt)
        got = p.forward_quant(g).cpu().numpy()
        p.set_fallback_counter(None)
        assert np.array_equal(got, want), (tag, "counter, variant %s" % variant, first_bad(got, want))
        counts[variant] = int(cnt.item())
    if entries is not None:
        assert counts[None] >= entries, (tag, counts, entries)
    assert counts[None] == counts[4], (tag, counts)
    for variant in (3, 1):
        got = dm.Plan(q, ad, variant=variant).forward_quant(g).cpu().numpy()
        assert np.array_equal(got, want), (tag, "variant %d" % variant, first_bad(got, want))
    side = [gpu_px(T, O.synth_plane(7, O.KINDS[k], 8 * 21, 8 * 5)) for k in ("uniform", "smooth")]
    got = plan.forward_quant_planes([side[0], g, side[1]])[1].cpu().numpy()
    assert np.array_equal(got, want), (tag, "forward_quant_planes[1]", first_bad(got, want))
    got = plan.round_trip_planes([g])[0][0].cpu().numpy()
    assert np.array_equal(got, want), (tag, "round_trip_planes", first_bad(got, want))
    woff, wsym = O.rle_encode_plane(want)
    for sb in sorted({4, plan.symbol_bytes}):
        ec, off, sym = plan.encode_planes([g], symbol_bytes=sb)
        got = ec[0].cpu().numpy()
        assert np.array_equal(got, want), (tag, "encode_planes %d" % sb, first_bad(got, want))
        assert np.array_equal(off.cpu().numpy().view(np.uint32), woff), (tag, "offsets", sb)
        assert np.array_equal(sym32(sym), wsym), (tag, "symbols", sb)
    bits = plan.huffman_bits_planes([g]).cpu().numpy().view(np.uint32)
    assert np.array_equal(bits, O.huffman_bits_plane(want)), (tag, "huffman_bits_planes")
    check_distortion(T, plan, g, px, want, vn, ad, tag)


def check_distortion(T, plan, g, px, want, vn, ad, tag):
    """distortion_planes against the u8 error of decode_planes of the ORACLE's coefficients."""
    gv = T.from_numpy(np.array(vn)).cuda()
    pix = plan.decode_planes([T.from_numpy(np.array(want)).cuda()], shapes=[px.shape],
                             var_nums=[gv] if ad else None)[0].cpu().numpy()[0]
    err = (px.astype(np.int64) - pix.astype(np.int64)) ** 2
    sse = err.reshape(px.shape[0] // 8, 8, px.shape[1] // 8, 8).sum((1, 3)).reshape(-1)
    got = plan.distortion_planes([g]).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, sse), (tag, "distortion_planes", int((got != sse).sum()))


@pytest.mark.parametrize("tr", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("q,ad", PF.EXACT_PLANS)
def test_every_exact_implementation(T, dm, q, ad, tr):
    """One batch per block row with 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 128 (256 at q84)
    tie entries: <= 8 entries run exact_grouped<8>; 9..16 exact_grouped<4> and 17..32
    exact_grouped<2> in the kernels with wide rounds (the forward without extras: <2> for 9..32);
    33..64 one entry per lane; above 64 several passes, lanes holding up to four flags in both
    words.  exact_grouped<4> is instantiated in the fused Huffman sizes alone, so it is observed
    only through per-block sizes: tests/test_pixel_families_cpu.py shows that in these 9..16-entry
    batches a tie moved to its other side changes the block's size.  Compared against the oracle of the plane as laid out (the transposed plane against
    the oracle of the transposed plane)."""
    px, want, vn = reference(("batched", tr), q, ad)
    blocks, _, counts = PF.batched_blocks(q, ad)
    entries = sum(counts)
    if tr:  # (0,4) and (4,0) change places and their divisors differ: the transposed plane's own true ties
        blocks = PF.transposed(blocks)
        flat = (blocks.reshape(-1, 64) == blocks.reshape(-1, 64)[:, :1]).all(1)
        entries = int((PF.tie_mask(blocks, q, ad)[0] & ~flat[:, None]).sum())
        assert entries > 64
    check_everything(T, dm, q, ad, px, want, vn, entries)


def test_regression_q6_adaptive_tie_between_the_clamp_edges(T, dm):
    """q6 adaptive, (a, b, c) = (16, 8, 20): var = 720, M = 200 (2 - 0.72) = 256 and 8 a / M is
    exactly 0.5 at (0,4); the reference returns 0 for every d."""
    import oracle as O
    s = PF.S
    blocks = np.stack([(128 + d + 16 * s[None, :] + 8 * s[:, None] + 20 * np.outer(s, s)).astype(np.uint8)
                       for d in range(-64, 64)])
    px = PF.plane(blocks)
    want = O.forward_plane(px, 6, 1)
    assert (want[:, PF.H] == 0).all()
    for tr in (False, True):
        p = PF.plane(PF.transposed(blocks)) if tr else px
        w = O.forward_plane(p, 6, 1)
        got = dm.Plan(6, 1).forward_quant(gpu_px(T, p)).cpu().numpy()
        assert np.array_equal(got, w), (tr, first_bad(got, w))


# ---- edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "near_flat"])
@pytest.mark.parametrize("q", EDGE_QUALITIES)
def test_edge_families(T, dm, q, name):
    """variance_edges + range_edge, and near_flat: forward_quant with var_num and the encoder in
    every symbol width the plan admits, both modes."""
    import oracle as O
    for ad in (0, 1):
        px, want, vn = reference((name, False), q, ad)
        g = gpu_px(T, px)
        plan = dm.Plan(q, ad)
        v = T.zeros(want.shape[0], dtype=T.int32, device="cuda")
        cnt = T.zeros(1, dtype=T.int64, device="cuda")
        plan.set_fallback_counter(cnt)
        got = plan.forward_quant(g, var_num=v).cpu().numpy()
        plan.set_fallback_counter(None)
        assert np.array_equal(got, want), (q, ad, name, first_bad(got, want))
        assert np.array_equal(v.cpu().numpy(), vn), (q, ad, name)
        print(f"{name} q{q} a{ad}: exact-path entries {int(cnt.item())}, max |coef| {int(np.abs(got).max())}, "
              f"symbol_bytes {plan.symbol_bytes}")
        if plan.symbol_bytes == 2:
            assert np.abs(got.astype(int)).max() <= 511, (q, ad, name)
        if name == "near_flat" and q == 50:
            # These DCs must not take the constant-block table.  They cannot be seen in the fallback
            # counter: 8 (v - 128) +- 1/8 over Q = 16 lies 1/128 from the odd levels' tie, far outside
            # the fast path's guard band (~1e-5), so no correct kernel sends them to the exact path
            # (measured: 0 entries).  What shows the table was not taken is the DC itself: for every
            # odd level one of the two directions rounds to the other side than the constant block.
            blocks, const = PF.near_flat()
            table = O.forward_plane(PF.plane(np.broadcast_to(blocks[:, :1, :1], blocks.shape).copy()), q, ad)[:, 0]
            moved = ~const & (want[:, 0] != table)
            assert moved.sum() >= 256 and np.array_equal(got[moved, 0], want[moved, 0]), (q, ad)
        woff, wsym = O.rle_encode_plane(want)
        for sb in sorted({4, plan.symbol_bytes}):
            ec, off, sym = plan.encode_planes([g], symbol_bytes=sb)
            assert np.array_equal(ec[0].cpu().numpy(), want), (q, ad, name, sb)
            assert np.array_equal(off.cpu().numpy().view(np.uint32), woff), (q, ad, name, sb)
            assert np.array_equal(sym32(sym), wsym), (q, ad, name, sb)


# ---- grid-stride ---------------------------------------------------------------------------------
@pytest.mark.parametrize("q,ad", [(84, 0), (6, 1)])
def test_tie_dense_plane_one_workgroup(T, dm, q, ad):
    """The batched plane under a grid of one workgroup: each wave meets several tie-heavy batches
    in a row (its flags, scratch entries and stage are reused batch after batch)."""
    import oracle as O
    px, want, vn = reference(("batched", False), q, ad)
    g = gpu_px(T, px)
    with dm.grid_limit(1):
        plan = dm.Plan(q, ad)
        got = plan.forward_quant(g).cpu().numpy()
        assert dm.last_grid() == 1
        assert np.array_equal(got, want), (q, ad, "forward_quant", first_bad(got, want))
        got = plan.round_trip_planes([g])[0][0].cpu().numpy()
        assert np.array_equal(got, want), (q, ad, "round_trip_planes", first_bad(got, want))
        ec, off, sym = plan.encode_planes([g])
        assert np.array_equal(ec[0].cpu().numpy(), want), (q, ad, "encode_planes")
        assert np.array_equal(sym32(sym), O.rle_encode_plane(want)[1]), (q, ad, "symbols")
        bits = plan.huffman_bits_planes([g]).cpu().numpy().view(np.uint32)
        assert np.array_equal(bits, O.huffman_bits_plane(want)), (q, ad, "huffman_bits_planes")
        check_distortion(T, plan, g, px, want, vn, ad, (q, ad, "one workgroup"))
