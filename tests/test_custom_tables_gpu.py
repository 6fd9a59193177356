"""GPU: plans built from a caller's quantization table (dctq_plan_from_context through
Plan.from_table).  Every exactness claim of the project -- bit-exact int16 coefficients, the guard
band of the fp32 fast path, the 2-byte symbol format, the admission of the fp32 inverse, the
decoders' 0.5 + e pixel bound -- had only been exercised on the 100 tables quant_matrix(8, quality)
can produce: integer-valued, small, monotone in frequency.  The tables here (tables()) leave that
family: non-integer entries, divisors in the tens of thousands next to 1, and a DC divisor that
puts the largest quantized value exactly on the 2-byte format's edge of 511.  The checker is the
oracle's table-taking plane drivers (tests/test_oracle.py pins them to the compiled reference).

Pictures (pictures()): two planes in one call, 40 x 104 (65 blocks: a full 64-block batch, a
one-block tail, two full and a one-block 32-block batch) and 8 x 8 (a plane switch) -- the geometry
of test_gpu_parity.py::test_every_dispatch_leaf -- of six kinds.

In-range shares (reference pixels strictly inside (0, 255), where a rounding check means
something), measured on the CPU, in per cent, for noise / quarter / zeros / full / const / smooth
(test_inverse_and_decoders prints them and asserts the best kind of every plan above 5 %):
    scaled   a0  100   100   100   100   100   100       a1   95.1 100     0     0    98.5 100
    flat137  a0  100   100   100   100   100   100       a1   99.6 100   100     0   100   100
    ramp     a0  100   100   100   100   100   100       a1   98.2 100   100   100   100   100
    checker  a0  100   100   100   100   100   100       a1  100   100   100   100   100   100
    edge511  a0  100   100   100   100   100   100       a1  100   100   100   100   100   100
    edge512  a0  100   100   100   100   100   100       a1  100   100   100   100   100   100
Non-adaptive plans dequantize with 1 / Q (src/quantization.c:139,144), so their recon stays next
to 128 wherever Q is large and is the picture itself where Q is 1.  Adaptive plans multiply by
Q (2 - nv), but a divisor of tens of thousands quantizes its coefficient to 0 first, so what comes
back is the picture without those frequencies: max |reference| over all of this file is 333,
and every kind but the two saturated pictures of some plans carries the rounding check.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_decode_foreign_gpu import blocks_of, check_pixels

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
STD_QUALITIES = [1, 50, 72, 100]
CUSTOM = ["scaled", "flat137", "ramp", "checker", "edge511", "edge512"]
KINDS = ["noise", "quarter", "zeros", "full", "const", "smooth"]
SHAPES = [(40, 104), (8, 8)]


@functools.lru_cache(maxsize=None)
def tables():
    """name -> 8 x 8 float64, read-only.  std<q>: the anchor, quant_matrix(8, q)."""
    import oracle as O
    i, j = np.indices((8, 8))
    t = {f"std{q}": O.quant_matrix(8, q) for q in STD_QUALITIES}
    t["scaled"] = np.maximum(1.0, 0.7391 * O.quant_matrix(8, 50))           # non-integer entries
    t["flat137"] = np.full((8, 8), 1.37)                                    # near 1, every divisor != 1
    t["ramp"] = np.minimum(65535.0, 65535.0 ** ((i + j) / 14.0))            # geometric along i + j: 1 .. 65535
    t["checker"] = np.where((i + j) % 2 == 0, 1.0, 65535.0)                 # extreme neighbours
    t["edge511"] = np.full((8, 8), 1024.0)
    t["edge511"][0, 0] = 2.002                                              # round(1024 / 2.002) = 511
    t["edge512"] = np.full((8, 8), 1024.0)
    t["edge512"][0, 0] = 2.0                                                # 1024 / 2 = 512
    assert t["ramp"][0, 0] == 1.0 and t["ramp"][7, 7] == 65535.0
    for a in t.values():
        assert a.dtype == np.float64 and a.shape == (8, 8) and (a >= 1.0).all() and (a <= 65535.0).all()
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def pictures():
    """kind -> [u8 40 x 104, u8 8 x 8], read-only, seeded."""
    import oracle as O
    rng = np.random.default_rng(2718)
    p = {
        "noise": [rng.integers(0, 256, size=s, dtype=np.uint8) for s in SHAPES],
        # a quarter of the range: block variances of 150-400, an adaptive plan scales every block differently
        "quarter": [rng.integers(96, 160, size=s, dtype=np.uint8) for s in SHAPES],
        "zeros": [np.zeros(s, np.uint8) for s in SHAPES],
        "full": [np.full(s, 255, np.uint8) for s in SHAPES],
        "const": [np.kron(rng.integers(0, 256, size=(h // 8, w // 8), dtype=np.uint8), np.ones((8, 8), np.uint8))
                  for h, w in SHAPES],
        "smooth": [O.synth_plane(31 + k, O.KINDS["smooth"], w, h) for k, (h, w) in enumerate(SHAPES)],
    }
    assert list(p) == KINDS
    for planes in p.values():
        for a, s in zip(planes, SHAPES):
            assert a.dtype == np.uint8 and a.shape == s
            a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def forward_ref(tname, ad, kind):
    """The oracle's forward of one picture under one table: (coef [int16 [nblk_k, 64]] per plane, var per plane)."""
    import oracle as O
    hosts = pictures()[kind]
    coef = [O.forward_plane(p, 0, ad, table=tables()[tname]) for p in hosts]
    var = [O.plane_variance(p) for p in hosts]
    for a in coef + var:
        a.setflags(write=False)
    return coef, var


@functools.lru_cache(maxsize=None)
def inverse_ref(tname, ad, kind):
    """(want [n, 64] = the oracle's inverse_plane + 128 of forward_ref's coefficients, blocks of both planes
    concatenated; var_num int32 [n]; tol64 [n, 64], the bound include/dct_amd.h states for dctq_inverse:
    2^-24 max(|reference|, 128) + 1e-9 max(1, sum_k x_k / 1024), the multipliers from the table)."""
    import oracle as O
    import inv_bound as IB  # tools/, on the path through test_decode_foreign_gpu
    Q = tables()[tname].ravel()
    coef, var = forward_ref(tname, ad, kind)
    coef, var = np.concatenate(coef), np.concatenate(var)
    vn = np.round(var * 4096.0).astype(np.int32)
    assert np.array_equal(vn / 4096.0, var)  # calculate_block_variance == var_num / 4096 exactly
    if ad:
        want = O.inverse_plane(coef, 0, 1, var, table=Q) + 128.0
        nv = np.minimum(1.0, np.maximum(0.1, var / 1000.0))
        mult = Q[None, :] * (2.0 - nv)[:, None]
        mult[:, 0] = Q[0]
    else:
        want = O.inverse_plane(coef, 0, 0, table=Q) + 128.0
        mult = (1.0 / Q)[None, :]
    sx = IB.block_magnitudes(coef, mult).sum(axis=1, keepdims=True)
    tol64 = U * np.maximum(np.abs(want), 128.0) + 1e-9 * np.maximum(1.0, sx / 1024.0)
    for a in (want, vn, tol64):
        a.setflags(write=False)
    return want, vn, tol64


def in_range_share(tname, ad, kind):
    want = inverse_ref(tname, ad, kind)[0]
    return float(((want > 0.0) & (want < 255.0)).mean())


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


def host(t):
    return t.cpu().numpy()


def sym32(sym):
    """An encoder symbol tensor (int32: 4-byte format, int16: 2-byte format) as 4-byte symbols."""
    import oracle as O
    a = host(sym)
    return O.unpack16(a.view(np.uint16)) if a.dtype == np.int16 else a.view(np.uint32)


def fresh_var_nums(T):
    return [T.full((h * w // 64,), -1, dtype=T.int32, device="cuda") for h, w in SHAPES]


def everything(T, plan, planes):
    """Every pixel-fed entry point of a plan on one picture, as a flat list of (name, tensor)."""
    out = []
    vns = fresh_var_nums(T)
    out += [(f"forward coef {k}", c) for k, c in enumerate(plan.forward_quant_planes(planes, var_nums=vns))]
    out += [(f"forward var_num {k}", v) for k, v in enumerate(vns)]
    vns = fresh_var_nums(T)
    coefs, recs = plan.round_trip_planes(planes, var_nums=vns)
    out += [(f"round trip coef {k}", c) for k, c in enumerate(coefs)]
    out += [(f"round trip recon {k}", r) for k, r in enumerate(recs)]
    out += [(f"round trip var_num {k}", v) for k, v in enumerate(vns)]
    for sb in [4] + ([2] if plan.symbol_bytes == 2 else []):
        ec, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
        out += [(f"encode{sb} coef {k}", c) for k, c in enumerate(ec)] + [(f"encode{sb} offsets", off),
                                                                          (f"encode{sb} symbols", sym)]
    pix = plan.decode_planes(coefs, shapes=SHAPES, var_nums=vns if plan.adaptive else None)
    out += [(f"decode {k}", p) for k, p in enumerate(pix)]
    out += [("huffman bits", plan.huffman_bits_planes(planes)), ("distortion", plan.distortion_planes(planes))]
    return out


# ---- 1. the anchor: a standard table through from_table is the standard plan ---------------------
@pytest.mark.parametrize("q", STD_QUALITIES)
def test_anchor_standard_tables(T, dm, q):
    for ad in (0, 1):
        a, b = dm.Plan.from_table(tables()[f"std{q}"], ad, quality=q), dm.Plan(q, ad)
        assert a.symbol_bytes == b.symbol_bytes == (4 if q == 100 else 2), (q, ad)
        assert np.array_equal(a.table, tables()[f"std{q}"]) and (a.quality, a.adaptive) == (q, bool(ad))
        for kind in KINDS:
            planes = [gpu(T, p) for p in pictures()[kind]]
            ra, rb = everything(T, a, planes), everything(T, b, planes)
            assert [n for n, _ in ra] == [n for n, _ in rb]
            for (name, x), (_, y) in zip(ra, rb):
                assert T.equal(x, y), (q, ad, kind, name)


# ---- 2. the forward, bit exact -------------------------------------------------------------------
@pytest.mark.parametrize("ad", [0, 1])
@pytest.mark.parametrize("tname", CUSTOM)
def test_forward_bit_exact(T, dm, tname, ad):
    """Coefficients of forward_quant_planes, round_trip_planes and encode_planes equal the oracle's
    table-taking forward_plane; var_num / 4096 equals plane_variance; the fallback counter is 0
    when detached, equal between the fused and the unfused forward, and at least the number of
    blocks whose DC lies within 1e-9 of a half integer (inside every guard band, which is >= 2^-25
    wide for every table: fill_fast_tables); offsets, symbols and Huffman sizes are the oracle's."""
    import oracle as O
    Q = tables()[tname]
    plan = dm.Plan.from_table(Q, ad)
    ties_seen = 0
    for kind in KINDS:
        hosts = pictures()[kind]
        planes = [gpu(T, p) for p in hosts]
        want_c, var = forward_ref(tname, ad, kind)
        sums = np.concatenate([p.astype(np.int64).reshape(h // 8, 8, w // 8, 8).sum(axis=(1, 3)).ravel() - 64 * 128
                               for p, (h, w) in zip(hosts, SHAPES)])
        dc = np.abs(sums / 8.0 / Q[0, 0])
        dc_ties = int((np.abs(dc - np.floor(dc) - 0.5) < 1e-9).sum())
        ties_seen += dc_ties
        counts = {}
        for with_cnt in (True, False):
            cnt = T.zeros(1, dtype=T.int64, device="cuda")
            plan.set_fallback_counter(cnt if with_cnt else None)
            for fused in (False, True):
                vns = fresh_var_nums(T)
                if fused:
                    coefs, _ = plan.round_trip_planes(planes, var_nums=vns)
                else:
                    coefs = plan.forward_quant_planes(planes, var_nums=vns)
                for k in range(2):
                    got = host(coefs[k])
                    assert np.array_equal(got, want_c[k]), (tname, ad, kind, fused, k, int((got != want_c[k]).sum()),
                                                            np.argwhere(got != want_c[k])[:4].tolist())
                    assert np.array_equal(host(vns[k]).astype(np.float64) / 4096.0, var[k]), (tname, ad, kind, fused, k)
                n = int(cnt.item())
                cnt.zero_()
                if with_cnt:
                    counts[fused] = n
                else:
                    assert n == 0, (tname, ad, kind, fused)
            plan.set_fallback_counter(None)
        print(f"{tname} a{ad} {kind}: fallbacks {counts[False]} of {64 * 66} coefficients, DC ties {dc_ties}")
        assert counts[False] == counts[True] >= dc_ties, (tname, ad, kind, counts, dc_ties)
        allc = np.concatenate(want_c)
        woff, wsym = O.rle_encode_plane(allc)
        for sb in [4] + ([2] if plan.symbol_bytes == 2 else []):
            ec, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
            for k in range(2):
                assert np.array_equal(host(ec[k]), want_c[k]), (tname, ad, kind, "encode", sb, k)
            assert np.array_equal(host(off).view(np.uint32), woff), (tname, ad, kind, "offsets", sb)
            assert sym.dtype == (T.int16 if sb == 2 else T.int32)
            assert np.array_equal(sym32(sym), wsym), (tname, ad, kind, "symbols", sb)
        bits = host(plan.huffman_bits_planes(planes)).view(np.uint32)
        assert np.array_equal(bits, O.huffman_bits_plane(allc)), (tname, ad, kind, "huffman")
    if Q[0, 0] == 1.0:  # sum(px - 128) / 8 is a half integer for one block in eight: the lower bound is not idle
        assert ties_seen >= 4, (tname, ties_seen)


# ---- 3. the 511 edge of the 2-byte symbol format ---------------------------------------------------
def test_edge_511(T, dm):
    import oracle as O
    planes = [gpu(T, p) for p in pictures()["zeros"]]
    for ad in (0, 1):
        want = np.concatenate(forward_ref("edge511", ad, "zeros")[0])
        assert (want[:, 0] == -511).all() and not want[:, 1:].any()  # on the oracle first: not a vacuous pass
        plan = dm.Plan.from_table(tables()["edge511"], ad)
        assert plan.symbol_bytes == 2
        vns = [gpu(T, np.zeros(h * w // 64, np.int32)) for h, w in SHAPES]  # all-0 picture: variance 0
        c2, off2, sym2 = plan.encode_planes(planes, symbol_bytes=2)
        c4, off4, sym4 = plan.encode_planes(planes, symbol_bytes=4)
        assert sym2.dtype == T.int16 and sym4.dtype == T.int32
        for c in (c2, c4):
            assert np.array_equal(np.concatenate([host(x) for x in c]), want), ad
        woff, wsym = O.rle_encode_plane(want)
        assert np.array_equal(host(off2).view(np.uint32), woff) and np.array_equal(host(off4).view(np.uint32), woff)
        assert np.array_equal(host(sym4).view(np.uint32), wsym)
        assert np.array_equal(host(sym2).view(np.uint16), O.pack16(host(sym4).view(np.uint32)))
        assert np.array_equal(host(dm.rle_decode(sym2, off2)), want)
        direct = plan.decode_planes(c2, shapes=SHAPES, var_nums=vns if ad else None)
        for sym, off in ((sym2, off2), (sym4, off4)):
            got = plan.decode_symbols(sym, off, shapes=SHAPES, var_nums=vns if ad else None)
            assert all(T.equal(g, d) for g, d in zip(got, direct)), (ad, sym.dtype)

        want = np.concatenate(forward_ref("edge512", ad, "zeros")[0])
        assert (want[:, 0] == -512).all() and not want[:, 1:].any()
        plan = dm.Plan.from_table(tables()["edge512"], ad)
        assert plan.symbol_bytes == 4
        with pytest.raises(dm.DctqError, match="dctq error -1:"):
            plan.encode_planes(planes, symbol_bytes=2)
        c4, off4, sym4 = plan.encode_planes(planes)
        assert sym4.dtype == T.int32
        assert np.array_equal(np.concatenate([host(x) for x in c4]), want), ad
        woff, wsym = O.rle_encode_plane(want)
        assert np.array_equal(host(off4).view(np.uint32), woff) and np.array_equal(host(sym4).view(np.uint32), wsym)
        assert np.array_equal(host(dm.rle_decode(sym4, off4)), want)
        direct = plan.decode_planes(c4, shapes=SHAPES, var_nums=vns if ad else None)
        got = plan.decode_symbols(sym4, off4, shapes=SHAPES, var_nums=vns if ad else None)
        assert all(T.equal(g, d) for g, d in zip(got, direct)), ad


# ---- 4. the inverse and the decoders ---------------------------------------------------------------
@pytest.mark.parametrize("ad", [0, 1])
@pytest.mark.parametrize("tname", CUSTOM)
def test_inverse_and_decoders(T, dm, tname, ad):
    """Coefficients: the oracle's forward of the pictures, so inside the plan's forward range.
    dctq_inverse and the round trip's recon against the oracle's table-taking inverse_plane + 128:
    1e-4 for non-adaptive plans (|recon| < 2048, asserted on the reference), the fp64 bound of
    include/dct_amd.h for adaptive ones, whose recon leaves 2048 on large divisors.  The three
    decoders agree bit for bit and lie within 0.5 + e of the clamped reference, clamped exactly
    beyond e: e = max(fp64 bound, 1e-4) non-adaptive (whichever inverse the plan admits), the fp64
    bound adaptive.  distortion_planes is the squared error of that picture."""
    import oracle as O
    plan = dm.Plan.from_table(tables()[tname], ad)
    shares = {}
    for kind in KINDS:
        hosts = pictures()[kind]
        planes = [gpu(T, p) for p in hosts]
        coef_h, _ = forward_ref(tname, ad, kind)
        want, vn, tol64 = inverse_ref(tname, ad, kind)
        if ad:
            tol_rec = e = tol64
        else:
            assert np.abs(want).max() < 2048.0, (tname, kind)
            tol_rec, e = np.full_like(tol64, 1e-4), np.maximum(tol64, 1e-4)
        coefs = [gpu(T, c) for c in coef_h]
        allc = T.cat(coefs)
        gvn = gpu(T, vn)
        vns = list(T.split(gvn, [c.shape[0] for c in coefs]))
        rec = host(plan.inverse(allc, var_num=gvn if ad else None)).astype(np.float64)
        err = np.abs(rec - want)
        print(f"{tname} a{ad} {kind}: max |recon| {np.abs(want).max():.4g}, dctq_inverse max err / bound "
              f"{(err / tol_rec).max():.3f}")
        assert (err <= tol_rec).all(), (tname, ad, kind, "inverse", float((err / tol_rec).max()))
        rc, rr = plan.round_trip_planes(planes)
        assert all(T.equal(a, b) for a, b in zip(rc, coefs)), (tname, ad, kind)
        err = np.abs(np.concatenate([host(r) for r in rr]).astype(np.float64) - want)
        print(f"{tname} a{ad} {kind}: round trip recon max err / bound {(err / tol_rec).max():.3f}")
        assert (err <= tol_rec).all(), (tname, ad, kind, "round trip", float((err / tol_rec).max()))

        pix = plan.decode_planes(coefs, shapes=SHAPES, var_nums=vns if ad else None)
        woff, wsym = O.rle_encode_plane(np.concatenate(coef_h))
        goff, gsym = gpu(T, woff.view(np.int32)), gpu(T, wsym.view(np.int32))
        from_sym = plan.decode_symbols(gsym, goff, shapes=SHAPES, var_nums=vns if ad else None)
        packed, boff = dm.bits_pack(gsym, goff)
        from_bits = plan.decode_bits(packed, boff, shapes=SHAPES, var_nums=vns if ad else None)
        for k in range(2):
            assert T.equal(from_sym[k], pix[k]), (tname, ad, kind, "decode_symbols", k)
            assert T.equal(from_bits[k], pix[k]), (tname, ad, kind, "decode_bits", k)
        pb = np.concatenate([blocks_of(host(p)[0]) for p in pix])
        shares[kind] = check_pixels(pb, want, e, f"{tname} a{ad} {kind}")
        src = np.concatenate([blocks_of(p) for p in hosts]).astype(np.int64)
        sse = host(plan.distortion_planes(planes))
        assert np.array_equal(sse, ((src - pb.astype(np.int64)) ** 2).sum(axis=1)), (tname, ad, kind, "distortion")
    # a rounding check needs pixels that land inside the range (the shares in the module docstring)
    assert max(shares.values()) > 0.05, (tname, ad, shares)


# ---- 5. ownership and validation -------------------------------------------------------------------
def coefficients(T, plan):
    return T.cat(plan.forward_quant_planes([gpu(T, p) for p in pictures()["quarter"]]))


def test_plan_copies_the_table(T, dm):
    """The plan copies the VALUES of quant_matrix: the caller's array may change afterwards, and
    dequant_matrix -- NULL or garbage -- is not read."""
    for tname in ("scaled", "ramp"):
        for ad in (0, 1):
            want = np.concatenate(forward_ref(tname, ad, "quarter")[0])
            mine = np.array(tables()[tname])
            plan = dm.Plan.from_table(mine, ad)          # dequant_matrix NULL
            mine[:] = 7.0
            assert np.array_equal(plan.table, tables()[tname])
            assert np.array_equal(host(coefficients(T, plan)), want), (tname, ad)
            mine = np.array(tables()[tname])
            garbage = np.full((8, 8), np.nan)
            garbage[::2] = -1e300
            ctx = dm.quant_context(mine, ad, 50, dequant=garbage)
            plan2 = dm.Plan.from_context(ctx)
            mine[:] = 65535.0
            garbage[:] = 0.0
            del ctx
            assert np.array_equal(plan2.table, tables()[tname])
            assert np.array_equal(host(coefficients(T, plan2)), want), (tname, ad)
            vn = inverse_ref(tname, ad, "quarter")[1]
            a = plan.inverse(gpu(T, want), var_num=gpu(T, vn) if ad else None)
            b = plan2.inverse(gpu(T, want), var_num=gpu(T, vn) if ad else None)
            assert T.equal(a, b), (tname, ad)


BAD_ENTRIES = [0.999, 65535.5, float("nan"), float("inf"), -4.0]


def test_validation(T, dm):
    """What build_plan and dctq_plan_from_context refuse is refused with the invalid-argument error,
    and a valid call still works afterwards."""
    std50 = tables()["std50"]
    want = host(coefficients(T, dm.Plan(50, 0)))

    def still_works():
        assert np.array_equal(host(coefficients(T, dm.Plan.from_table(std50))), want)

    for bad in BAD_ENTRIES:
        for where in [(0, 0), (3, 5), (7, 7)]:
            t = np.array(std50)
            t[where] = bad
            with pytest.raises(dm.DctqError, match="dctq error -1:"):
                dm.Plan.from_table(t)
        still_works()
    with pytest.raises(dm.DctqError, match="dctq error -1:"):
        dm.Plan.from_context(dm.quant_context(np.array(std50), block_size=16))
    still_works()
    ctx = dm.quant_context(np.array(std50))
    ctx.quant_matrix = None
    with pytest.raises(dm.DctqError, match="dctq error -1:"):
        dm.Plan.from_context(ctx)
    still_works()
    with pytest.raises(dm.DctqError, match="dctq error -1:"):
        dm.Plan.from_context(None)
    still_works()
    L = dm.lib()
    ctx = dm.quant_context(np.array(std50))
    assert L.dctq_plan_from_context(C.byref(ctx), None) == -1  # a NULL plan pointer
    assert b"NULL" in L.dctq_error_string(-1)
    still_works()
