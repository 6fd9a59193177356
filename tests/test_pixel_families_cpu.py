"""CPU: the generators of tools/pixel_families.py against the oracle, so that
tests/test_pixel_ties_gpu.py cannot pass vacuously.  Conditions, not measurements: the counts
are printed and asserted."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inv_bound as IB  # noqa: E402
import pixel_families as PF  # noqa: E402

NAMES = {PF.DC: "(0,0)", PF.H: "(0,4)", PF.V: "(4,0)", PF.HV: "(4,4)"}
P = list(PF.POSITIONS)


@pytest.fixture(scope="module")
def sweep():
    """Per plan of the GPU forward sweep (every quality, both modes): ties and ties against
    round-half-away at the four positions, and the adaptive non-DC ties with 100 < var < 1000."""
    out = {}
    for q in range(1, 101):
        for ad in (0, 1):
            blocks, ties = PF.sweep_blocks(q, ad)
            m, against = PF.tie_mask(blocks, q, ad)
            assert sorted(ties) == sorted((int(b), P[k]) for b, k in zip(*np.nonzero(m[:, P])))
            var = PF.var_num(blocks) / 4096.0
            mid = int((m[:, P[1:]] & ((var > 100) & (var < 1000))[:, None]).sum()) if ad else 0
            out[(q, ad)] = (m[:, P].sum(0), against[:, P].sum(0), mid, np.bincount(m[:, P].sum(1), minlength=5))
    return out


def test_every_admitted_position_has_ties(sweep):
    """Each of (0,4), (4,0), (4,4) that the plan's divisors admit a tie at has >= 32 built ties."""
    for (q, ad), (cnt, against, mid, per) in sweep.items():
        admitted = PF.tie_positions(q, ad)
        print(f"q{q} a{ad}: ties at (0,0) (0,4) (4,0) (4,4) = {cnt.tolist()}, against half-away {against.tolist()}, "
              f"blocks with 0..4 ties {per.tolist()}")
        for k, p in enumerate(P):
            if p in admitted and p != PF.DC:
                assert cnt[k] >= 32, (q, ad, NAMES[p], int(cnt[k]))


def test_ties_depend_on_the_reference_order(sweep):
    """>= 20 % of all built ties are resolved by the oracle against round-half-away-from-zero
    (the unsteered family measured 70 %); >= 64 adaptive non-DC ties have 100 < var < 1000; ties
    in the first flag word only, the second only and both, and 1 to 4 per block, all occur."""
    tot = sum(int(c.sum()) for c, _, _, _ in sweep.values())
    ag = sum(int(a.sum()) for _, a, _, _ in sweep.values())
    mid = sum(m for _, _, m, _ in sweep.values())
    per = sum(p for _, _, _, p in sweep.values())
    print(f"{tot} ties, {ag} against half-away ({100.0 * ag / tot:.1f} %), {mid} adaptive non-DC ties with "
          f"100 < var < 1000, blocks with 0..4 ties {per.tolist()}")
    assert ag >= 0.2 * tot
    assert mid >= 64
    assert (per[1:] > 0).all()
    blocks, _ = PF.sweep_blocks(84, 0)
    m, _ = PF.tie_mask(blocks, 84, 0)
    lo, hi = m[:, [PF.DC, PF.V]].any(1), m[:, [PF.H, PF.HV]].any(1)  # slots 0, 8 | 32, 40
    assert (lo & ~hi).any() and (hi & ~lo).any() and (lo & hi).any()


def test_exact_plans_cover_their_positions_and_edges():
    """The plans every exact implementation runs on: q25 ties at (0,4), q52 at (4,0), q60 at (4,4),
    q84 at all four with four-tie blocks; adaptive ties strictly between the clamp edges, at var
    exactly 100 and at var exactly 1000; every batch holds exactly its chosen number of entries."""
    seen = {}
    for q, ad in PF.EXACT_PLANS:
        blocks, ties = PF.tie_blocks(q, ad)
        m, against = PF.tie_mask(blocks, q, ad)
        var = PF.var_num(blocks) / 4096.0
        seen[(q, ad)] = m[:, P].sum(0)
        edge = {v: (int(m[var == v][:, P].sum()), int(m[var == v][:, P[1:]].sum())) for v in (100, 1000)}
        mid = int((m[:, P[1:]] & ((var > 100) & (var < 1000))[:, None]).sum())
        print(f"q{q} a{ad}: ties {m[:, P].sum(0).tolist()} against half-away {against[:, P].sum(0).tolist()}; "
              f"at var 100 {edge[100]}, at var 1000 {edge[1000]} (all, non-DC); between {mid}")
        if (q, ad) == (6, 1):
            assert mid >= 64
        if (q, ad) == (50, 1):
            assert edge[100][0] > 0  # the DC: the only position that can tie at var = 100 (pixel_families.EXACT_PLANS)
        if (q, ad) == (60, 1):
            assert edge[1000][1] > 0
        out, entries, counts = PF.batched_blocks(q, ad)
        flat = (out.reshape(-1, 64) == out.reshape(-1, 64)[:, :1]).all(1)
        bm, _ = PF.tie_mask(out, q, ad)
        got = (bm & ~flat[:, None]).reshape(len(counts), -1).sum(1)
        assert got.tolist() == counts == [len(e) for e in entries], (q, ad)
        assert max(counts) >= 128 and set(PF.ENTRY_COUNTS[:-1]) <= set(counts)
    assert seen[(25, 0)][1] >= 32 and seen[(52, 0)][2] >= 32 and seen[(60, 0)][3] >= 32 and seen[(50, 0)][0] >= 32
    assert (seen[(84, 0)] >= 32).all() and 256 in PF.batched_blocks(84, 0)[2]


def test_variance_edges_hit_both_edges_and_their_nearest_neighbours():
    """var_num equals both edges exactly, and the neighbours are the nearest attainable: edge - 1 and
    edge + 7.  var_num = 64 s2 - s1^2 with s2 = s1 (mod 2) (x^2 = x mod 2), so whether edge + d is
    attainable at all depends on s1 mod 128 only: enumerated here, no d in 1..6 passes."""
    import oracle as O
    blocks, vn = PF.variance_edges()
    var = O.plane_variance(PF.plane(PF.pad(blocks)))[:len(blocks)]
    assert np.array_equal(var * 4096.0, vn.astype(np.float64))
    assert PF.VAR_STEPS == (-1, 7)
    for edge in PF.VAR_EDGES:
        for d in range(1, 7):
            assert not any((edge + d + s1 * s1) % 64 == 0 and ((edge + d + s1 * s1) // 64 - s1) % 2 == 0
                           for s1 in range(128)), (edge, d)
        below, above = vn[vn < edge].max(), vn[(vn > edge) & (vn < 2 * edge)].min()
        print(f"var_num {edge}: {int((vn == edge).sum())} blocks exactly, {int((vn == below).sum())} at {below - edge}, "
              f"{int((vn == above).sum())} at +{above - edge}")
        assert (vn == edge).sum() >= 8 and below == edge - 1 and above == edge + 7
        assert (vn == below).sum() >= 4 and (vn == above).sum() >= 4
    assert set(vn.tolist()) == {e + d for e in PF.VAR_EDGES for d in (-1, 0, 7)}
    assert (var == 100.0).any() and (var == 1000.0).any()


def test_divisors_are_the_oracles():
    """PF.divisors against oracle.adjust block by block, and the quantized value against
    round(coefficient / divisor): the tie census uses the divisor the oracle uses."""
    import oracle as O
    for q, ad in ((6, 1), (50, 1), (60, 1), (25, 0)):
        blocks = PF.tie_blocks(q, ad)[0][::7]
        div = PF.divisors(blocks, q, ad)
        var = O.plane_variance(PF.plane(PF.pad(blocks)))[:len(blocks)]
        Q = O.quant_matrix(8, q)
        for b in range(0, len(blocks), 5):
            want = O.adjust(Q, float(var[b]), 1).ravel() if ad else Q.ravel()
            assert np.array_equal(div[b], want), (q, ad, b)
        got, quo = PF.quotients(blocks, q, ad)
        far = np.abs(quo - np.floor(quo) - 0.5) > 1e-6
        assert np.array_equal(got[far], np.floor(quo + 0.5)[far].astype(np.int16)), (q, ad)


def test_four_lane_rounds_show_in_the_huffman_sizes():
    """exact_grouped<4> (passes of 9..16 entries) exists only in the fused Huffman sizes, whose output
    is a size per block: a tie resolved to the wrong side shows only if the block's size changes.
    Moving one tie alone to its other side often keeps the size (the block's symbol frequencies stay
    the same), so batched_blocks fills the 9..16-entry batches from blocks with a tie whose flip does
    change it (size_sensitive).  Asserted: in every such batch of every plan at least a quarter of
    the entries change their block's size when flipped -- every block there holds such an entry and
    no block has more than four entries."""
    import oracle as O
    for q, ad in PF.EXACT_PLANS:
        out, entries, counts = PF.batched_blocks(q, ad)
        got, quo = PF.quotients(out, q, ad)
        half = np.floor(quo) + 0.5
        other = (2 * half - got).astype(np.int16)  # floor <-> ceil of the half-integer
        bits = O.huffman_bits_plane(got)
        seen = []
        for r, n in enumerate(counts):
            if not 9 <= n <= 16:
                continue
            changed = 0
            for lane, c in entries[r]:
                b = 64 * r + lane
                alt = got[b].copy()
                alt[c] = other[b, c]
                changed += int(O.huffman_bits(alt.reshape(8, 8)) != int(bits[b]))
            seen.append((n, changed))
            assert 4 * changed >= n, (q, ad, n, changed)
        print(f"q{q} a{ad}: (entries, of them changing the block's size when flipped) {seen}")


def test_near_flat_blocks_are_not_constant():
    """Every near-flat block differs from a constant in one pixel by one; at q50 the oracle's DC of
    such a block differs from the constant block's for many of them (the odd levels' exact ties:
    +-1/8 decides the side), so taking the constant-block table for them cannot go unseen."""
    import oracle as O
    blocks, const = PF.near_flat()
    flat = blocks.reshape(-1, 64)
    assert np.array_equal((flat == flat[:, :1]).all(1), const)
    nf = flat[~const].astype(int)
    level = np.median(nf, axis=1).astype(int)
    assert ((nf != level[:, None]).sum(1) == 1).all() and (np.abs(nf - level[:, None]).max(1) == 1).all()
    assert 256 * 4 <= const.sum() < 256 * 5 and set(level.tolist()) == set(range(256))
    dc = O.forward_plane(PF.plane(blocks), 50, 0)[:, 0]
    dc_const = O.forward_plane(PF.plane(np.repeat(np.arange(256, dtype=np.uint8), 16)[:, None, None]
                                        * np.ones((1, 8, 8), np.uint8)), 50, 0)[:, 0]
    differ = int((dc[~const] != dc_const[~const]).sum())
    print(f"near_flat: {int((~const).sum())} near-flat blocks, {int(const.sum())} constant; q50 DC differs from "
          f"the constant block's in {differ}")
    assert differ >= 256


def test_range_edge_reaches_the_plan_bound():
    """The two sign patterns of basis (u, v) reach max_quantized's bound floor(cmax / Q + 0.5),
    cmax = 128 L1(D_u) L1(D_v), wherever rounding allows: wherever the largest |coefficient| a u8
    block has there (127 on one sign, 128 on the other) rounds to the same integer.  The DC
    gives -1024 (all 0) and 1016 (all 255) at q100."""
    import oracle as O
    blocks = PF.range_edge()
    assert blocks.shape == (128, 8, 8) and set(np.unique(blocks).tolist()) == {0, 255}
    px = PF.plane(PF.pad(blocks))
    k = np.arange(64)
    for q in (1, 10, 50, 90, 100):
        Q = IB.quant_table(q)
        qmax = np.floor(IB.coef_max() / Q + 0.5)
        got, f = O.forward_plane(px, q, 0, want_float=True)
        got, f = got[:128].astype(int), f[:128]
        own = np.abs(got.reshape(64, 2, 64)[k, :, k]).max(1)   # |q_k| of the two blocks built for k
        quo = np.abs(f.reshape(64, 2, 64)[k, :, k]).max(1) / Q
        allowed = (np.floor(quo + 0.5) == qmax) & (np.abs(quo - np.floor(quo) - 0.5) > 1e-6)  # a tie may go either way
        print(f"q{q}: bound reached at {int((own == qmax).sum())} of 64 coefficients, rounding allows {int(allowed.sum())}")
        assert (own <= qmax).all() and (np.abs(got) <= qmax[None, :]).all()
        assert (own[allowed] == qmax[allowed]).all()
        # how many must reach it: a coarse table hides the 127/128 between the two signs, a fine one
        # shows it everywhere but at the DC, whose all-0 block is exactly -1024
        assert allowed.sum() >= {1: 64, 10: 60, 50: 48, 90: 32, 100: 1}[q], (q, int(allowed.sum()))
    assert got[:, 0].min() == -1024 and got[:, 0].max() == 1016
