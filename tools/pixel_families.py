"""u8 pixel blocks built to sit on exact rounding ties of the forward path: the inputs of
tests/test_pixel_families_cpu.py (which checks the generators against the oracle) and of
tests/test_pixel_ties_gpu.py (which runs them through every kernel that resolves ties).

With s = [1,-1,-1,1,1,-1,-1,1] the block  128 + d + a s(x) + b s(y) + c s(x) s(y)  has the
exact coefficients 8d at (0,0), 8a at (0,4), 8b at (4,0), 8c at (4,4) and 0 elsewhere, and
the exact variance a^2 + b^2 + c^2: u, v in {0, 4} are the only positions whose basis is
rational.  Where 16 amp / M is an odd integer for the plan's divisor M (Q, or Q (2 - nv) for
an adaptive plan) the real quotient is exactly k + 0.5, and the side the reference lands on
is decided by its own fp64 noise -- the only inputs on which a tie path's summation order,
row/column roles and divisor formula can be told from the reference's.

Every generator is deterministic given its rng.  A "tie" is defined operationally: the
oracle's fp64 coefficient divided by the divisor the oracle uses lies within 2^-40 relative
of a half-integer (true_ties).  numpy and the oracle only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S = np.array([1, -1, -1, 1, 1, -1, -1, 1])  # D[4][k] * 2 sqrt 2
T = np.array([1, 1, -1, -1, -1, -1, 1, 1])  # orthogonal to 1 and to S: frequencies 2 and 6 only
DC, H, V, HV = 0, 4, 32, 36                 # (0,0) (0,4) (4,0) (4,4); processing slots 0, 32, 8, 40
POSITIONS = (DC, H, V, HV)
TIE_EPS = 2.0 ** -40
AMP = 32        # |a|, |b|, |c| of the search grid
ENTRY_COUNTS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 128, 256)


def _oracle():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import oracle
    return oracle


def quant_table(q):
    """The plan's 64 divisors, from the oracle (src/quantization.c:51-99)."""
    return _oracle().quant_matrix(8, min(max(int(q), 1), 100)).ravel()


def plane(blocks, bw=64):
    """u8 blocks [n, 8, 8] -> the plane [n / bw * 8, bw * 8] whose raster block order is theirs."""
    n = blocks.shape[0]
    assert n % bw == 0, (n, bw)
    return np.ascontiguousarray(blocks.reshape(n // bw, bw, 8, 8).transpose(0, 2, 1, 3).reshape(n // bw * 8, bw * 8))


def pad(blocks, bw=64, level=128):
    """Constant blocks up to a multiple of bw."""
    n = -(-blocks.shape[0] // bw) * bw
    return np.concatenate([blocks, np.full((n - blocks.shape[0], 8, 8), level, np.uint8)])


def transposed(blocks):
    """Every block transposed (rows <-> columns), block order kept."""
    return np.ascontiguousarray(blocks.transpose(0, 2, 1))


def divisors(blocks, q, adaptive):
    """[n, 64] the divisor the oracle's quantize uses for every coefficient: Q, or for an
    adaptive plan Q (2 - nv) clamped to >= 1 with the DC keeping Q (oracle.adjust)."""
    Q = quant_table(q)
    if not adaptive:
        return np.broadcast_to(Q, (blocks.shape[0], 64))
    O = _oracle()
    var = O.plane_variance(plane(pad(blocks)))[:blocks.shape[0]]
    levels, inv = np.unique(var, return_inverse=True)
    return np.stack([O.adjust(Q.reshape(8, 8), float(v), 1).ravel() for v in levels])[inv]


def quotients(blocks, q, adaptive):
    """(quantized int16 [n, 64], fp64 quotient [n, 64]) of the oracle."""
    O = _oracle()
    got, f = O.forward_plane(plane(pad(blocks)), q, adaptive, want_float=True)
    n = blocks.shape[0]
    return got[:n], f[:n] / divisors(blocks, q, adaptive)


def tie_mask(blocks, q, adaptive):
    """(ties [n, 64] bool, against [n, 64] bool): the oracle's quotient within 2^-40 relative
    of a half-integer, and among those the ones the oracle does not round half away from zero."""
    got, quo = quotients(blocks, q, adaptive)
    half = np.floor(quo) + 0.5
    ties = np.abs(quo - half) <= TIE_EPS * np.abs(half)
    away = np.sign(half) * np.ceil(np.abs(half))
    return ties, ties & (got != away)


def true_ties(blocks, q, adaptive, positions=POSITIONS):
    """The (block, coefficient) pairs of tie_mask at the constructed positions."""
    ties, _ = tie_mask(blocks, q, adaptive)
    b, c = np.nonzero(ties[:, list(positions)])
    return [(int(i), int(positions[j])) for i, j in zip(b, c)]


def _half(quo):
    return np.abs(quo - (np.floor(quo) + 0.5)) < 1e-9


def _tie_amps(Qp, lim=100):
    """Integer amplitudes with 8 amp / Q a half-integer (16 amp / Q odd), by |amp|."""
    a = np.arange(-lim, lim + 1)
    a = a[_half(8.0 * a / Qp)]
    return a[np.argsort(np.abs(a), kind="stable")]


def _grid(Q, adaptive):
    """The amplitude triples searched: every |amp| <= AMP for an adaptive plan (its ties depend
    on all three through the variance), |amp| <= 10 otherwise, plus on each axis the amplitudes
    up to 64 that tie against the unscaled Q; |a| + |b| + |c| <= 110."""
    r = np.arange(-AMP, AMP + 1) if adaptive else np.arange(-10, 11)
    axes = [np.union1d(r, _tie_amps(Q[p], 64)) for p in (H, V, HV)]
    a, b, c = [x.ravel() for x in np.meshgrid(*axes, indexing="ij")]
    keep = np.abs(a) + np.abs(b) + np.abs(c) <= 110
    return a[keep], b[keep], c[keep]


def _candidates(Q, adaptive, tex_var=0.0):
    """The amplitude triples (a, b, c) of the search grid with their tie flags [m, 3] at
    (0,4), (4,0), (4,4) under the divisor of a block of variance a^2 + b^2 + c^2 + tex_var."""
    a, b, c = _grid(Q, adaptive)
    scale = 1.0
    if adaptive:
        var = (a * a + b * b + c * c) + tex_var
        scale = 2.0 - np.minimum(1.0, np.maximum(0.1, var / 1000.0))
    flags = np.stack([_half(8.0 * amp / np.maximum(Q[p] * scale, 1.0)) & (amp != 0)
                      for amp, p in ((a, H), (b, V), (c, HV))], axis=1)
    return np.stack([a, b, c], axis=1), flags


def tie_positions(q, adaptive):
    """The positions among (0,0), (0,4), (4,0), (4,4) at which the search grid of rational()
    holds a tie for this plan."""
    Q = quant_table(q)
    _, flags = _candidates(Q, adaptive)
    out = [DC] if len(_tie_amps(Q[DC])) else []
    return out + [p for k, p in enumerate((H, V, HV)) if flags[:, k].any()]


def _texture(rng):
    """e t(x) g(y) + e' g'(x) t(y) with small integer g, g': (pattern [8, 8] int, max |.|, variance)."""
    while True:
        g1, g2 = rng.integers(-3, 4, 8), rng.integers(-3, 4, 8)
        e1, e2 = rng.integers(0, 4, 2)
        tex = e1 * np.outer(g1, T) + e2 * np.outer(T, g2)  # [y, x]
        if tex.any() and (tex * tex).sum() % 64 == 0:  # an integer variance keeps adaptive ties within reach
            return tex, int(np.abs(tex).max()), float((tex * tex).sum()) / 64.0


def _subsets(k):
    return [[j for j in range(k) if m >> j & 1] for m in range(1, 1 << k)]


def _build(q, adaptive, n, rng, textures):
    """n blocks cycling through every non-empty subset of the positions that admit a tie;
    textures: list of (pattern, max, variance), block i takes textures[i % len]."""
    Q = quant_table(q)
    dc_amps = _tie_amps(Q[DC])
    blocks = np.empty((n, 8, 8), np.uint8)
    sx, sy = np.broadcast_to(S[None, :], (8, 8)), np.broadcast_to(S[:, None], (8, 8))
    sxy = sx * sy
    for t, (tex, tmax, tvar) in enumerate(textures):
        idx = np.arange(t, n, len(textures))
        abc, flags = _candidates(Q, adaptive, tvar)
        room = np.abs(abc).sum(1) + tmax
        abc, flags, room = abc[room <= 126], flags[room <= 126], room[room <= 126]
        admit = [k for k in range(3) if flags[:, k].any()]
        subs = _subsets(len(admit) + (1 if len(dc_amps) else 0))
        rows_of = []
        for sub in subs:
            need = [admit[k] for k in sub if k < len(admit)]
            pick = np.ones(len(abc), bool)
            for k in need:
                pick &= flags[:, k]
            if len(admit) in sub:
                pick &= room + np.abs(dc_amps[0]) <= 127
            rows = np.nonzero(pick)[0]
            if len(rows) == 0:      # these positions never tie together: any triple with the first of them
                rows = np.nonzero(flags[:, need[0]] if need else np.ones(len(abc), bool))[0]
            rows_of.append(rows)
        if not subs:
            subs, rows_of = [[]], [np.arange(len(abc))]
        for j, i in enumerate(idx):
            sub, rows = subs[j % len(subs)], rows_of[j % len(subs)]
            want_dc = len(admit) in sub and len(dc_amps) > 0
            r = rows[rng.integers(len(rows))]
            a, b, c = abc[r]
            left = 127 - room[r]
            ds = dc_amps[np.abs(dc_amps) <= left] if want_dc else np.empty(0, int)
            d = ds[rng.integers(len(ds))] if len(ds) else rng.integers(-left, left + 1)
            px = 128 + d + a * sx + b * sy + c * sxy + tex
            assert px.min() >= 0 and px.max() <= 255
            blocks[i] = px
    return blocks


def rational(q, adaptive, n, rng):
    """(blocks [n, 8, 8] u8, ties): the four-amplitude blocks above, amplitudes steered to the
    plan's table so that the positions tie in every combination the plan admits -- one to four
    ties per block, in the first flag word only ((0,0), (4,0)), the second only ((0,4), (4,4))
    and both.  ties: the (block, coefficient) pairs that are true ties by the oracle."""
    blocks = _build(q, adaptive, n, rng, [(np.zeros((8, 8), int), 0, 0.0)])
    return blocks, true_ties(blocks, q, adaptive)


def textured(q, adaptive, n, rng, ntex=2):
    """rational() plus e t(x) g(y) + e' g'(x) t(y): t is orthogonal to 1 and to s, so the four
    rational coefficients keep their exact values while the others become ordinary non-zero
    ones, the variance moves, and the fp64 noise around each tie changes."""
    blocks = _build(q, adaptive, n, rng, [_texture(rng) for _ in range(ntex)])
    return blocks, true_ties(blocks, q, adaptive)


def var_num(blocks):
    """64 sum x^2 - (sum x)^2 of every block (x = px - 128): 4096 times the exact variance."""
    x = blocks.reshape(-1, 64).astype(np.int64) - 128
    return 64 * (x * x).sum(1) - x.sum(1) ** 2


VAR_EDGES = (409600, 4096000)  # var = 100 and var = 1000: the clamp edges of nv


def _s_block(d, a, b, c):
    sx, sy = S[None, :], S[:, None]
    px = 128 + d + a * sx + b * sy + c * sx * sy
    assert px.min() >= 0 and px.max() <= 255
    return px.astype(np.uint8)


VAR_STEPS = (-1, 7)  # the nearest attainable var_num below and above either edge (_nearest)


def _nearest(base, target, lim=45):
    """64 centred pixels x = px - 128 with 64 s2 - s1^2 == target: the 60 values of `base` plus
    four free ones in [-lim, lim], found by meeting two pair tables (sum, sum of squares) in the
    middle; the first hit in a fixed order, so the block is the same on every run.
    var_num = 64 s2 - s1^2 with s2 = s1 (mod 2).  Below an edge E = 0 (mod 128) the nearest value
    is E - 1 (s1^2 = 1 (mod 64) with s2 odd: s1 = 31 does).  Above, E + d needs s1^2 = -d (mod 64):
    squares mod 64 are 0, 1, 4, 9, 16, 17, 25, 33, 36, 41, 49, 57, so d = 7 (s1^2 = 57: s1 = 21, with s2
    odd) is the smallest step -- none of 63 .. 58 is a square.  tests/test_pixel_families_cpu.py
    enumerates this."""
    base = np.asarray(base, np.int64)
    assert base.size == 60
    b1, b2 = int(base.sum()), int((base * base).sum())
    r = np.arange(-lim, lim + 1)
    i, j = np.triu_indices(len(r))
    pa, pb = r[i], r[j]
    p, q = pa + pb, pa * pa + pb * pb
    for lo in range(0, len(p), 256):
        s1 = b1 + p[lo:lo + 256, None] + p[None, :]
        s2 = b2 + q[lo:lo + 256, None] + q[None, :]
        hit = np.argwhere(64 * s2 - s1 * s1 == target)
        if len(hit):
            u, v = int(hit[0][0]) + lo, int(hit[0][1])
            x = np.concatenate([base, [pa[u], pb[u], pa[v], pb[v]]])
            assert 64 * int((x * x).sum()) - int(x.sum()) ** 2 == target
            return (x + 128).astype(np.uint8).reshape(8, 8)
    raise ValueError("no block with var_num %d" % target)


_edges = {}


def variance_edges():
    """Blocks whose var_num is exactly 409600 (var = 100) and 4096000 (var = 1000) and the nearest
    attainable var_num below and above each (edge - 1 and edge + 7, _nearest), each in several
    arrangements: the s-patterns (rational coefficients, so ties meet the clamp edge) and
    shuffles of their pixels; the nearest neighbours, which no s-pattern reaches, as found and
    shuffled.  Returns (blocks, var_num per block); the same blocks on every call."""
    if "v" in _edges:
        return _edges["v"]
    rng = np.random.default_rng(1000)
    out = []
    # var = 100: 32 px at 118, 32 at 138 (a = 10) and (6, 8, 0) splits; var = 1000: 20 px at 168,
    # 20 at 88, 24 at 128 (two levels +-40 around 128) and the s-patterns with a^2+b^2+c^2 = 1000
    exact = [_s_block(d, *abc) for d in (0, 7, -16) for abc in
             ((10, 0, 0), (0, 10, 0), (0, 0, 10), (6, 8, 0), (0, 6, 8), (8, 0, -6))]
    exact += [_s_block(d, *abc) for d in (0, 5, -8) for abc in
              ((30, 10, 0), (10, 30, 0), (0, 10, 30), (18, 26, 0), (26, 0, 18), (0, -18, 26), (30, 0, -10))]
    lv = np.array([168] * 20 + [88] * 20 + [128] * 24, np.uint8)
    exact.append(lv.reshape(8, 8))
    exact.append(np.array([118] * 32 + [138] * 32, np.uint8).reshape(8, 8))
    for blk in exact:
        out.append(blk)
        for _ in range(2):
            out.append(rng.permutation(blk.reshape(64)).reshape(8, 8))
    bases = ([10] * 30 + [-10] * 30, [40] * 19 + [-40] * 19 + [0] * 22)
    for base, edge in zip(bases, VAR_EDGES):
        for step in VAR_STEPS:
            blk = _nearest(base, edge + step)
            out.append(blk)
            for _ in range(3):
                out.append(rng.permutation(blk.reshape(64)).reshape(8, 8))
    blocks = np.ascontiguousarray(np.stack(out), np.uint8)
    blocks.setflags(write=False)
    _edges["v"] = (blocks, var_num(blocks))
    return _edges["v"]


NEAR_FLAT_SPOTS = ((0, 0), (0, 7), (7, 0), (7, 7), (3, 2), (4, 5))  # (y, x): corners, centre, both words of a row


def near_flat():
    """For every level v the constant block with one pixel moved by +-1 at each of
    NEAR_FLAT_SPOTS, interleaved with true constant blocks: 16 blocks per level, 12 near-flat
    (at v = 0 and 255 the impossible direction stays constant) and 4 constant, so both kinds
    sit in every wave.  Returns (blocks [4096, 8, 8], constant [4096] bool)."""
    blocks = np.empty((256, 16, 8, 8), np.uint8)
    const = np.zeros((256, 16), bool)
    for v in range(256):
        blocks[v] = v
        const[v, 0::4] = True  # slots 0, 4, 8, 12 stay constant; the other twelve take (spot, sign)
        moves = [(y, x, sg) for (y, x) in NEAR_FLAT_SPOTS for sg in (1, -1)]
        for slot, (y, x, sg) in zip([s for s in range(16) if s % 4], moves):
            if 0 <= v + sg <= 255:
                blocks[v, slot, y, x] = v + sg
            else:
                const[v, slot] = True
    return blocks.reshape(4096, 8, 8), const.reshape(4096)


def range_edge():
    """For every (u, v) the 0/255 sign pattern of that basis function and its negation: the
    128 blocks that maximise |coefficient (u, v)| over u8 pixels, block 2 (8u + v) + negated."""
    O = _oracle()
    D = O.dct_matrix(8)
    out = []
    for u in range(8):
        for v in range(8):
            pos = np.outer(D[u], D[v]) > 0  # [y, x]
            out.append(np.where(pos, 255, 0))
            out.append(np.where(pos, 0, 255))
    return np.ascontiguousarray(np.stack(out), np.uint8)


def batched(blocks, entries_per_batch, ties=None, rng=None, prefer=None):
    """One 64-block batch per block row: row r holds blocks whose tie entries (their pairs in
    `ties`; one each when ties is None) number exactly entries_per_batch[r], at random lanes,
    the rest constant blocks (their DC goes to the constant-block table, their other
    coefficients are exactly 0).  Returns (plane blocks [64 rows, 8, 8], entries) with
    entries[r] the constructed (lane, coefficient) pairs of row r.  Raises ValueError where a
    count cannot be met (more than 64 blocks' worth of entries).  prefer: block ids that the rows of
    9..16 entries draw from where they can (batched_blocks: blocks a four-lane round's output shows)."""
    rng = rng or np.random.default_rng(77)
    per = {}
    if ties is None:
        per = {i: [DC] for i in range(len(blocks))}
    else:
        for b, c in ties:
            per.setdefault(b, []).append(c)
    by_count = {}
    for b, cs in per.items():
        by_count.setdefault(len(cs), []).append(b)
    kmax = max(by_count) if by_count else 0
    used = {k: 0 for k in by_count}
    every = by_count
    liked = {k: [b for b in bs if b in prefer] for k, bs in by_count.items()} if prefer else {}
    liked = {k: bs for k, bs in liked.items() if bs}
    used_liked = {k: 0 for k in liked}
    out = np.empty((len(entries_per_batch) * 64, 8, 8), np.uint8)
    entries = []
    for r, want in enumerate(entries_per_batch):
        if want > 64 * kmax:
            raise ValueError("%d entries need more than 64 blocks of at most %d ties" % (want, kmax))
        chosen, left = [], want
        narrow = 9 <= want <= 16 and 1 in liked  # single-tie preferred blocks can fill any count
        by_count, cnt = (liked, used_liked) if narrow else (every, used)
        while left > 0:
            slots = 64 - len(chosen)
            ks = [k for k in by_count if k <= left and (left - k) <= (slots - 1) * max(by_count)
                  and ((left - k) == 0 or (left - k) >= min(by_count))]
            if not ks:
                raise ValueError("cannot split %d entries over the blocks given" % want)
            # a class in proportion to its blocks not placed yet, so a class of few blocks is not
            # repeated while others are fresh; a class is reused only once it is exhausted
            fresh = np.array([max(len(by_count[k]) - cnt[k], 0) for k in ks], float)
            k = ks[rng.choice(len(ks), p=fresh / fresh.sum())] if fresh.sum() else ks[rng.integers(len(ks))]
            chosen.append(by_count[k][cnt[k] % len(by_count[k])])
            cnt[k] += 1
            left -= k
        lanes = rng.choice(64, len(chosen), replace=False)
        row = np.empty((64, 8, 8), np.uint8)
        row[:] = rng.integers(0, 256, 64).astype(np.uint8)[:, None, None]
        ent = []
        for lane, b in zip(lanes, chosen):
            row[lane] = blocks[b]
            ent += [(int(lane), c) for c in per[b]]
        out[64 * r:64 * r + 64] = row
        entries.append(ent)
    return out, entries


# ---- the planes the two test files share --------------------------------------------------------
# Plans on which every exact implementation runs: non-adaptive plans whose ties fall at (0,4)
# (q25), the DC only (q50), (4,0) (q52), (4,4) (q60) and all four positions (q84: up to four
# entries per lane); adaptive plans with ties strictly between the clamp edges of nv (q6), at
# var = 100 (q50: the DCs of variance_edges, the only position that can tie there -- 16 amp /
# (1.9 Q) odd needs 19 | amp, and 19^2 > 100) and at var = 1000 (q60: (0,4) of variance_edges);
# and q41 adaptive, whose (0,4) ties change sides when var / 1000.0 becomes var * 0.001.
EXACT_PLANS = ((25, 0), (50, 0), (52, 0), (60, 0), (84, 0), (6, 1), (50, 1), (60, 1), (41, 1))
_planes = {}


def sweep_blocks(q, adaptive, n=512):
    """(blocks [2n, 8, 8], ties): rational + textured for one plan, seeded by the plan."""
    key = ("sweep", q, adaptive, n)
    if key not in _planes:
        rng = np.random.default_rng(2 * q + adaptive)
        blocks = np.concatenate([rational(q, adaptive, n, rng)[0], textured(q, adaptive, n, rng)[0]])
        blocks.setflags(write=False)
        _planes[key] = (blocks, true_ties(blocks, q, adaptive))
    return _planes[key]


def tie_blocks(q, adaptive):
    """sweep_blocks plus variance_edges (ties at the clamp edges of nv where the plan has them)."""
    key = ("tie", q, adaptive)
    if key not in _planes:
        blocks = np.concatenate([sweep_blocks(q, adaptive)[0], variance_edges()[0]])
        blocks.setflags(write=False)
        _planes[key] = (blocks, true_ties(blocks, q, adaptive))
    return _planes[key]


def size_sensitive(blocks, ties, q, adaptive):
    """The blocks with a tie whose other side changes the block's Huffman size (oracle): the only
    blocks on which an output of per-block sizes shows how that tie was resolved."""
    O = _oracle()
    got, quo = quotients(blocks, q, adaptive)
    bits = O.huffman_bits_plane(got)
    out = set()
    for b, c in ties:
        alt = got[b].copy()
        alt[c] = np.int16(2 * (np.floor(quo[b, c]) + 0.5) - got[b, c])  # floor <-> ceil of the half-integer
        if O.huffman_bits(alt.reshape(8, 8)) != int(bits[b]):
            out.add(b)
    return out


def batched_blocks(q, adaptive):
    """(blocks [64 r, 8, 8], entries per row, counts): tie_blocks laid out one batch per row with
    0 and every count of ENTRY_COUNTS the plan's ties can fill (twice, in two orders)."""
    key = ("batched", q, adaptive)
    if key not in _planes:
        blocks, ties = tie_blocks(q, adaptive)
        per = np.bincount([b for b, _ in ties], minlength=1)
        counts = [c for c in ENTRY_COUNTS if c <= 64 * per.max()]
        counts = [0] + counts + counts[::-1]
        out, entries = batched(blocks, counts, ties, np.random.default_rng(100 * q + adaptive),
                               prefer=size_sensitive(blocks, ties, q, adaptive))
        out.setflags(write=False)
        _planes[key] = (out, entries, counts)
    return _planes[key]
