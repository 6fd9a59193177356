"""CPU: the inputs of tests/test_window_scaled_foreign_gpu.py -- the window decoder
(dctq_decode_bits_window_planes) and the scaled decoder (dctq_decode_bits_window_scaled_planes) on
blocks, var_num and tables no forward of ours produced -- built and checked with no device: every
layout and share condition the GPU module relies on is asserted here, on the references alone.

Every stream is packed on the host (tools/bits_ref.py pack; blocks that hold a bad code or a cut
last code are assembled from the same symbol_bits, bit string by bit string) and the expected
coefficients are bits_ref's own decode of those bytes: no kernel of ours is in the yardstick.

Part 1, the catalogue.  The scaled decoder's bit walk stops once the position has reached END =
25, 5, 1 (n = 4, 2, 1): the catalogue puts values of both signs at zigzag position END - 1 (the
corner's last: natural (3,3), (1,1), (0,0)), at END (natural (2,4), (0,2), (0,1): outside), at
both; first runs of 1, 5, 25, 63, 64 and 65535; runs that jump over END and over 63; zero values
inside the corner; empty, all-zero, 64-symbol and 368-byte blocks; a bad code right after and
right before the symbol at END - 1, and a last code cut by the block's length.  Layout: one plane
(2, 8 C, 1040), C the catalogue's size, 130 blocks a row (runs of 64, 64 and 2).  Frame 0 holds
catalogue block (r + j) mod C at row r, column j, so every block sits in every lane of every
run, and alone in the run of a 1-wide window; frame 1 is the same with the first half of each
row's first run filled with 368-byte neighbours (six chunks of the 2 560 B stage) around three
catalogue blocks, in its first, a middle and its last chunk.

Part 2, in-range shares of the scaled decoder's reference (scaled_ref.unrounded strictly inside
(0, 255)), per cent, for int16 / pm511 / range_x1 / range_x4 / range_x32 / sparse, adaptive plans
with TF.plain_var_num (test_family_shares prints them and asserts the best of every row >= 25):
    (1,0)    s2 100.0 100.0 100.0 100.0 100.0 100.0    s4 100.0 100.0 100.0 100.0 100.0 100.0    s8 100.0 100.0 100.0 100.0 100.0 100.0
    (50,0)   s2  15.6 100.0 100.0 100.0  99.6  96.9    s4  25.1 100.0 100.0 100.0 100.0  98.9    s8  51.0 100.0 100.0 100.0 100.0  99.7
    (72,0)   s2   8.8 100.0 100.0 100.0  62.9  94.4    s4  14.3 100.0 100.0 100.0  84.1  98.2    s8  28.3 100.0 100.0 100.0 100.0  99.5
    (100,0)  s2   1.1  60.4  37.1   9.7   1.3  85.0    s4   2.0  91.8  64.2  17.8   2.6  96.2    s8   3.2 100.0  99.6  25.8   3.2  98.9
    (50,1)   s2   0.0   3.5  32.0   8.2   1.0  73.4    s4   0.1   8.8  57.8  15.7   2.3  93.2    s8   0.2  12.6  99.2  25.7   3.2  98.1
    (100,1)  s2   0.9  52.9  32.1   8.2   1.1  84.4    s4   1.8  85.5  57.8  15.6   2.2  96.0    s8   3.2 100.0  99.6  25.8   3.2  98.9
    (1,1)    s2   0.0   0.2  31.8   8.3   1.1  62.8    s4   0.0   0.4  55.5  15.1   1.9  90.1    s8   0.0   0.8  94.0  25.9   3.4  97.4
Part 5, ties.  n = 1 with Q00 a power of two and n = 4 with coefficients at (0,0), (0,2), (2,0),
(2,2) only are exact in fp64, so R = k + 0.5 exists and the expected pixel is stated with
rationals: the even neighbour.  For n = 2 the literal r = 0x1.6a09e667f3bcdp-1 is not dyadic and
r * r != 0.5, so no R is an exact tie by construction; tests/golden/scaled_n2_near_ties.npy holds
256 corners whose R is within a few ulp of a half, 128 from either side (the search is
tests/golden/make_scaled_n2_near_ties.py)."""
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bits_ref  # noqa: E402
import coef_families as CF  # noqa: E402
import scaled_ref  # noqa: E402
import window_ref  # noqa: E402
import test_custom_tables_gpu as TC  # noqa: E402
import test_decode_foreign_gpu as TF  # noqa: E402

STAGE = 2560           # bits_core.h kBitsStage
ENDS = {4: 25, 2: 5, 1: 1}   # n -> the walk's end (decode_scaled.hip corner_end)
SCALES = (2, 4, 8)
ZZ = np.array(bits_ref.ZIGZAG)
BAD = "0" * 17 + "1"   # a prefix of more than 16 zero bits
U = 2.0 ** -24
SCALED_PLANS = [(1, 0), (50, 0), (72, 0), (100, 0), (50, 1), (100, 1), (1, 1)]
TABLES = ["scaled", "flat137", "ramp", "checker", "edge511", "edge512", "std50", "std100"]
TABLE_KINDS = ["noise", "quarter", "smooth"]
MAG = {(100, 0): 8, (50, 1): 1}   # the catalogue's value unit per plan: Q = 1 needs values a pixel shows


def std_table(q):
    import oracle as O
    return O.quant_matrix(8, q)


def corner_mask(n):
    m = np.zeros((8, 8), bool)
    m[:n, :n] = True
    return m.ravel()


# ---- blocks as bit strings -------------------------------------------------------------------------
class Blk:
    """items: (value, run) symbols and raw bit strings, in order; cut: bytes dropped from the end."""

    def __init__(self, name, items, cut=0):
        self.name, self.items, self.cut = name, list(items), cut

    def data(self):
        bits = "".join(bits_ref.symbol_bits(*it) if isinstance(it, tuple) else it for it in self.items)
        bits += "0" * (-len(bits) % 8)
        raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
        return raw[:len(raw) - self.cut]

    def pure(self):
        return not self.cut and all(isinstance(it, tuple) for it in self.items)

    def without(self, i):
        """The block with its i-th symbol (raw strings are not counted) taken out."""
        k, items = -1, []
        for it in self.items:
            k += isinstance(it, tuple)
            if not (isinstance(it, tuple) and k == i):
                items.append(it)
        last = i == sum(isinstance(it, tuple) for it in self.items) - 1
        return Blk(self.name, items, 0 if last else self.cut)   # a cut tail goes with its symbol

    def landings(self):
        """(position or None if never read, value) of every symbol: the walk of tools/bits_ref.py."""
        syms = [it for it in self.items if isinstance(it, tuple)]
        out, pos, alive, k = [], 0, True, 0
        for it in self.items:
            if not isinstance(it, tuple):
                alive = False
                continue
            last = k == len(syms) - 1
            k += 1
            if not alive or pos >= 64 or k > 64 or (self.cut and last):
                alive = alive and not (self.cut and last)
                out.append((None, it[0]))
                continue
            pos += min(it[1], 64)
            out.append((pos, it[0]))
            pos += 1
        return out


def decode(blks):
    return bits_ref.unpack(*pack_raw([b.data() for b in blks]))


def pack_raw(datas):
    off = np.cumsum([0] + [len(d) for d in datas]).astype(np.uint32)
    return np.frombuffer(b"".join(datas) or b"", np.uint8).copy(), off


# 368 B as the catalogue's own, but told apart by its last value code (m = 65535: the other 33-bit code)
NEIGHBOUR = Blk("368 B neighbour", [(-32768, 64)] * 63 + [(32768, 64)])


@functools.lru_cache(maxsize=None)
def catalogue(m):
    """The catalogue with values in units of m."""
    rng = np.random.default_rng(7)
    cat = []
    for n, E in ENDS.items():
        t = f"n{n} "
        cat += [
            Blk(t + "+ at END-1", [(5 * m, E - 1)]), Blk(t + "- at END-1", [(-7 * m, E - 1)]),
            Blk(t + "+ at END", [(6 * m, E)]), Blk(t + "- at END", [(-9 * m, E)]),
            Blk(t + "+- at END-1, END", [(5 * m, E - 1), (-8 * m, 0)]),
            Blk(t + "-+ at END-1, END", [(-6 * m, E - 1), (7 * m, 0)]),
            Blk(t + "jump over END", [(4 * m, 0), (9 * m, E + 2)]),
            Blk(t + "jump past 63, run 64", [(5 * m, E - 1), (-6 * m, 64)]),
            Blk(t + "jump past 63, lands at 70", [(-5 * m, E - 1), (6 * m, 70 - E)]),
            Blk(t + "bad code after END-1", [(5 * m, E - 1), BAD, (7 * m, 0)]),
            Blk(t + "bad code before END-1", ([(4 * m, 0), BAD, (6 * m, E - 2)] if E > 1 else [BAD, (6 * m, 0)])),
            Blk(t + "last code cut", ([(4 * m, 0), (-900 * m, E - 2)] if E > 1 else [(-900 * m, 0)]), cut=1),
        ]
    for k, r in enumerate((1, 5, 25, 63, 64, 65535)):   # 65535 is packed as 64: its values tell the two apart
        cat.append(Blk(f"first run {r}", [((5 + k) * m, r), (-7 * m, 0)]))
    dense = [(int(v) * m, 0) for v in rng.integers(2, 10, 64) * rng.choice([-1, 1], 64)]
    cat += [
        Blk("zero at 1 between 0 and 2", [(5 * m, 0), (0, 0), (-7 * m, 0)]),
        Blk("zeros at 2 and 23, values at 0, 3, 24", [(5 * m, 0), (0, 1), (-7 * m, 0), (0, 19), (6 * m, 0)]),
        Blk("zero at 0, value at 1", [(0, 0), (5 * m, 0)]),
        Blk("empty", []),
        Blk("all-zero", [(0, 64)]),
        Blk("64 symbols run 0", dense),
        Blk("64 symbols run 0, ends of int16", [((32767, -32768)[i & 1], 0) for i in range(64)]),
        Blk("368 B", [(-32768, 64)] * 64),
    ]
    assert len(cat[-1].data()) == 368 and len({b.name for b in cat}) == len(cat)
    return cat


@functools.lru_cache(maxsize=None)
def catalogue_layout():
    """slot [2, C, 130]: the catalogue index of every stored block (C: the neighbour)."""
    C = len(catalogue(1))
    r, j = np.indices((C, 130))
    slot = np.stack([(r + j) % C, (r + j) % C])
    slot[1, :, :32] = C
    for k, lane in enumerate((0, 15, 31)):
        slot[1, :, lane] = (np.arange(C) + k) % C
    slot.setflags(write=False)
    return slot


def catalogue_shape():
    return (2, 8 * len(catalogue(1)), 1040)


def catalogue_windows():
    f, h, w = catalogue_shape()
    return {"whole": [((0, f), (0, h), (0, w))],
            "origin not block 0": [((0, f), (8, h), (24, w))],
            "1 wide": [((0, f), (0, h), (w - 8, w))]}


@functools.lru_cache(maxsize=None)
def catalogue_stream(m):
    """dict(bytes, off, coef): the laid-out stream and bits_ref's decode of the catalogue's blocks, per slot."""
    cat = list(catalogue(m)) + [NEIGHBOUR]
    datas = [b.data() for b in cat]
    for b, d in zip(cat, datas):
        if b.pure():
            assert bytes(bits_ref.pack([b.items])[0]) == d, b.name
    slot = catalogue_layout().ravel()
    data, off = pack_raw([datas[s] for s in slot])
    coef = decode(cat)[slot]
    for a in (data, off, coef):
        a.setflags(write=False)
    return dict(bytes=data, off=off, coef=coef)


def chunks_of(off, h0, h1):
    """The chunks bits_rebuild_half cuts blocks [h0, h1) of a run into: whole blocks that end inside the
    stage, counted from the first block's dword (bits_core.h); the stream's base is dword aligned."""
    off = np.asarray(off).astype(np.int64)
    out, s = [], h0
    while s < h1:
        room = STAGE - (off[s] & 3)
        e = s
        while e < h1 and off[e + 1] - off[s] <= room:
            e += 1
        e = max(e, s + 1)
        out.append((s, e))
        s = e
    return out


def bound64(coef, mult, want):
    """The fp64 path's pixel bound of include/dct_amd.h, as TF.reference and TC.inverse_ref state it."""
    import inv_bound as IB
    sx = IB.block_magnitudes(coef, mult).sum(axis=1, keepdims=True)
    return U * np.maximum(np.abs(want), 128.0) + 1e-9 * np.maximum(1.0, sx / 1024.0)


def oracle_ref(coef, Q, ad, vn, quality=0, table=True):
    """(reference recon + 128 [n, 64], fp64-path bound [n, 64]) of any coefficients under a table."""
    import oracle as O
    Q = np.asarray(Q, np.float64).ravel()
    coef = np.ascontiguousarray(coef)
    kw = {"table": Q} if table else {}
    if ad:
        var = np.asarray(vn) / 4096.0
        want = O.inverse_plane(coef, quality, 1, var, **kw) + 128.0
        nv = np.minimum(1.0, np.maximum(0.1, var / 1000.0))
        mult = Q[None, :] * (2.0 - nv)[:, None]
        mult[:, 0] = Q[0]
    else:
        want = O.inverse_plane(coef, quality, 0, **kw) + 128.0
        mult = (1.0 / Q)[None, :]
    return want, bound64(coef, mult, want)


# ---- streams of coefficients -----------------------------------------------------------------------
def pack_coef(coef):
    """int16 [n, 64] -> (bytes, offsets, bits_ref's decode): the reference run-length coder's symbols, packed."""
    import oracle as O
    off, sym = O.rle_encode_plane(np.ascontiguousarray(coef, np.int16))
    data, boff = bits_ref.pack(bits_ref.blocks_of(sym, off))
    back = bits_ref.unpack(data, boff)
    for a in (data, boff, back):
        a.setflags(write=False)
    return data, boff, back


@functools.lru_cache(maxsize=None)
def _family_stream(name, qkey):
    off, sym, _ = TF.streams(name, qkey)
    data, boff = bits_ref.pack(bits_ref.blocks_of(sym, off))
    back = bits_ref.unpack(data, boff)
    for a in (data, boff, back):
        a.setflags(write=False)
    return data, boff, back


def family_stream(name, q):
    """(bytes, offsets, decoded coefficients) of CF.family(name, q); families that do not depend on q share one."""
    return _family_stream(name, q if name.startswith("range_x") or name == "at_range_edge" else 50)


def family_windows(shape):
    h, w = shape
    return {"whole": [((0, 1), (0, h), (0, w))], "interior": [((0, 1), (8, h), (8, w))]}


# Part 3: 4 096 blocks as 2 frames of 16 x 128 blocks (two runs a row), a window whose first frame, row and column
# are not 0
VAR_SHAPE = (2, 128, 1024)
VAR_WINDOW = [((1, 2), (8, 128), (24, 1024))]
VAR_FAMILIES = ["pm511", "range_x1"]


# Part 4
@functools.lru_cache(maxsize=None)
def table_corner_blocks():
    """Part-1-style blocks for caller tables: values that are no multiples of any Q at END - 1 and END of every
    n, in every corner position at once, and at the ends of the 2-byte range."""
    rng = np.random.default_rng(11)
    c = np.zeros((16, 64), np.int16)
    for i, (n, E) in enumerate(ENDS.items()):
        c[2 * i, ZZ[E - 1]], c[2 * i, ZZ[E]] = 37, -53
        c[2 * i + 1, ZZ[E - 1]], c[2 * i + 1, ZZ[E]] = -211, 307
    c[6:12, :] = rng.integers(-97, 98, (6, 64))
    c[12, ZZ[:25]] = rng.integers(-511, 512, 25)
    c[13, ZZ[:5]] = [511, -512, 333, 0, -77]
    c[14, 0] = 1
    c[15, ZZ[24]] = -1
    c.setflags(write=False)
    return c


TABLE_SHAPES = [(1, 40, 104), (1, 8, 8), (1, 8, 128)]
TABLE_WINDOWS = {"whole": [((0, 1), (0, h), (0, w)) for _, h, w in TABLE_SHAPES],
                 "interior": [((0, 1), (8, 40), (8, 96)), ((0, 1), (0, 8), (0, 8)), ((0, 1), (0, 8), (24, 128))]}


@functools.lru_cache(maxsize=None)
def table_stream(tname, ad, kind):
    """The picture's coefficients under the table (TC.forward_ref) and the corner blocks as a third plane:
    dict(bytes, off, coef (bits_ref's decode), vn, want, e)."""
    Q = TC.tables()[tname]
    coef = np.concatenate(list(TC.forward_ref(tname, ad, kind)[0]) + [table_corner_blocks()])
    want, vn, tol64 = TC.inverse_ref(tname, ad, kind)
    vn2 = TF.plain_var_num(16)
    want2, tol2 = oracle_ref(table_corner_blocks(), Q, ad, vn2)
    data, boff, back = pack_coef(coef)
    assert np.array_equal(back, coef)
    want, vn, tol = np.concatenate([want, want2]), np.concatenate([vn, vn2]), np.concatenate([tol64, tol2])
    e = tol if ad else np.maximum(tol, 1e-4)   # as TC.test_inverse_and_decoders
    return dict(bytes=data, off=boff, coef=back, vn=vn, want=want, e=e, npic=len(tol64))


# ---- Part 5: ties ------------------------------------------------------------------------------------
def half_even(x):
    """The pixel of an exact R: clamp first, then round to nearest, ties to even."""
    return int(round(min(max(Fraction(x), Fraction(0)), Fraction(255))))


@functools.lru_cache(maxsize=None)
def ties_n1(q00, ad):
    """Blocks whose R = DC m / 8 + 128 (m = 1 / Q00, adaptive Q00) is k + 0.5 for k in 0..254, -0.5, 255.5, 0
    and the nearest DC on each side of every one of them: (coef [N, 64], pixels [N]).  Position 1 holds a value
    the walk must not place."""
    m = Fraction(q00) if ad else 1 / Fraction(q00)
    dcs = []
    for k2 in [-1] + [2 * k + 1 for k in range(255)] + [511, 0]:   # R = k2 / 2
        dc = (Fraction(k2, 2) - 128) * 8 / m
        assert dc.denominator == 1, (q00, ad, k2)
        dcs += [int(dc) - 1, int(dc), int(dc) + 1]
    coef = np.zeros((len(dcs), 64), np.int16)
    coef[:, 0] = dcs
    coef[:, 1] = 1000
    pix = np.array([half_even(Fraction(dc) * m / 8 + 128) for dc in dcs], np.uint8)
    return coef, pix


SGN = (1, -1, -1, 1)   # the signs of D4's row 2


@functools.lru_cache(maxsize=None)
def ties_n4():
    """Q = 1, coefficients at (0,0), (0,2), (2,0), (2,2): R[i][j] = (x00 + s_j x02 + s_i x20 + s_i s_j x22) / 8
    + 128 exactly.  x00 puts pixel (0, 0) on k + 0.5 (and one step to each side), the others are multiples of 4
    (every pixel a tie) or any (only some are): (coef [N, 64], pixels [N, 4, 4])."""
    rng = np.random.default_rng(13)
    rows = []
    for k2 in [-1] + [2 * k + 1 for k in range(255)] + [511, 0]:
        a, b, c = (int(v) for v in rng.integers(-10, 11, 3) * (4 if k2 % 4 == 1 else 1))
        for d in (-1, 0, 1):
            rows.append((4 * k2 - 1024 - a - b - c + d, a, b, c))
    coef = np.zeros((len(rows), 64), np.int16)
    coef[:, [0, 2, 16, 18]] = rows
    pix = np.array([[[half_even(Fraction(x00 + SGN[j] * a + SGN[i] * b + SGN[i] * SGN[j] * c, 8) + 128)
                      for j in range(4)] for i in range(4)] for x00, a, b, c in rows], np.uint8)
    return coef, pix


@functools.lru_cache(maxsize=None)
def near_ties_n2():
    """tests/golden/scaled_n2_near_ties.npy: int16 [256, 4], the corner (0,0), (0,1), (1,0), (1,1) -> coef [256, 64]."""
    corner = np.load(os.path.join(ROOT, "tests", "golden", "scaled_n2_near_ties.npy"))
    coef = np.zeros((len(corner), 64), np.int16)
    coef[:, [0, 1, 8, 9]] = corner
    return coef


# ======================================================================================================
# Part 1
def test_catalogue_decodes_as_built():
    """bits_ref's decode of every catalogue block is what its symbols say (landings), and the laid-out
    stream decodes, block by block, to the catalogue's coefficients."""
    for m in MAG.values():
        cat = catalogue(m)
        coef = decode(cat)
        for b, c in zip(cat, coef):
            want = np.zeros(64, np.int16)
            for pos, v in b.landings():
                if pos is not None and pos < 64:
                    want[ZZ[pos]] = np.int16(v)
            assert np.array_equal(c, want), b.name
        s = catalogue_stream(m)
        assert np.array_equal(bits_ref.unpack(s["bytes"], s["off"]), s["coef"])
    # what the issue's catalogue asks for, by position
    by = {b.name: b for b in catalogue(1)}
    for n, E in ENDS.items():
        assert [p for p, _ in by[f"n{n} +- at END-1, END"].landings()] == [E - 1, E]
        assert corner_mask(n)[ZZ[E - 1]] and not corner_mask(n)[ZZ[E]]
        assert by[f"n{n} bad code after END-1"].landings() == [(E - 1, 5), (None, 7)]
        assert all(p is None for p, _ in by[f"n{n} bad code before END-1"].landings()[-1:])
        assert by[f"n{n} last code cut"].landings()[-1][0] is None
        assert by[f"n{n} jump over END"].landings()[1][0] == E + 3
    assert by["first run 65535"].landings() == [(64, 10), (None, -7)]
    assert len(by["64 symbols run 0"].items) == 64 and by["empty"].data() == b""


@pytest.mark.parametrize("q,ad", list(MAG))
def test_every_catalogue_symbol_shows(q, ad):
    """Taking each symbol out in turn: the expected pixels of the block change at every scale where the
    symbol lands in the corner (a zero value: where something behind it does), R does not move where it
    is never read or lands at or beyond END with nothing behind it (a follower would move up into
    the corner), and everywhere a changed corner is a changed pixel."""
    Q = std_table(q)
    cat = catalogue(MAG[q, ad])
    checked = 0
    for vn in ([0, 2000000, 2 ** 31 - 1] if ad else [0]):
        for b in cat:
            base = decode([b])
            lands = b.landings()
            for i, (pos, v) in enumerate(lands):
                cut = decode([b.without(i)])
                for scale in SCALES:
                    n = 8 // scale
                    mask = corner_mask(n)
                    R0, R1 = (scaled_ref.unrounded(c, Q, scale, ad, [vn]) for c in (base, cut))
                    P0, P1 = (scaled_ref.blocks(c, Q, scale, ad, [vn]) for c in (base, cut))
                    changed = not np.array_equal(base[0][mask], cut[0][mask])
                    assert changed == (not np.array_equal(P0, P1)), (b.name, i, scale, vn)
                    later = any(p is not None and p < 64 and mask[ZZ[p]] and w for p, w in lands[i + 1:])
                    if pos is not None and pos < 64 and mask[ZZ[pos]] and (v or later):
                        assert changed, (b.name, i, scale)
                        checked += 1
                    follower = i < len(lands) - 1   # it would move up by run + 1, into the corner perhaps
                    if pos is None or (pos >= ENDS[n] and not follower):
                        assert np.array_equal(R0, R1), (b.name, i, scale)
    assert checked > 100


def test_catalogue_layout_from_offsets():
    """From the offsets and bytes alone: every catalogue block at lanes 0, 31, 32 and 63 of a run and alone in
    a run; a half beyond the stage with every catalogue block in its first, a middle and its last chunk."""
    s = catalogue_stream(1)
    cat = list(catalogue(1)) + [NEIGHBOUR]
    C = len(cat) - 1
    datas = [b.data() for b in cat]
    off = s["off"].astype(np.int64)
    raw = bytes(s["bytes"])
    index = {d: k for k, d in enumerate(datas)}
    assert len(index) == len(datas)                      # the blocks' bytes tell them apart
    which = np.array([index[raw[off[b]:off[b + 1]]] for b in range(len(off) - 1)])
    shape = [catalogue_shape()]
    assert len(which) == 2 * C * 130
    runs = window_ref.runs(shape, catalogue_windows()["whole"])
    assert sorted(set(runs[:, 1].tolist())) == [2, 64]
    seen = {lane: set() for lane in (0, 31, 32, 63)}
    for name in ("whole", "origin not block 0"):
        for s0, nb in window_ref.runs(shape, catalogue_windows()[name]):
            for lane in seen:
                if lane < nb:
                    seen[lane].add(int(which[s0 + lane]))
    assert all(v >= set(range(C)) for v in seen.values()), {k: len(v) for k, v in seen.items()}
    one = window_ref.runs(shape, catalogue_windows()["1 wide"])
    assert (one[:, 1] == 1).all() and {int(which[s0]) for s0, _ in one} == set(range(C))
    assert sorted(set(window_ref.runs(shape, catalogue_windows()["origin not block 0"])[:, 1].tolist())) == [63, 64]
    where = {"first": set(), "middle": set(), "last": set()}
    for r in range(C):
        h0 = (C + r) * 130                               # frame 1, row r: the first half of its first run
        assert off[h0 + 32] - off[h0] > STAGE
        chunks = chunks_of(off, h0, h0 + 32)
        assert len(chunks) >= 3
        for b in range(h0, h0 + 32):
            if which[b] == C:
                assert off[b + 1] - off[b] == 368
                continue
            k = [i for i, (cs, ce) in enumerate(chunks) if cs <= b < ce][0]
            where["first" if k == 0 else "last" if k == len(chunks) - 1 else "middle"].add(int(which[b]))
    assert all(v == set(range(C)) for v in where.values()), {k: len(v) for k, v in where.items()}


# Part 2
def scaled_share(name, q, ad, scale):
    coef = CF.family(name, q)
    R = scaled_ref.unrounded(coef, std_table(q), scale, ad, TF.plain_var_num(coef.shape[0]) if ad else None)
    return float(((R > 0.0) & (R < 255.0)).mean())


def test_family_streams_are_lossless():
    for q in (1, 50, 100):
        for name in CF.NAMES:
            assert np.array_equal(family_stream(name, q)[2], CF.family(name, q)), (name, q)


def test_family_shares():
    """The condition against a vacuous pass: for every (plan, scale) the best random family has at least 25 %
    of its reference values strictly inside (0, 255).  Prints the module docstring's table."""
    for q, ad in SCALED_PLANS:
        row = f"    ({q},{ad})".ljust(12)
        for scale in SCALES:
            sh = [scaled_share(name, q, ad, scale) for name in CF.RANDOM]
            row += f" s{scale} " + " ".join(f"{100 * v:5.1f}" for v in sh) + "   "
            assert max(sh) >= 0.25, (q, ad, scale, sh)
        print(row.rstrip())


@pytest.mark.parametrize("q,ad", TF.PLANS)
def test_window_families_keep_the_5_per_cent_rule(q, ad):
    shares = []
    for name in CF.RANDOM:
        want = TF.reference(name, q, ad)[2]
        shares.append(float(((want > 0.0) & (want < 255.0)).mean()))
    assert max(shares) >= 0.05, shares


# Part 3
@pytest.mark.parametrize("q,ad", TF.ADAPTIVE_PLANS)
def test_a_neighbours_var_num_changes_a_pixel(q, ad):
    """var_num read from the block before (the array shifted by one) changes expected pixels: of the
    full-size reference and of the scaled one at 1/2 and 1/4 (at 1/8 only the DC is left, which an
    adaptive plan does not scale: nothing can show there), inside the window the GPU module decodes."""
    Q = std_table(q)
    inside = window_ref.blocks([VAR_SHAPE], VAR_WINDOW)[0].ravel()
    assert VAR_SHAPE[2] // 8 >= 65 and all(lo > 0 for (lo, _) in VAR_WINDOW[0])
    for name in VAR_FAMILIES:
        coef, vn, want, tol = TF.reference(name, q, ad, True)
        assert coef.shape[0] == 4096 and set(vn[:len(TF.VAR_NUMS)].tolist()) == set(TF.VAR_NUMS)
        wrong = np.roll(vn, 1)
        other = oracle_ref(coef, Q, 1, wrong, quality=q, table=False)[0]
        clip = lambda a: np.rint(np.clip(a, 0.0, 255.0))  # noqa: E731
        moved = (np.abs(clip(want) - clip(other)) > 1.0).any(axis=1)   # more than the decoders' bound apart
        print(f"q{q} {name} full size: {int(moved[inside].sum())} of {len(inside)} blocks show a shifted var_num")
        assert moved[inside].sum() >= 32, (name, int(moved[inside].sum()))
        for scale in (2, 4):
            a = scaled_ref.blocks(coef, Q, scale, True, vn)
            b = scaled_ref.blocks(coef, Q, scale, True, wrong)
            moved = (a != b).reshape(len(a), -1).any(axis=1)
            print(f"q{q} {name} scale {scale}: {int(moved[inside].sum())} of {len(inside)} blocks show a shifted var_num")
            assert moved[inside].sum() >= 32, (name, scale)   # a half tile's worth, at the least
        assert np.array_equal(scaled_ref.blocks(coef, Q, 8, True, vn), scaled_ref.blocks(coef, Q, 8, True, wrong))


# Part 4
@pytest.mark.parametrize("ad", [0, 1])
@pytest.mark.parametrize("tname", TABLES)
def test_table_streams(tname, ad):
    """The streams decode to the oracle's coefficients, the best kind has more than 5 % of its reference
    inside (0, 255), and the corner blocks meet multipliers that are no integers where the table has them."""
    Q = TC.tables()[tname]
    shares = []
    for kind in TABLE_KINDS:
        s = table_stream(tname, ad, kind)
        assert s["coef"].shape[0] == sum(f * (h // 8) * (w // 8) for f, h, w in TABLE_SHAPES)
        want = s["want"][:s["npic"]]
        shares.append(float(((want > 0.0) & (want < 255.0)).mean()))
    assert max(shares) > 0.05, (tname, ad, shares)
    c = table_corner_blocks()
    if tname in ("scaled", "flat137", "ramp"):
        assert (np.mod(c[:, ZZ[:25]] / Q.ravel()[ZZ[:25]], 1.0) != 0.0).any()
    for scale in SCALES:
        px = scaled_ref.blocks(c, Q, scale, ad, TF.plain_var_num(16))
        assert len(np.unique(px)) > 2 or tname.startswith("edge") or tname in ("ramp", "checker"), (tname, scale)


# Part 5
def test_ties_are_exact_and_even():
    """The stated pixels are scaled_ref's, R is exactly the half (or the step next to it), and both parities
    of k and both clamps occur."""
    for q00, ad in [(1.0, 0), (1.0, 1), (2.0, 0), (2.0, 1)]:
        coef, pix = ties_n1(q00, ad)
        Q = np.array(TC.tables()["edge512"]) if q00 == 2.0 else np.ones((8, 8))
        assert Q[0, 0] == q00
        vn = np.full(len(coef), 2 ** 31 - 1) if ad else None
        R = scaled_ref.unrounded(coef, Q, 8, ad, vn)[:, 0, 0]
        assert np.array_equal(scaled_ref.blocks(coef, Q, 8, ad, vn)[:, 0, 0], pix), (q00, ad)
        ties = R[1::3]
        assert np.array_equal(ties[:257], np.r_[-0.5, np.arange(255) + 0.5, 255.5]) and ties[257] == 0.0
        assert (R[0::3] < ties).all() and (R[2::3] > ties).all()
        assert np.array_equal(pix[1::3][1:256], (np.arange(255) + 1) // 2 * 2)      # the even neighbour
        assert pix[1] == 0 and pix[3 * 256 + 1] == 255 and pix[0] == 0 and pix[3 * 257] == 0
    coef, pix = ties_n4()
    for ad in (0, 1):
        vn = np.full(len(coef), 2 ** 31 - 1) if ad else None     # nv = 1: the adaptive scale is 1.0 exactly
        R = scaled_ref.unrounded(coef, np.ones((8, 8)), 2, ad, vn)
        assert np.array_equal(scaled_ref.blocks(coef, np.ones((8, 8)), 2, ad, vn), pix), ad
        assert np.array_equal(R[1::3, 0, 0][:257], np.r_[-0.5, np.arange(255) + 0.5, 255.5])
        frac = R - np.floor(R)
        all_ties = (frac == 0.5).all(axis=(1, 2))
        some = (frac == 0.5).sum(axis=(1, 2))
        assert all_ties.sum() >= 100 and ((some > 0) & (some < 16)).sum() >= 100
    inside = (R > 0.0) & (R < 255.0) & (frac == 0.5)
    assert (pix[inside] % 2 == 0).all() and inside.sum() > 2000


def test_n2_has_no_exact_tie_and_the_golden_is_near():
    r = scaled_ref.D[2][0, 0]
    assert r * r != 0.5 and Fraction(r) ** 2 != Fraction(1, 2)
    coef = near_ties_n2()
    assert coef.shape == (256, 64)
    R = scaled_ref.unrounded(coef, np.ones((8, 8)), 4, False)
    d = R - np.floor(R) - 0.5
    dist, Rb = d[:, 0, 0], R[:, 0, 0]     # pixel (0, 0) is the one the search put next to the half
    assert ((Rb > 0.0) & (Rb < 255.0)).all()
    print(f"n = 2: |R - (k + 0.5)| between {np.abs(dist).min():.3e} and {np.abs(dist).max():.3e}, "
          f"{int((dist < 0).sum())} below and {int((dist > 0).sum())} above")
    assert (np.abs(dist) <= 2.0 ** -44).all() and (dist < 0).sum() == 128 and (dist > 0).sum() == 128
    # one ulp of R at these magnitudes is 2^-45 or more: these are the nearest values fp64 has
    px = scaled_ref.blocks(coef, np.ones((8, 8)), 4, False)[:, 0, 0]
    assert np.array_equal(px, np.where(dist < 0, np.floor(Rb), np.floor(Rb) + 1))
