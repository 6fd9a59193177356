"""The container "frame v1" in plain Python/numpy, written from its specification (DESIGN.md
3.15, include/dct_amd.h): the yardstick of tests/test_frame_*.py.  Little-endian.

  header    48 + 16 * nplanes bytes
               0  8 B  magic b"DCTQFRM1"
               8  u32  header_bytes = 48 + 16 * nplanes
              12  u8   quality 1..100      13  u8  adaptive 0 / 1
              14  u8   nplanes 1..4        15  u8  length_bytes 1 / 2
              16  u8   colour: 0 plain planes; 1 the three planes are Y, Cb, Cr of color_ref
                       (nplanes 3, chroma 4:4:4 or 4:2:0 of plane 0, equal nframes)
              17..23   reserved, 0
              24  u64  nblocks = sum of nframes * (width / 8) * (height / 8), 1..11 671 106
              32  u64  payload_bytes < 2^32
              40  u64  total_bytes, the container's length
              48 + 16 k  4 x u32  plane k: width, height, nframes, 0
  sections  each at the next multiple of 16, padding 0:
              lengths  nblocks * length_bytes bytes, entry b = offsets[b + 1] - offsets[b]
              var_num  4 * nblocks bytes of int32, only when adaptive
              payload  payload_bytes bytes of bits v1 (bits_ref.py); total_bytes is its end
  reading   a length above 368 reads as 368; offsets[0] = 0; the sum must be payload_bytes

Cropped pictures, "frame c1": magic b"DCTQFRC1", the same in every byte and rule but one: a plane
record's fourth word is pad_right | pad_bottom << 16, the columns and rows of that stored (edge-
padded) plane to drop after decoding.  Plain planes: each pad 0..7.  colour: plane 0 carries 0..15
(4:2:0) or 0..7 (4:4:4), planes 1 and 2 carry 0.  pad_right < width, pad_bottom < height.  At
least one word is non-zero: with no crop the container is frame v1, so a picture has one encoding.

    pack(payload, offsets, shapes, quality, adaptive=False, var_nums=None, colour=False,
         length_bytes=None, crops=None) -> bytes; crops: per plane (pad_bottom, pad_right), or None
    parse(buf) -> dict(quality, adaptive, colour, length_bytes, shapes, nblocks, lengths,
                       offsets, var_nums, payload, crops); crops is None for frame v1;
                       raises FrameError for everything a reader refuses
    lengths_from_offsets(offsets) / offsets_from_lengths(lengths)
    refusal_cases(buf) -> [(rule, bytes)]: a valid container broken once per rule of refusal
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"DCTQFRM1"
MAGIC_CROP = b"DCTQFRC1"
MAX_BLOCK_BYTES = 368       # bits v1: 64 symbols of 46 bits
MAX_BLOCKS = 11_671_106     # 368 * nblocks < 2^32


class FrameError(ValueError):
    pass


def align16(n: int) -> int:
    return (n + 15) // 16 * 16


def lengths_from_offsets(offsets) -> np.ndarray:
    """uint32 differences (mod 2^32) of N + 1 offsets, as int64 [N]."""
    o = np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF
    return (o[1:] - o[:-1]) & 0xFFFFFFFF


def offsets_from_lengths(lengths) -> np.ndarray:
    """uint32 [N + 1]: exclusive prefix sums of min(length, 368); the last entry is the total."""
    ln = np.minimum(np.asarray(lengths).astype(np.int64), MAX_BLOCK_BYTES)
    return np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)


def _shapes3(shapes):
    out = [(1, *map(int, s)) if len(s) == 2 else tuple(map(int, s)) for s in shapes]
    if any(len(s) != 3 for s in out):
        raise FrameError("shapes entries are (F, H, W) or (H, W)")
    return out


def _check_geometry(shapes, colour):
    """The plane records' rules; returns nblocks."""
    if not 1 <= len(shapes) <= 4:
        raise FrameError("nplanes must be 1..4")
    n = 0
    for f, h, w in shapes:
        if w < 8 or h < 8 or w % 8 or h % 8 or f < 1:
            raise FrameError(f"plane {w} x {h} x {f}: width and height are multiples of 8, nframes >= 1")
        n += f * (h // 8) * (w // 8)
    if not 1 <= n <= MAX_BLOCKS:
        raise FrameError(f"nblocks {n} outside 1..{MAX_BLOCKS}")
    if colour:
        if len(shapes) != 3:
            raise FrameError("colour needs three planes")
        (f, h, w), cb, cr = shapes
        if cb != cr or cb[0] != f or ((cb[1], cb[2]) != (h, w) and (2 * cb[1], 2 * cb[2]) != (h, w)):
            raise FrameError("colour: chroma must be 4:4:4 or 4:2:0 of plane 0")
    return n


def _check_crops(crops, shapes, colour):
    """The rules of the fourth words of frame c1; crops: per plane (pad_bottom, pad_right)."""
    if len(crops) != len(shapes):
        raise FrameError("crops: one (pad_bottom, pad_right) per plane")
    for k, ((pb, pr), (_, h, w)) in enumerate(zip(crops, shapes)):
        most = 7
        if colour:
            most = 0 if k else (15 if shapes[1][1:] != shapes[0][1:] else 7)
        if not (0 <= pb <= most and 0 <= pr <= most):
            raise FrameError(f"plane {k}: pads ({pb}, {pr}) outside 0..{most}")
        if pr >= w or pb >= h:
            raise FrameError(f"plane {k}: a pad is not smaller than the plane")
    if not any(pb or pr for pb, pr in crops):
        raise FrameError("frame c1 with no crop: that picture is frame v1")


def pack(payload, offsets, shapes, quality, adaptive=False, var_nums=None, colour=False, length_bytes=None,
         crops=None) -> bytes:
    """payload: the bits v1 bytes; offsets: its N + 1 byte offsets; shapes: per plane (F, H, W) or
    (H, W); var_nums: int32 [N] (or per-plane pieces), needed when adaptive.  length_bytes None:
    1 when every block is at most 255 B, else 2.  crops: per plane (pad_bottom, pad_right); None or
    all zero gives frame v1, anything else frame c1."""
    shapes = _shapes3(shapes)
    if crops is not None:
        crops = [tuple(map(int, c)) for c in crops]
        if len(crops) != len(shapes):
            raise FrameError("crops: one (pad_bottom, pad_right) per plane")
        if not any(pb or pr for pb, pr in crops):
            crops = None
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise FrameError("quality must be 1..100")
    nblocks = _check_geometry(shapes, colour)
    if crops is not None:
        _check_crops(crops, shapes, colour)
    payload = bytes(np.ascontiguousarray(payload, np.uint8)) if not isinstance(payload, (bytes, bytearray)) else bytes(payload)
    off = np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF
    if off.shape != (nblocks + 1,) or off[0] != 0 or off[-1] != len(payload):
        raise FrameError("offsets: N + 1 entries from 0 to len(payload)")
    ln = lengths_from_offsets(off)
    if length_bytes is None:
        length_bytes = 1 if ln.max() <= 255 else 2
    if length_bytes not in (1, 2) or ln.max() >= 1 << (8 * length_bytes):
        raise FrameError("a block's length does not fit length_bytes")
    if len(payload) >= 1 << 32:
        raise FrameError("payload_bytes must stay below 2^32")
    sections = [ln.astype("<u1" if length_bytes == 1 else "<u2").tobytes()]
    if adaptive:
        if var_nums is None:
            raise FrameError("an adaptive container needs var_nums")
        vn = np.concatenate([np.asarray(v).reshape(-1) for v in var_nums]) if isinstance(var_nums, (list, tuple)) \
            else np.asarray(var_nums).reshape(-1)
        if vn.shape != (nblocks,):
            raise FrameError("var_nums: one int32 per block")
        sections.append(vn.astype("<i4").tobytes())
    sections.append(payload)
    header_bytes = 48 + 16 * len(shapes)
    total = header_bytes
    for s in sections:
        total = align16(total) + len(s)
    out = bytearray(MAGIC if crops is None else MAGIC_CROP)
    out += struct.pack("<IBBBBB7xQQQ", header_bytes, quality, int(bool(adaptive)), len(shapes), length_bytes,
                       int(bool(colour)), nblocks, len(payload), total)
    for (f, h, w), (pb, pr) in zip(shapes, crops or [(0, 0)] * len(shapes)):
        out += struct.pack("<IIII", w, h, f, pr | pb << 16)
    assert len(out) == header_bytes
    for s in sections:
        out += bytes(align16(len(out)) - len(out)) + s
    assert len(out) == total
    return bytes(out)


def parse(buf) -> dict:
    """Everything in the container, checked; FrameError for every rule of the "Refusals" list."""
    buf = bytes(np.ascontiguousarray(buf, np.uint8)) if not isinstance(buf, (bytes, bytearray)) else bytes(buf)
    if len(buf) < 48:
        raise FrameError("shorter than the fixed header")
    if buf[:8] not in (MAGIC, MAGIC_CROP):
        raise FrameError("bad magic")
    cropped = buf[:8] == MAGIC_CROP
    header_bytes, quality, adaptive, nplanes, length_bytes, colour = struct.unpack_from("<IBBBBB", buf, 8)
    nblocks, payload_bytes, total = struct.unpack_from("<QQQ", buf, 24)
    if not 1 <= quality <= 100 or adaptive > 1 or not 1 <= nplanes <= 4 or length_bytes not in (1, 2) or colour > 1:
        raise FrameError("a field is out of range")
    if any(buf[17:24]):
        raise FrameError("reserved bytes are not 0")
    if header_bytes != 48 + 16 * nplanes:
        raise FrameError("header_bytes does not match nplanes")
    if len(buf) < header_bytes:
        raise FrameError("shorter than header_bytes")
    shapes, words = [], []
    for k in range(nplanes):
        w, h, f, word = struct.unpack_from("<IIII", buf, 48 + 16 * k)
        if word and not cropped:
            raise FrameError("a plane record's fourth word is not 0")
        shapes.append((f, h, w))
        words.append(word)
    if _check_geometry(shapes, colour) != nblocks:
        raise FrameError("nblocks does not match the plane records")
    crops = None
    if cropped:
        crops = [(word >> 16, word & 0xFFFF) for word in words]
        _check_crops(crops, shapes, colour)
    if payload_bytes >= 1 << 32:
        raise FrameError("payload_bytes must stay below 2^32")
    if len(buf) < total:
        raise FrameError("shorter than total_bytes")
    at = align16(header_bytes)
    sizes = [nblocks * length_bytes] + ([4 * nblocks] if adaptive else []) + [payload_bytes]
    starts = []
    for s in sizes:
        starts.append(at)
        if at + s > total:
            raise FrameError("a section ends past total_bytes")
        at = align16(at + s)
    if starts[-1] + payload_bytes != total:
        raise FrameError("total_bytes is not the end of the payload")
    lengths = np.frombuffer(buf, "<u1" if length_bytes == 1 else "<u2", nblocks, starts[0])
    offsets = offsets_from_lengths(lengths)
    if int(offsets[-1]) != payload_bytes:
        raise FrameError("the lengths do not sum to payload_bytes")
    var_nums = np.frombuffer(buf, "<i4", nblocks, starts[1]).astype(np.int32) if adaptive else None
    return {"quality": quality, "adaptive": bool(adaptive), "colour": bool(colour), "length_bytes": length_bytes,
            "shapes": shapes, "nblocks": nblocks, "lengths": lengths.copy(), "offsets": offsets, "var_nums": var_nums,
            "payload": buf[starts[-1]:starts[-1] + payload_bytes], "crops": crops}


def refusal_cases(buf):
    """[(rule, bytes)]: one mutation of the valid container `buf` per rule a reader refuses by.  A
    frame c1 buffer gets the rules of its fourth words instead of "fourth word set"."""
    buf = bytes(buf)
    header_bytes, = struct.unpack_from("<I", buf, 8)
    nblocks, payload_bytes, total = struct.unpack_from("<QQQ", buf, 24)

    def put(fmt, at, *values):
        b = bytearray(buf)
        struct.pack_into(fmt, b, at, *values)
        return bytes(b)

    first_length = align16(header_bytes)
    cases = [
        ("shorter than 48 bytes", buf[:47]),
        ("shorter than header_bytes", buf[:header_bytes - 1]),
        ("shorter than total_bytes", buf[:total - 1]),
        ("bad magic", b"DCTQFRM2" + buf[8:]),
        ("quality 0", put("<B", 12, 0)),
        ("quality 101", put("<B", 12, 101)),
        ("adaptive 2", put("<B", 13, 2)),
        ("nplanes 0", put("<B", 14, 0)),
        ("nplanes 5", put("<B", 14, 5)),
        ("length_bytes 3", put("<B", 15, 3)),
        ("colour 2", put("<B", 16, 2)),
        ("reserved byte set", put("<B", 20, 1)),
        ("width 12", put("<I", 48, 12)),
        ("nframes 0", put("<I", 56, 0)),
        ("plane record's fourth word set", put("<I", 60, 1)),
        ("payload_bytes 2^32", put("<Q", 32, 1 << 32)),
        ("header_bytes inconsistent", put("<I", 8, header_bytes + 16)),
        ("nblocks inconsistent", put("<Q", 24, nblocks + 1)),
        ("a section ends past total_bytes", put("<Q", 40, total - 1)),
        ("lengths sum differs", put("<B", first_length, buf[first_length] + 1 & 0xFF)),
    ]
    if buf[:8] != MAGIC_CROP:
        return cases
    nplanes, colour = buf[14], buf[16]
    (w0, h0), (w1, h1) = (struct.unpack_from("<II", buf, 48 + 16 * min(k, nplanes - 1)) for k in (0, 1))
    most = (15 if (w1, h1) != (w0, h0) else 7) if colour else 7
    word0, = struct.unpack_from("<I", buf, 60)
    zeroed = bytearray(buf)
    for k in range(nplanes):
        struct.pack_into("<I", zeroed, 60 + 16 * k, 0)
    cases = [c for c in cases if c[0] != "plane record's fourth word set"]
    cases[3] = ("bad magic", b"DCTQFRC2" + buf[8:])
    cases += [
        ("pad_right above the most", put("<I", 60, (word0 & 0xFFFF0000) | (most + 1))),
        ("pad_bottom above the most", put("<I", 60, (word0 & 0xFFFF) | (most + 1) << 16)),
        ("pad_right with high bits", put("<I", 60, word0 | 0x8000)),
        ("pad_bottom with high bits", put("<I", 60, word0 | 0x80000000)),
        ("no crop at all under the crop magic", bytes(zeroed)),
        ("the fourth words under the frame v1 magic", MAGIC + buf[8:]),
    ]
    if colour:
        cases += [("a chroma plane with a pad", put("<I", 60 + 16, 1)),
                  ("a chroma plane with a bottom pad", put("<I", 60 + 32, 1 << 16))]
    return cases
