"""The bit-packed coefficient stream "bits v1" in plain Python, written from its
specification (include/dct_amd.h): the yardstick of tests/test_bits_*.py.

  layout    block b owns bytes [offsets[b], offsets[b+1]) of one buffer; offsets has N + 1
            uint32 entries; every block starts on a byte boundary, its last byte padded
            with zero bits; bits are MSB first (bit i of a block is bit 7 - i % 8 of byte i / 8)
  ue(k)     x = k + 1 of bit length n: n - 1 zero bits, then x in n bits (Exp-Golomb, order 0)
  symbol    (value v, run r): ue(min(r, 64)), then ue(m), m = 2v - 1 for v > 0, else -2v
  block     its symbols in order, at most the first 64

    pack(blocks)            blocks: per block a list of (value, run) -> (bytes u8, offsets u32)
    unpack(bytes, offsets)  -> int16 [N, 64] coefficients in natural (row-major) order

Nothing here is fast, or meant to be: one Python loop per bit.
"""
from __future__ import annotations

import numpy as np

# zigzag position k -> natural (row-major) index of an 8x8 block
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
          12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
          58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
MAX_SYMBOLS = 64   # symbols of a block that are written, and that are read
MAX_PREFIX = 16    # zero bits in front of a code; a longer prefix is a bad code


def ue(k: int) -> str:
    """The code of k >= 0 as a string of '0' / '1'."""
    if k < 0:
        raise ValueError("ue(k) needs k >= 0")
    x = k + 1
    return "0" * (x.bit_length() - 1) + format(x, "b")


def value_code(v: int) -> int:
    """The signed value's index m: 1 -> 1, -1 -> 2, 2 -> 3, ...; 0 -> 0."""
    return 2 * v - 1 if v > 0 else -2 * v


def symbol_bits(v: int, r: int) -> str:
    return ue(min(int(r), 64)) + ue(value_code(int(v)))


def block_bits(symbols) -> str:
    return "".join(symbol_bits(v, r) for v, r in list(symbols)[:MAX_SYMBOLS])


def pack(blocks):
    """blocks: for every block a sequence of (value, run), value any int16, run >= 0.
    Returns (bytes uint8 [total], offsets uint32 [N + 1])."""
    out = bytearray()
    offsets = [0]
    for symbols in blocks:
        bits = block_bits(symbols)
        bits += "0" * (-len(bits) % 8)
        out += bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
        offsets.append(len(out))
    return np.frombuffer(bytes(out), np.uint8).copy(), np.array(offsets, np.uint32)


def _read_ue(bits: str, at: int):
    """(k, next position), or None for a bad code: a prefix of more than MAX_PREFIX
    zero bits, or a code that would use a bit past the block's last byte."""
    z = 0
    while True:
        if at + z >= len(bits):
            return None
        if bits[at + z] == "1":
            break
        z += 1
        if z > MAX_PREFIX:
            return None
    end = at + 2 * z + 1
    if end > len(bits):
        return None
    return int(bits[at + z:end], 2) - 1, end


def unpack_block(data: bytes) -> np.ndarray:
    """One block's bytes -> its 64 coefficients in natural order (int16).  Any bytes decode."""
    bits = "".join(format(b, "08b") for b in data)
    coef = np.zeros(64, np.int16)
    pos = at = 0
    for _ in range(MAX_SYMBOLS):
        if pos >= 64:
            break
        run = _read_ue(bits, at)
        if run is None:
            break
        val = _read_ue(bits, run[1])
        if val is None:
            break
        m, at = val
        v = (m + 1) >> 1 if m & 1 else -(m >> 1)
        v = ((v + 0x8000) & 0xFFFF) - 0x8000  # (int16_t)
        pos += run[0]
        if pos < 64:
            coef[ZIGZAG[pos]] = v
        pos += 1
    return coef


def unpack(data, offsets) -> np.ndarray:
    """bytes (uint8 array or bytes) + offsets (N + 1 entries) -> int16 [N, 64]."""
    raw = bytes(np.ascontiguousarray(data, np.uint8)) if not isinstance(data, (bytes, bytearray)) else bytes(data)
    off = [int(o) for o in np.asarray(offsets).astype(np.uint32)]
    out = np.zeros((len(off) - 1, 64), np.int16)
    for b in range(len(off) - 1):
        out[b] = unpack_block(raw[off[b]:off[b + 1]]) if off[b + 1] > off[b] else 0
    return out


def blocks_of(symbols, offsets):
    """A device symbol stream -> pack()'s input.  symbols: uint32 ((uint16)value | run << 16)
    or uint16 ((run & 63) << 10 | (value & 0x3FF), 0x0000 = (0, 64)); offsets: N + 1 entries."""
    s = np.asarray(symbols)
    off = np.asarray(offsets).view(np.uint32) if np.asarray(offsets).dtype.itemsize == 4 else np.asarray(offsets)
    if s.dtype.itemsize == 2:
        u = s.view(np.uint16).astype(np.int64)
        value = ((u & 0x3FF) ^ 0x200) - 0x200
        run = np.where(u == 0, 64, u >> 10)
    else:
        u = s.view(np.uint32).astype(np.int64)
        value = ((u & 0xFFFF) ^ 0x8000) - 0x8000
        run = u >> 16
    return [[(int(value[i]), int(run[i])) for i in range(int(off[b]), int(off[b + 1]))] for b in range(len(off) - 1)]
