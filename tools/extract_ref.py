"""A window of a "bits v1" stream as a stream of its own, and containers cut and joined, in
plain numpy (CPU only): the yardstick of tests/test_extract_*.py.  Written from the definition
(include/dct_amd.h); nothing is decoded anywhere.

No block of bits v1 depends on another, so the stream of a block-aligned sub-picture is the
sub-sequence of the stored stream's blocks.  The destination numbers the window's blocks as the
window's own picture does: plane by plane, then frames, block rows, block columns -- the order of
window_ref.blocks(shapes, windows)[k].reshape(-1).

    window_stream(bytes, offsets, shapes, windows, var_nums=None) -> (bytes', offsets', var_nums')
        for destination block d that is stored block s:
            offsets'[d + 1] - offsets'[d] = offsets[s + 1] - offsets[s]   (exact, no 368 clamp)
            offsets'[0] = 0
            bytes'[offsets'[d] : offsets'[d + 1]] = bytes[offsets[s] : offsets[s + 1]]
            var_nums'[k][d_k] = var_nums[k][s_k]
        for any bytes and any non-decreasing offsets whose last entry is at most len(bytes)
    run_alignments(offsets, shapes, windows, src_base=0, dst_base=0)
        -> the set of (source start mod 4, destination start mod 4) over the window's runs
    frame_window(buf, region=None, frames=None) -> bytes   a container of part of a container
    frame_concat(bufs) -> bytes                             containers joined along the frame axis

    python tools/extract_ref.py     # a worked example
"""
from __future__ import annotations

import numpy as np

import frame_ref
import window_ref


def _u32(offsets) -> np.ndarray:
    return np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF


def window_stream(data, offsets, shapes, windows, var_nums=None):
    """(bytes' uint8, offsets' uint32 [N' + 1], var_nums' per plane int32 or None)."""
    raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8)
    off = _u32(offsets)
    per_plane = window_ref.blocks(shapes, windows)
    src = np.concatenate([b.reshape(-1) for b in per_plane])
    ln = off[src + 1] - off[src]
    if (ln < 0).any() or off[-1] > len(raw):
        raise ValueError("offsets must be non-decreasing and end inside bytes")
    new = np.concatenate([[0], np.cumsum(ln)])
    out = np.empty(int(new[-1]), np.uint8)
    for d, s in enumerate(src):
        out[new[d]:new[d + 1]] = raw[off[s]:off[s + 1]]
    var = None
    if var_nums is not None:
        first = 0
        var = []
        for (f, h, w), b, v in zip(shapes, per_plane, var_nums):
            var.append(np.asarray(v).reshape(-1).astype(np.int32)[b.reshape(-1) - first])
            first += f * (h // 8) * (w // 8)
    return out, new.astype(np.uint32), var


def run_alignments(offsets, shapes, windows, src_base=0, dst_base=0):
    """{(source start mod 4, destination start mod 4)} over the runs of the window; src_base and
    dst_base: the addresses of bytes[0] and bytes'[0] mod 4."""
    off = _u32(offsets)
    src = np.concatenate([b.reshape(-1) for b in window_ref.blocks(shapes, windows)])
    new = np.concatenate([[0], np.cumsum(off[src + 1] - off[src])])
    pairs, d = set(), 0
    for s0, nb in window_ref.runs(shapes, windows):
        pairs.add((int(off[s0] + src_base) % 4, int(new[d] + dst_base) % 4))
        d += int(nb)
    return pairs


def _windows(shapes, crops, colour, region, frames):
    """The region arithmetic: (windows, crops') for stored shapes and crops (or None), a region in
    pixels of the TRUE picture (one, or a list of one per plain plane; None: all of it) and
    frames (f0, f1) or None.  A region starts on a multiple of m (8; 16 for a 4:2:0 picture) and
    may end anywhere; the window is the region grown to multiples of m, and crops' = (window
    height - region height, window width - region width) on plane 0 of a picture, per plane
    for plain planes."""
    crops = crops or [(0, 0)] * len(shapes)
    nf = min(f for f, _, _ in shapes)
    f0, f1 = (0, nf) if frames is None else map(int, frames)
    if not 0 <= f0 < f1 <= nf:
        raise ValueError("frames is empty or leaves the stack")
    npic = 1 if colour else len(shapes)
    true = [(h - pb, w - pr) for (_, h, w), (pb, pr) in zip(shapes, crops)][:npic]
    if region is None:
        regions = [((0, h), (0, w)) for h, w in true]
    elif np.ndim(region[0][0]) == 0:
        regions = [region] * npic
    else:
        regions = list(region)
    if len(regions) != npic:
        raise ValueError("one region per plane")
    sub = 2 if colour and shapes[1][1:] != shapes[0][1:] else 1
    m = 8 * sub
    windows, new_crops = [], []
    for ((y0, y1), (x0, x1)), (th, tw) in zip(regions, true):
        if not (0 <= y0 < y1 <= th and 0 <= x0 < x1 <= tw):
            raise ValueError("region is empty or leaves the true picture")
        if y0 % m or x0 % m:
            raise ValueError(f"a region starts on a multiple of {m}: a stream cannot begin inside a block")
        yb, xb = -(-y1 // m) * m, -(-x1 // m) * m
        windows.append(((f0, f1), (y0, yb), (x0, xb)))
        new_crops.append((yb - y1, xb - x1))
    if colour:
        (_, (ya, yb), (xa, xb)) = windows[0]
        windows += [((f0, f1), (ya // sub, yb // sub), (xa // sub, xb // sub))] * 2
        new_crops += [(0, 0), (0, 0)]
    return windows, new_crops


def frame_window(buf, region=None, frames=None) -> bytes:
    """The container of a region and a frame range of the container buf: quality, adaptive and
    colour carried over, length_bytes chosen from the window's own blocks."""
    p = frame_ref.parse(buf)
    windows, crops = _windows(p["shapes"], p["crops"], p["colour"], region, frames)
    var = None
    if p["adaptive"]:
        nbs = [f * (h // 8) * (w // 8) for f, h, w in p["shapes"]]
        var = np.split(p["var_nums"], np.cumsum(nbs)[:-1])
    data, off, var = window_stream(p["payload"], p["offsets"], p["shapes"], windows, var)
    shapes = [(f1 - f0, y1 - y0, x1 - x0) for (f0, f1), (y0, y1), (x0, x1) in windows]
    return frame_ref.pack(data, off, shapes, p["quality"], p["adaptive"], var, p["colour"], crops=crops)


def frame_concat(bufs) -> bytes:
    """Containers that agree in quality, adaptive, colour, the planes' stored (H, W) and crops,
    joined along the frame axis: plane k of the result is plane k of each source in turn, in the
    lengths, var_num and payload sections alike.  length_bytes is 2 if any source's is 2."""
    ps = [frame_ref.parse(b) for b in bufs]
    if len(ps) < 2:
        raise ValueError("two or more containers")
    a = ps[0]
    for p in ps[1:]:
        if any(p[key] != a[key] for key in ("quality", "adaptive", "colour", "crops")):
            raise ValueError("the containers disagree in quality, adaptive, colour or crops")
        if [s[1:] for s in p["shapes"]] != [s[1:] for s in a["shapes"]]:
            raise ValueError("the containers disagree in their planes")
    chunks, lengths, var = [], [], []
    for k in range(len(a["shapes"])):
        for p in ps:
            nbs = [f * (h // 8) * (w // 8) for f, h, w in p["shapes"]]
            b0, b1 = sum(nbs[:k]), sum(nbs[:k + 1])
            off = _u32(p["offsets"])
            chunks.append(p["payload"][off[b0]:off[b1]])
            lengths.append(frame_ref.lengths_from_offsets(off[b0:b1 + 1]))
            if a["adaptive"]:
                var.append(p["var_nums"][b0:b1])
    shapes = [(sum(p["shapes"][k][0] for p in ps), h, w) for k, (_, h, w) in enumerate(a["shapes"])]
    off = np.concatenate([[0], np.cumsum(np.concatenate(lengths))])
    return frame_ref.pack(b"".join(chunks), off, shapes, a["quality"], a["adaptive"],
                          np.concatenate(var) if var else None, a["colour"],
                          length_bytes=max(p["length_bytes"] for p in ps), crops=a["crops"])


if __name__ == "__main__":
    import bits_ref
    shapes = [(2, 16, 24)]
    blocks = [[(b + 1, 0)] * (1 + b % 4) for b in range(12)]
    data, off = bits_ref.pack(blocks)
    windows = [((1, 2), (0, 16), (8, 24))]
    out, new, _ = window_stream(data, off, shapes, windows)
    print(f"stored {shapes}, {len(data)} bytes, offsets {off.tolist()}")
    print(f"window {windows}: blocks {window_ref.blocks(shapes, windows)[0].reshape(-1).tolist()}")
    print(f"-> {len(out)} bytes, offsets {new.tolist()}")
    print(f"run alignments (source, destination) mod 4: {sorted(run_alignments(off, shapes, windows))}")
