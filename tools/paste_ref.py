"""A window of a "bits v1" stream replaced by another stream's blocks, and containers pasted into
and tiled, in plain numpy (CPU only): the yardstick of tests/test_paste_*.py.  Written from the
definition (include/dct_amd.h); nothing is decoded anywhere.

No block of bits v1 depends on another, so the stream of an edited picture is the stored stream
with some blocks' bytes swapped for the patch's.  The result has the stored geometry `shapes`,
numbered plane by plane, then frames, block rows, block columns; the patch numbers its blocks as
the window's own picture does -- the order of window_ref.blocks(shapes, windows)[k].reshape(-1),
which is what extract_ref.window_stream produces.

    paste_stream(bytes, offsets, shapes, windows, pbytes, poffsets, var_nums=None, pvar_nums=None)
        -> (bytes', offsets', var_nums')
        for result block s:   source = patch block d  when s is block d of its plane's window
                                     = base block s   otherwise
            offsets'[s + 1] - offsets'[s] = the source block's offsets[i + 1] - offsets[i]
                                            (mod 2^32, exact: no 368 clamp),  offsets'[0] = 0
            bytes'[offsets'[s] : offsets'[s + 1]] = the source block's bytes
            var_nums'[k][s_k] = pvar_nums[k][d_k] or var_nums[k][s_k]
        for any bytes and any non-decreasing offsets that end inside their bytes
    frame_paste(buf, patch, at=(y, x), frame=0) -> bytes   a container with a container written in
    frame_blank(shapes, quality, adaptive=False, colour=False, crops=None) -> bytes
                                                            a container of empty blocks
    frame_tile(grid) -> bytes                               rows of containers joined spatially

The host rules of frame_paste (anything else is refused, ValueError):
    quality, adaptive, colour, the number of planes and (colour) the subsampling agree;
    at = (y, x) in pixels of the TRUE picture, multiples of m (8; 16 for a 4:2:0 picture); plain
        planes take one pair when every plane has one true size, or a list of one per plane;
    frame >= 0 and frame + the patch's frames <= buf's frames, plane by plane;
    on each axis either the patch has no crop and ends inside the true picture, or the patch's
        TRUE extent ends exactly on the true picture's edge -- its padded rows / columns are then
        what compress of the edited picture writes there.  A patch that ends anywhere else would
        write replicated edge pixels over real ones.
    The result keeps buf's geometry and crops; length_bytes is chosen from the result's blocks.
frame_blank: every block has length 0 (an empty block is valid bits v1 and decodes as zero
    coefficients) and, adaptive, var_num 0.
frame_tile: all containers agree in quality, adaptive, colour, planes, subsampling and frames; true
    heights are equal along a row and true widths along a column; only the last row and the
    last column may carry a crop.  It is frame_blank plus one frame_paste per tile.

    python tools/paste_ref.py     # a worked example
"""
from __future__ import annotations

import numpy as np

import frame_ref
import window_ref


def _u32(offsets) -> np.ndarray:
    return np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF


def _raw(data) -> np.ndarray:
    return np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8)


def paste_stream(data, offsets, shapes, windows, pdata, poffsets, var_nums=None, pvar_nums=None):
    """(bytes' uint8, offsets' uint32 [N + 1], var_nums' per plane int32 or None)."""
    raw, praw = _raw(data), _raw(pdata)
    off, poff = _u32(offsets), _u32(poffsets)
    per_plane = window_ref.blocks(shapes, windows)
    nbs = [f * (h // 8) * (w // 8) for f, h, w in shapes]
    if len(off) != sum(nbs) + 1 or len(poff) != sum(b.size for b in per_plane) + 1:
        raise ValueError("offsets: one entry per block, plus one")
    if (var_nums is None) != (pvar_nums is None):
        raise ValueError("var_nums and pvar_nums are both given or both None")
    # src[s] = -1: the base's block s; d >= 0: the patch's block d
    src = np.full(sum(nbs), -1, np.int64)
    src[np.concatenate([b.reshape(-1) for b in per_plane])] = np.arange(len(poff) - 1)
    s = np.arange(len(src))
    d = np.maximum(src, 0)
    ln = np.where(src >= 0, poff[d + 1] - poff[d], off[s + 1] - off[s])
    if (ln < 0).any() or off[-1] > len(raw) or poff[-1] > len(praw):
        raise ValueError("offsets must be non-decreasing and end inside bytes")
    new = np.concatenate([[0], np.cumsum(ln)])
    if new[-1] >= 1 << 32:
        raise ValueError("the result's payload must stay below 2^32 bytes")
    out = np.empty(int(new[-1]), np.uint8)
    for b in range(len(src)):
        out[new[b]:new[b + 1]] = praw[poff[src[b]]:poff[src[b] + 1]] if src[b] >= 0 else raw[off[b]:off[b + 1]]
    var = None
    if var_nums is not None:
        first, var = 0, []
        for nb, blocks, v, pv in zip(nbs, per_plane, var_nums, pvar_nums):
            merged = np.asarray(v).reshape(-1).astype(np.int32).copy()
            merged[blocks.reshape(-1) - first] = np.asarray(pv).reshape(-1).astype(np.int32)
            var.append(merged)
            first += nb
    return out, new.astype(np.uint32), var


def _split_var(p):
    if not p["adaptive"]:
        return None
    nbs = [f * (h // 8) * (w // 8) for f, h, w in p["shapes"]]
    return np.split(p["var_nums"], np.cumsum(nbs)[:-1])


def _sub(p) -> int:
    return 2 if p["colour"] and p["shapes"][1][1:] != p["shapes"][0][1:] else 1


def _agree(a, b, what):
    for key in ("quality", "adaptive", "colour"):
        if a[key] != b[key]:
            raise ValueError(f"{what}: the containers disagree in {key}")
    if len(a["shapes"]) != len(b["shapes"]) or _sub(a) != _sub(b):
        raise ValueError(f"{what}: the containers disagree in their planes or subsampling")


def paste_windows(shapes, crops, pshapes, pcrops, colour, at, frame):
    """The host rules of frame_paste -> the stored windows, one per plane."""
    crops = crops or [(0, 0)] * len(shapes)
    pcrops = pcrops or [(0, 0)] * len(pshapes)
    npic = 1 if colour else len(shapes)
    sub = 2 if colour and shapes[1][1:] != shapes[0][1:] else 1
    m = 8 * sub
    true = [(h - pb, w - pr) for (_, h, w), (pb, pr) in zip(shapes, crops)][:npic]
    if np.ndim(at[0]) == 0:
        if len(set(true)) != 1:
            raise ValueError("the planes differ in size: at must be a list of one (y, x) per plane")
        ats = [tuple(at)] * npic
    else:
        ats = [tuple(a) for a in at]
    if len(ats) != npic or colour and np.ndim(at[0]) != 0:
        raise ValueError("one (y, x) per plane, or one for a picture")
    frame = int(frame)
    windows = []
    for k, ((y, x), (th, tw)) in enumerate(zip(ats, true)):
        y, x = int(y), int(x)
        if y < 0 or x < 0 or y % m or x % m:
            raise ValueError(f"at must be non-negative multiples of {m}: a stream cannot begin inside a block")
        pf, ph, pw = pshapes[k]
        if frame < 0 or frame + pf > shapes[k][0]:
            raise ValueError("the patch's frames leave the stack")
        for a0, stored, pad, t in ((y, ph, pcrops[k][0], th), (x, pw, pcrops[k][1], tw)):
            inside = pad == 0 and a0 + stored <= t
            on_edge = a0 + stored - pad == t
            if not (inside or on_edge):
                raise ValueError("the patch must end inside the true picture without a crop, or with its true "
                                 "extent exactly on the true picture's edge")
        windows.append(((frame, frame + pf), (y, y + ph), (x, x + pw)))
    if colour:
        (_, (ya, yb), (xa, xb)) = windows[0]
        pf = pshapes[0][0]
        if any(s[0] != shapes[0][0] for s in shapes) or any(s[0] != pf for s in pshapes):
            raise ValueError("a picture's planes have one number of frames")
        windows += [((frame, frame + pf), (ya // sub, yb // sub), (xa // sub, xb // sub))] * 2
    return windows


def frame_paste(buf, patch, at=(0, 0), frame=0) -> bytes:
    """The container buf with the container patch written in at `at` of frame `frame` on."""
    b, p = frame_ref.parse(buf), frame_ref.parse(patch)
    _agree(b, p, "frame_paste")
    windows = paste_windows(b["shapes"], b["crops"], p["shapes"], p["crops"], b["colour"], at, frame)
    data, off, var = paste_stream(b["payload"], b["offsets"], b["shapes"], windows, p["payload"], p["offsets"],
                                  _split_var(b), _split_var(p))
    return frame_ref.pack(data, off, b["shapes"], b["quality"], b["adaptive"], var, b["colour"], crops=b["crops"])


def frame_blank(shapes, quality, adaptive=False, colour=False, crops=None) -> bytes:
    """A container of the stored shapes whose every block is empty."""
    shapes = [(1, *map(int, s)) if len(s) == 2 else tuple(map(int, s)) for s in shapes]
    n = sum(f * (h // 8) * (w // 8) for f, h, w in shapes)
    return frame_ref.pack(b"", np.zeros(n + 1, np.uint32), shapes, quality, adaptive,
                          np.zeros(n, np.int32) if adaptive else None, colour, crops=crops)


def tile_layout(parsed):
    """The rules of frame_tile for a grid (rows of parsed containers) -> (shapes, crops, ats):
    the joined container's stored shapes and crops and, per tile [r][c], its `at` (one (y, x) for
    a picture, a list of one per plane for plain planes)."""
    rows, cols = len(parsed), len(parsed[0]) if parsed else 0
    if rows < 1 or cols < 1 or any(len(row) != cols for row in parsed):
        raise ValueError("frame_tile: a grid of one or more equal rows")
    a = parsed[0][0]
    for row in parsed:
        for p in row:
            _agree(a, p, "frame_tile")
            if [s[0] for s in p["shapes"]] != [s[0] for s in a["shapes"]]:
                raise ValueError("frame_tile: the containers disagree in their frames")
    colour, n = a["colour"], len(a["shapes"])
    npic = 1 if colour else n
    sub = _sub(a)

    def true(p, k):
        (_, h, w), (pb, pr) = p["shapes"][k], (p["crops"] or [(0, 0)] * n)[k]
        return h - pb, w - pr, pb, pr

    shapes, crops, ys, xs = [], [], [], []
    for k in range(npic):
        for r, row in enumerate(parsed):
            if len({true(p, k)[0] for p in row}) != 1:
                raise ValueError("frame_tile: true heights must be equal along a row")
            if r < rows - 1 and any(true(p, k)[2] for p in row):
                raise ValueError("frame_tile: only the last row may carry a bottom crop")
        for c in range(cols):
            col = [row[c] for row in parsed]
            if len({true(p, k)[1] for p in col}) != 1:
                raise ValueError("frame_tile: true widths must be equal along a column")
            if c < cols - 1 and any(true(p, k)[3] for p in col):
                raise ValueError("frame_tile: only the last column may carry a right crop")
        hs = [true(row[0], k)[0] for row in parsed]
        ws = [true(p, k)[1] for p in parsed[0]]
        ys.append(np.concatenate([[0], np.cumsum(hs)]).tolist())
        xs.append(np.concatenate([[0], np.cumsum(ws)]).tolist())
        pb, pr = true(parsed[-1][0], k)[2], true(parsed[0][-1], k)[3]
        shapes.append((a["shapes"][k][0], ys[k][-1] + pb, xs[k][-1] + pr))
        crops.append((pb, pr))
    if colour:
        f, h, w = shapes[0]
        shapes += [(f, h // sub, w // sub)] * 2
        crops += [(0, 0), (0, 0)]
    ats = [[(ys[0][r], xs[0][c]) if colour else [(ys[k][r], xs[k][c]) for k in range(n)] for c in range(cols)]
           for r in range(rows)]
    return shapes, crops, ats


def frame_tile(grid) -> bytes:
    """grid: a list of rows of containers, joined spatially."""
    parsed = [[frame_ref.parse(b) for b in row] for row in grid]
    shapes, crops, ats = tile_layout(parsed)
    a = parsed[0][0]
    out = frame_blank(shapes, a["quality"], a["adaptive"], a["colour"], crops)
    for row, at_row in zip(grid, ats):
        for tile, at in zip(row, at_row):
            out = frame_paste(out, tile, at=at, frame=0)
    return out


if __name__ == "__main__":
    import bits_ref
    import extract_ref
    shapes = [(2, 16, 24)]
    blocks = [[(b + 1, 0)] * (1 + b % 4) for b in range(12)]
    data, off = bits_ref.pack(blocks)
    windows = [((1, 2), (0, 16), (8, 24))]
    pdata, poff = bits_ref.pack([[(-7, 1)] * 5] * 4)
    out, new, _ = paste_stream(data, off, shapes, windows, pdata, poff)
    print(f"stored {shapes}, {len(data)} bytes, offsets {off.tolist()}")
    print(f"window {windows}: blocks {window_ref.blocks(shapes, windows)[0].reshape(-1).tolist()} <- patch offsets {poff.tolist()}")
    print(f"-> {len(out)} bytes, offsets {new.tolist()}")
    back = extract_ref.window_stream(out, new, shapes, windows)
    print("the window of the result is the patch:", bytes(back[0]) == bytes(pdata) and back[1].tolist() == poff.tolist())
