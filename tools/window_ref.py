"""The window decoder's block mapping, stated in plain numpy (CPU only): which stored blocks a
window of a "bits v1" stream takes, in which units (runs), and in which order.

Stored plane k has shape (F, H, W), so F * (H / 8) * (W / 8) blocks in raster order (frames,
block rows, block columns); the planes' blocks are numbered one plane after the other, which
is how the stream's offsets are indexed.  A window of plane k is ((f0, f1), (y0, y1), (x0, x1)),
half-open, rows and columns in pixels and multiples of 8.

A RUN is up to 64 consecutive stored blocks that lie in one block row of one frame of one
plane and inside that plane's window: a window wb blocks wide has ceil(wb / 64) runs per block
row, run j of a row holding its blocks [64 j, min(64 j + 64, wb)).  Runs are numbered over the
window's rows, then its frames, then the planes; none straddles a row, a frame or a plane.

    runs(shapes, windows)    -> int64 [R, 2]: (s0, nb) of every run, in run order
    blocks(shapes, windows)  -> per plane, int64 [f1 - f0, (y1 - y0) / 8, (x1 - x0) / 8]: the
                                stored number of the block at each position of the window
    outside(shapes, windows) -> the stored blocks that are in no run (sorted)

    python tools/window_ref.py     # a worked example
"""
import numpy as np

RUN = 64


def _geometry(shapes, windows):
    if len(shapes) != len(windows):
        raise ValueError("one window per stored plane")
    first, out = 0, []
    for (f, h, w), ((f0, f1), (y0, y1), (x0, x1)) in zip(shapes, windows):
        if f < 1 or h < 8 or w < 8 or h % 8 or w % 8:
            raise ValueError(f"stored plane {(f, h, w)} is not whole blocks")
        if any(v % 8 for v in (y0, y1, x0, x1)):
            raise ValueError("window rows and columns must be multiples of 8")
        if not (0 <= f0 < f1 <= f and 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w):
            raise ValueError("window is empty or leaves the stored plane")
        out.append((first, h // 8, w // 8, (f0, f1), (y0 // 8, y1 // 8), (x0 // 8, x1 // 8)))
        first += f * (h // 8) * (w // 8)
    return out, first


def blocks(shapes, windows):
    """Per plane: the stored (concatenated) block number at each window position [frame, row, column]."""
    res = []
    for first, bh, bw, (f0, f1), (r0, r1), (c0, c1) in _geometry(shapes, windows)[0]:
        f = np.arange(f0, f1, dtype=np.int64)[:, None, None]
        r = np.arange(r0, r1, dtype=np.int64)[None, :, None]
        c = np.arange(c0, c1, dtype=np.int64)[None, None, :]
        res.append(first + (f * bh + r) * bw + c)
    return res


def runs(shapes, windows):
    """(s0, nb) of every run, in run order: int64 [R, 2]."""
    res = []
    for b in blocks(shapes, windows):
        wb = b.shape[2]
        for row in b.reshape(-1, wb):           # window rows, frame after frame
            for j in range(0, wb, RUN):
                res.append((int(row[j]), min(RUN, wb - j)))
    return np.array(res, dtype=np.int64).reshape(-1, 2)


def outside(shapes, windows):
    """The stored blocks that no run holds: what a window decode must not read."""
    total = _geometry(shapes, windows)[1]
    inside = np.zeros(total, dtype=bool)
    for s0, nb in runs(shapes, windows):
        inside[s0:s0 + nb] = True
    return np.flatnonzero(~inside)


if __name__ == "__main__":
    shapes = [(2, 32, 1056), (2, 16, 528), (2, 16, 528)]
    windows = [((1, 2), (8, 32), (8, 528)), ((1, 2), (0, 16), (0, 264)), ((0, 1), (8, 16), (520, 528))]
    r = runs(shapes, windows)
    print(f"stored {shapes}\nwindows {windows}\n{len(r)} runs (s0, nb):")
    print(r.tolist())
    print(f"{int(r[:, 1].sum())} blocks inside, {len(outside(shapes, windows))} outside")
