"""Same-box A/B of writing a tile into a container without decoding (frame_paste) against today's
only other route, decompress -> write the tile into the pixels -> compress.  The bench step's
geometry (4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma stacks, q50) as three plain
planes, 60 frames as tools/extract_ab.py.  Per patch -- (a) a 256 x 256 tile of one frame, (b) a
960 x 544 tile of one frame, (c) one whole frame:
  X   frame_paste, end to end: frame_unpack's offset scans of both containers, the result's offsets
      and copy, frame_pack's lengths, every read-back
  P   its copy launch alone (dctq_bits_paste_copy on offsets computed before)
  A   decompress, write the decompressed patch into the planes, compress: the bit walk, the IDCT
      and the whole encoder; every block it did not touch is a second generation, so its container
      differs from X's, which is recorded
  C   a copy_ of as many bytes as the result's payload: the byte-movement yardstick for P
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events on one stream, medians; passes: uniform, smooth, uniform adaptive.  Reports times and the
ratios X/A and P/C; no ratio is a pass condition.  Exits non-zero only if a container differs from
its definition: frame_paste of the base's own window is the base, frame_paste of compress of new
pixels is compress of the edited frame range (checked through frame_window, which keeps the check
to the frames that changed), and its window reads back as the patch.

    timeout 900 python tools/paste_ab.py [--rounds 5] [--launches 2] [--frames 60]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dct_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=2)
ap.add_argument("--frames", type=int, default=60)
args = ap.parse_args()

F = args.frames
H, W = 2160, 3840
shapes = [(F, H, W), (F, H // 2, W // 2), (F, H // 2, W // 2)]
nb = sum(s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes)
AT_FRAME = F // 2


def picture(rows, cols):
    """A luma region and its 4:2:0 chroma regions, one per plain plane."""
    half = lambda r: (r[0] // 2, r[1] // 2)  # noqa: E731
    return [(rows, cols)] + [(half(rows), half(cols))] * 2


CASES = {   # name: the region of frame AT_FRAME that is replaced, per plane
    "(a) 256x256": picture((512, 768), (1024, 1280)),
    "(b) 960x544": picture((544, 1088), (960, 1920)),
    "(c) one frame": picture((0, H), (0, W)),
}
print(f"{F} frames 4:2:0 4K as plain planes, q50: {nb} blocks; device {torch.cuda.get_device_name(0)}")


def timed(runs):
    times = {k: [] for k in runs}
    for r in range(args.rounds + 1):
        for k, fn in runs.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) / args.launches)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def copy_alone(buf, patch, at):
    """The paste's copy launch on its own: everything else done once, before."""
    d, p = dct_amd.frame_unpack(buf), dct_amd.frame_unpack(patch)
    hb, hp = (dct_amd._frame_open(x, None)[1] for x in (buf, patch))
    windows = dct_amd._paste_windows(hb, hp, at, AT_FRAME)
    wins, wshapes, _ = dct_amd._stored_windows(d["shapes"], windows)
    n = len(wshapes)
    exts = (dct_amd._Extent * n)(*[dct_amd._Extent(w, h, f) for f, h, w in wshapes])
    packed, ooff, _ = dct_amd.bits_paste(d["bytes"], d["offsets"], d["shapes"], windows, p["bytes"], p["offsets"],
                                         d["var_nums"], p["var_nums"])
    out = torch.empty_like(packed)
    L = dct_amd.lib()

    def run():
        dct_amd._check(L.dctq_bits_paste_copy(d["bytes"].data_ptr(), d["offsets"].data_ptr(), p["bytes"].data_ptr(),
                                              p["offsets"].data_ptr(), wins, exts, n, ooff.data_ptr(), out.data_ptr(),
                                              C.c_size_t(out.numel()), dct_amd._stream_ptr()))
    run()
    assert torch.equal(out, packed)
    return run, packed.numel()


def one_pass(kind: str, adaptive: int) -> bool:
    label = f"{kind} a{adaptive}"
    planes = [dct_amd.synth(12345 + 50000 * k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    buf = dct_amd.compress(planes, 50, adaptive=bool(adaptive))
    ok = True
    runs, payload, patches, ats, news = {}, {}, {}, {}, {}
    for c, region in CASES.items():
        # new pixels for the region: another seed's picture, cut to the region
        new = [dct_amd.synth(777 + 50000 * k, kind, s[2], s[1], 1)[:, r[0][0]:r[0][1], r[1][0]:r[1][1]].contiguous()
               for k, (s, r) in enumerate(zip(shapes, region))]
        patch = dct_amd.compress(new, 50, adaptive=bool(adaptive))
        at = [(r[0][0], r[1][0]) for r in region]
        news[c], patches[c], ats[c] = new, patch, at
        g, payload[c] = copy_alone(buf, patch, at)
        src = dct_amd.frame_unpack(buf)["bytes"]
        src = src[:payload[c]] if src.numel() >= payload[c] else torch.empty(payload[c], dtype=torch.uint8, device="cuda")
        dst = torch.empty(payload[c], dtype=torch.uint8, device="cuda")

        def decode_edit_encode(region=region, patch=patch):
            px = [p.contiguous() for p in dct_amd.decompress(buf)]
            for p, q, r in zip(px, dct_amd.decompress(patch), region):
                p[AT_FRAME:AT_FRAME + 1, r[0][0]:r[0][1], r[1][0]:r[1][1]] = q
            return dct_amd.compress(px, 50, adaptive=bool(adaptive))

        runs[f"X {c}"] = lambda patch=patch, at=at: dct_amd.frame_paste(buf, patch, at=at, frame=AT_FRAME)
        runs[f"P {c}"] = g
        runs[f"A {c}"] = decode_edit_encode
        runs[f"C {c}"] = lambda src=src, dst=dst: dst.copy_(src)
    t = timed(runs)
    for k, (m, lo, hi) in t.items():
        print(f"{label:12s} {k:18s} median {m:9.4f} ms  min {lo:9.4f}  max {hi:9.4f}")
    one = (AT_FRAME, AT_FRAME + 1)
    for c, region in CASES.items():
        x = runs[f"X {c}"]()
        a = runs[f"A {c}"]()
        second = x.shape != a.shape or not torch.equal(x, a)
        # the definitions, on the frame that changed and on its neighbours
        edited = [p[AT_FRAME:AT_FRAME + 1].clone() for p in planes]
        for p, q, r in zip(edited, news[c], region):
            p[:, r[0][0]:r[0][1], r[1][0]:r[1][1]] = q
        ok = ok and torch.equal(dct_amd.frame_window(x, frames=one), dct_amd.compress(edited, 50, adaptive=bool(adaptive)))
        ok = ok and torch.equal(dct_amd.frame_window(x, region=region, frames=one), patches[c])
        ok = ok and torch.equal(dct_amd.frame_window(x, frames=(0, AT_FRAME)), dct_amd.frame_window(buf, frames=(0, AT_FRAME)))
        back = dct_amd.frame_paste(buf, dct_amd.frame_window(buf, region=region, frames=one), at=ats[c], frame=AT_FRAME)
        ok = ok and torch.equal(back, buf)
        print(f"{label:12s} {c:14s} payload {payload[c] / 1e6:9.3f} MB  X/A = {t['X ' + c][0] / t['A ' + c][0]:7.4f}  "
              f"P/C = {t['P ' + c][0] / t['C ' + c][0]:7.4f}  P {payload[c] / t['P ' + c][0] / 1e6:8.1f} GB/s  "
              f"C {payload[c] / t['C ' + c][0] / 1e6:8.1f} GB/s  A's container differs from X's: {second}")
    print(f"{label:12s} packed {dct_amd.frame_unpack(buf)['bytes'].numel() / nb:6.2f} B/block; "
          f"containers equal their definitions: {ok}")
    return ok


results = [one_pass("uniform", 0), one_pass("smooth", 0), one_pass("uniform", 1)]
print("every container equals its definition:", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
