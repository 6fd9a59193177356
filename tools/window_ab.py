"""Same-box A/B of the window decoder (Plan.decode_bits_window, decompress(region=, frames=))
against what a caller does without it: decode_bits of the whole stack, then a copy of the
slice.  The bench step's geometry (4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma
stacks, q50), 60 frames as tools/bits_ab.py (dctq_bits_pack admits 11 671 106 blocks).
  A   decode_bits of all 60 frames                      (the yardstick every ratio is against)
  As  ... plus the contiguous copy of the window's slice of every plane
  W   decode_bits_window:  (a) the whole planes          (the price of the run mapping)
                           (b) one frame of 60
                           (c) a 960 x 544 region of one frame
                           (d) a 256 x 256 region of one frame (32 luma blocks, 16 chroma
                               blocks wide: half- and quarter-filled waves)
  (e) decompress(region=(c)'s, frames=one) of the RGB container end to end, frame_unpack's
      offset scan and read-backs included, against decompress of everything plus the slice.
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events on one stream, medians; passes: uniform, smooth, uniform adaptive, smooth adaptive.
Reports; gates only on equality of every window with the slice.

    timeout 600 python tools/window_ab.py [--rounds 8] [--launches 3] [--frames 60]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dct_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--launches", type=int, default=3)
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--no-container", action="store_true", help="skip (e)")
args = ap.parse_args()

F = args.frames
H, W = 2160, 3840
shapes = [(F, H, W), (F, H // 2, W // 2), (F, H // 2, W // 2)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
ONE = (F // 2, F // 2 + 1)


def picture(frames, rows, cols):
    """A luma window and its 4:2:0 chroma windows."""
    half = lambda r: (r[0] // 2, r[1] // 2)  # noqa: E731
    return [(frames, rows, cols)] + [(frames, half(rows), half(cols))] * 2


CASES = {
    "(a) whole": picture((0, F), (0, H), (0, W)),
    "(b) one frame": picture(ONE, (0, H), (0, W)),
    "(c) 960x544": picture(ONE, (544, 1088), (960, 1920)),
    "(d) 256x256": picture(ONE, (512, 768), (1024, 1280)),
}
print(f"{F} frames 4:2:0 4K, q50: {nb} blocks; device {torch.cuda.get_device_name(0)}")


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


def cut(full, windows):
    return [p[f0:f1, y0:y1, x0:x1] for p, ((f0, f1), (y0, y1), (x0, x1)) in zip(full, windows)]


def one_pass(kind: str, adaptive: int) -> bool:
    label = f"{kind} a{adaptive}"
    plan = dct_amd.Plan(50, adaptive)
    planes = [dct_amd.synth(12345 + 50000 * k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, boff, by = plan.encode_bits_planes(planes)
    del planes
    torch.cuda.empty_cache()
    va = vns if adaptive else None
    full = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes]
    outs = {c: [torch.empty((f1 - f0, y1 - y0, x1 - x0), dtype=torch.uint8, device="cuda")
                for (f0, f1), (y0, y1), (x0, x1) in w] for c, w in CASES.items()}
    copies = {c: [torch.empty_like(o) for o in outs[c]] for c in CASES}

    def a_side():
        plan.decode_bits(by, boff, outs=full, var_nums=va)

    def a_sliced(c):
        def run():
            a_side()
            for dst, src in zip(copies[c], cut(full, CASES[c])):
                dst.copy_(src)
        return run

    def w_side(c):
        return lambda: plan.decode_bits_window(by, boff, shapes, CASES[c], outs=outs[c], var_nums=va)

    runs = {"A decode_bits": a_side}
    for c in CASES:
        runs[f"As {c}"] = a_sliced(c)
        runs[f"W  {c}"] = w_side(c)
    t = timed(runs)
    equal = all(torch.equal(g, w) for c in CASES for g, w in zip(outs[c], cut(full, CASES[c])))
    equal = equal and all(torch.equal(g, w) for c in CASES for g, w in zip(copies[c], outs[c]))
    a = t["A decode_bits"][0]
    for k, (m, lo, hi) in t.items():
        print(f"{label:12s} {k:22s} median {m:8.4f} ms  min {lo:8.4f}  max {hi:8.4f}")
    print(f"{label:12s} packed {by.numel() / nb:6.2f} B/block; " + "  ".join(
        f"{c}: W/A = {t['W  ' + c][0] / a:6.4f}, W/As = {t['W  ' + c][0] / t['As ' + c][0]:6.4f}" for c in CASES)
        + f"; every window equals its slice: {equal}")
    return equal


def container_pass(kind: str, adaptive: int) -> bool:
    """(e): the RGB container end to end."""
    label = f"{kind} a{adaptive}"
    # RGB content: three synthetic planes interleaved
    rgb = torch.stack([dct_amd.synth(777 + c, kind, W, H, F) for c in range(3)], dim=-1)
    buf = dct_amd.compress(rgb, 50, adaptive=bool(adaptive))
    del rgb
    torch.cuda.empty_cache()
    _, rows, cols = CASES["(c) 960x544"][0]
    region = (rows, cols)
    odd = ((545, 1087), (961, 1919))  # the same region, one pixel in: the view and the cropping path
    t = timed({"A decompress": lambda: dct_amd.decompress(buf),
               "As decompress + slice": lambda: dct_amd.decompress(buf)[ONE[0]:ONE[1], region[0][0]:region[0][1],
                                                                        region[1][0]:region[1][1]].contiguous(),
               "W  decompress(region, frames)": lambda: dct_amd.decompress(buf, region=region, frames=ONE),
               "W  decompress(unaligned region)": lambda: dct_amd.decompress(buf, region=odd, frames=ONE)})
    whole = dct_amd.decompress(buf)
    equal = torch.equal(dct_amd.decompress(buf, region=region, frames=ONE),
                        whole[ONE[0]:ONE[1], region[0][0]:region[0][1], region[1][0]:region[1][1]])
    equal = equal and torch.equal(dct_amd.decompress(buf, region=odd, frames=ONE),
                                  whole[ONE[0]:ONE[1], odd[0][0]:odd[0][1], odd[1][0]:odd[1][1]])
    a = t["A decompress"][0]
    for k, (m, lo, hi) in t.items():
        print(f"{label:12s} (e) {k:32s} median {m:8.4f} ms  min {lo:8.4f}  max {hi:8.4f}  /A = {m / a:6.4f}")
    print(f"{label:12s} (e) container {buf.numel() / 1e6:8.2f} MB; W/As = "
          f"{t['W  decompress(region, frames)'][0] / t['As decompress + slice'][0]:6.4f}; equal: {equal}")
    return equal


results = [one_pass("uniform", 0), one_pass("smooth", 0), one_pass("uniform", 1), one_pass("smooth", 1)]
if not args.no_container:
    results += [container_pass("uniform", 0), container_pass("smooth", 1)]
print("equality in every pass:", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
