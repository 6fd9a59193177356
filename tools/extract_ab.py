"""Same-box A/B of cutting a window out of a container as a container (frame_window) against
today's only other route, decompress(region=, frames=) followed by compress.  The bench step's
geometry (4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma stacks, q50) as three plain
planes, 60 frames as tools/window_ab.py.  Per window -- (a) the whole stack, (b) one frame of 60,
(c) a 960 x 544 region of one frame, (d) a 256 x 256 region of one frame:
  X   frame_window, end to end: frame_unpack's offset scan, the window's offsets and gather,
      frame_pack's lengths, every read-back
  G   its gather launch alone (dctq_bits_window_gather on offsets computed before)
  A   decompress(region=, frames=) then compress: the bit walk, the IDCT and the whole encoder; its
      output is a second generation and differs from X's, which is recorded
  C   a copy_ of as many bytes as the window's payload: the byte-movement yardstick for G
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events on one stream, medians; passes: uniform, smooth, uniform adaptive, smooth adaptive.
Reports times and the ratios X/A and G/C; no ratio is a pass condition.  Exits non-zero only if
a container differs from its definition: frame_window of the sampled frame is compress of that
frame, the windows decompress as decompress(region=, frames=) does, and split + concat is the
identity.

    timeout 900 python tools/extract_ab.py [--rounds 5] [--launches 2] [--frames 60]
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
ONE = (F // 2, F // 2 + 1)


def picture(rows, cols):
    """A luma region and its 4:2:0 chroma regions, one per plain plane."""
    half = lambda r: (r[0] // 2, r[1] // 2)  # noqa: E731
    return [(rows, cols)] + [(half(rows), half(cols))] * 2


CASES = {   # name: (region, frames)
    "(a) whole": (None, None),
    "(b) one frame": (None, ONE),
    "(c) 960x544": (picture((544, 1088), (960, 1920)), ONE),
    "(d) 256x256": (picture((512, 768), (1024, 1280)), ONE),
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


def gather_alone(d, region, frames):
    """The window's gather launch on its own: everything else done once, before."""
    windows, wshapes, _ = dct_amd._window_crops(d["shapes"], d["crops"], d["colour"], region, frames)
    wins, _, _ = dct_amd._stored_windows(d["shapes"], windows)
    n = len(wshapes)
    exts = (dct_amd._Extent * n)(*[dct_amd._Extent(w, h, f) for f, h, w in wshapes])
    packed, woff, _ = dct_amd.bits_window(d["bytes"], d["offsets"], d["shapes"], windows, d["var_nums"])
    out = torch.empty_like(packed)
    L = dct_amd.lib()

    def run():
        dct_amd._check(L.dctq_bits_window_gather(d["bytes"].data_ptr(), d["offsets"].data_ptr(), wins, exts, n,
                                                 woff.data_ptr(), out.data_ptr(), C.c_size_t(out.numel()),
                                                 dct_amd._stream_ptr()))
    run()
    assert torch.equal(out, packed)
    return run, packed.numel()


def one_pass(kind: str, adaptive: int) -> bool:
    label = f"{kind} a{adaptive}"
    planes = [dct_amd.synth(12345 + 50000 * k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    buf = dct_amd.compress(planes, 50, adaptive=bool(adaptive))
    d = dct_amd.frame_unpack(buf)
    ok = True
    runs, payload = {}, {}
    for c, (region, frames) in CASES.items():
        g, payload[c] = gather_alone(d, region, frames)
        src, dst = d["bytes"][:payload[c]], torch.empty(payload[c], dtype=torch.uint8, device="cuda")
        runs[f"X {c}"] = lambda region=region, frames=frames: dct_amd.frame_window(buf, region=region, frames=frames)
        runs[f"G {c}"] = g
        runs[f"A {c}"] = lambda region=region, frames=frames: dct_amd.compress(
            [p.contiguous() for p in dct_amd.decompress(buf, region=region, frames=frames)], 50, adaptive=bool(adaptive))
        runs[f"C {c}"] = lambda src=src, dst=dst: dst.copy_(src)
    t = timed(runs)
    for k, (m, lo, hi) in t.items():
        print(f"{label:12s} {k:18s} median {m:9.4f} ms  min {lo:9.4f}  max {hi:9.4f}")
    second = []
    for c, (region, frames) in CASES.items():
        x = dct_amd.frame_window(buf, region=region, frames=frames)
        a = runs[f"A {c}"]()
        second.append(x.shape != a.shape or not torch.equal(x, a))
        if c != "(a) whole":   # the equalities of the tests, on the sampled frame
            f0, f1 = frames
            crop = [p[f0:f1] if region is None else p[f0:f1, r[0][0]:r[0][1], r[1][0]:r[1][1]].contiguous()
                    for p, r in zip(planes, region or [None] * 3)]
            ok = ok and torch.equal(x, dct_amd.compress(crop, 50, adaptive=bool(adaptive)))
            ok = ok and all(torch.equal(g, w) for g, w in zip(dct_amd.decompress(x),
                                                              dct_amd.decompress(buf, region=region, frames=frames)))
        else:
            ok = ok and torch.equal(x, buf)
        print(f"{label:12s} {c:14s} payload {payload[c] / 1e6:9.3f} MB  X/A = {t['X ' + c][0] / t['A ' + c][0]:7.4f}  "
              f"G/C = {t['G ' + c][0] / t['C ' + c][0]:7.4f}  G {payload[c] / t['G ' + c][0] / 1e6:8.1f} GB/s  "
              f"C {payload[c] / t['C ' + c][0] / 1e6:8.1f} GB/s  A's container differs from X's: {second[-1]}")
    halves = [dct_amd.frame_window(buf, frames=(0, ONE[0])), dct_amd.frame_window(buf, frames=(ONE[0], F))]
    ok = ok and torch.equal(dct_amd.frame_concat(halves), buf)
    print(f"{label:12s} packed {d['bytes'].numel() / nb:6.2f} B/block; containers equal their definitions: {ok}")
    return ok


results = [one_pass("uniform", 0), one_pass("smooth", 0), one_pass("uniform", 1), one_pass("smooth", 1)]
print("every container equals its definition:", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
