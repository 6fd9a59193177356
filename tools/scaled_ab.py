"""Same-box A/B of the reduced-size decoder (Plan.decode_bits_scaled) against what a caller does
without it.  The bench step's geometry (4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080
chroma stacks, q50), 60 frames as tools/window_ab.py.
  A   decode_bits of all 60 frames at full size          (the parent's code)
  B   A, then torch avg_pool2d of every plane to 1 / s   (what a caller does today)
  W   decode_bits_scaled of the whole stack, s = 2, 4, 8
  W1  decode_bits_scaled of one frame of 60 at s = 8     (against A: nothing cheaper exists)
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events on one stream, medians; passes: uniform, smooth, uniform adaptive.
Exits non-zero unless every sampled frame equals tools/scaled_ref.py byte for byte, and unless
every scaled launch is faster than A in every pass: it reads no more bytes, walks no more
symbols and writes at most 1/4 of the pixels, so slower would be a defect.  No ratio is fixed.

    timeout 900 python tools/scaled_ab.py [--rounds 8] [--launches 3] [--frames 60]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dct_amd  # noqa: E402
import scaled_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--launches", type=int, default=3)
ap.add_argument("--frames", type=int, default=60)
args = ap.parse_args()

F = args.frames
H, W = 2160, 3840
shapes = [(F, H, W), (F, H // 2, W // 2), (F, H // 2, W // 2)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
ONE = F // 2
SAMPLED = sorted({0, ONE, F - 1})
SCALES = (2, 4, 8)
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


def frame_ref(coef, vns, Q, adaptive, s, frame):
    """scaled_ref of one frame of every plane: uint8 [H / s, W / s] each."""
    res, first = [], 0
    for k, (f, h, w) in enumerate(shapes):
        per = (h // 8) * (w // 8)
        lo = first + frame * per
        c = coef[lo:lo + per].cpu().numpy()
        vn = None if not adaptive else vns[k][frame * per:(frame + 1) * per].cpu().numpy()
        res.append(scaled_ref.planes(c, [(1, h, w)], Q, s, adaptive, None if vn is None else [vn])[0][0])
        first += f * per
    return res


def one_pass(kind: str, adaptive: int):
    label = f"{kind} a{adaptive}"
    plan = dct_amd.Plan(50, adaptive)
    Q = dct_amd.debug_tables(50, adaptive)[3].reshape(8, 8)
    planes = [dct_amd.synth(12345 + 50000 * k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, boff, by = plan.encode_bits_planes(planes)
    del planes
    torch.cuda.empty_cache()
    va = vns if adaptive else None
    full = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes]
    outs = {s: [torch.empty((f, h // s, w // s), dtype=torch.uint8, device="cuda") for f, h, w in shapes] for s in SCALES}
    one = [torch.empty((1, h // 8, w // 8), dtype=torch.uint8, device="cuda") for _, h, w in shapes]
    one_win = [((ONE, ONE + 1), (0, h), (0, w)) for _, h, w in shapes]

    def a_side():
        plan.decode_bits(by, boff, outs=full, var_nums=va)

    def b_side(s):
        def run():
            a_side()
            for p in full:   # a frame at a time: the fp32 copy of a whole stack would not fit beside it
                for f in range(0, F, 10):
                    torch.nn.functional.avg_pool2d(p[f:f + 10].unsqueeze(1).float(), s).round_().to(torch.uint8)
        return run

    runs = {"A decode_bits": a_side}
    for s in SCALES:
        runs[f"B A + avg_pool2d /{s}"] = b_side(s)
        runs[f"W decode_bits_scaled /{s}"] = (lambda s=s: plan.decode_bits_scaled(by, boff, shapes, s, outs=outs[s], var_nums=va))
    runs["W1 one frame /8"] = lambda: plan.decode_bits_scaled(by, boff, shapes, 8, one_win, outs=one, var_nums=va)
    t = timed(runs)

    coef = dct_amd.bits_decode(by, boff)
    equal = True
    for s in SCALES:
        for f in SAMPLED:
            equal = equal and all(np.array_equal(o[f].cpu().numpy(), r)
                                  for o, r in zip(outs[s], frame_ref(coef, vns, Q, adaptive, s, f)))
    equal = equal and all(np.array_equal(o[0].cpu().numpy(), r) for o, r in zip(one, frame_ref(coef, vns, Q, adaptive, 8, ONE)))
    a = t["A decode_bits"][0]
    for k, (m, lo, hi) in t.items():
        print(f"{label:12s} {k:28s} median {m:8.4f} ms  min {lo:8.4f}  max {hi:8.4f}")
    faster = all(t[k][0] < a for k in t if k.startswith("W"))
    print(f"{label:12s} packed {by.numel() / nb:6.2f} B/block; " + "  ".join(
        f"/{s}: W/A = {t[f'W decode_bits_scaled /{s}'][0] / a:6.4f}, W/B = "
        f"{t[f'W decode_bits_scaled /{s}'][0] / t[f'B A + avg_pool2d /{s}'][0]:6.4f}" for s in SCALES)
        + f"; one frame /8: W1/A = {t['W1 one frame /8'][0] / a:6.4f}"
        + f"; sampled frames {SAMPLED} equal scaled_ref: {equal}; every scaled launch faster than A: {faster}")
    return equal, faster


results = [one_pass("uniform", 0), one_pass("smooth", 0), one_pass("uniform", 1)]
ok = all(e and f for e, f in results)
print("equality and W < A in every pass:", "PASS" if ok else "FAIL")
sys.exit(0 if ok else 1)
