"""Same-box A/B of the two ways to the per-block squared error of the decoded picture, on the
bench step's geometry (64 4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma stacks,
uniform input):
  A  the composition: forward_quant_planes (64 B read + 128 B written per block; + 4 B of
     var_num, adaptive plans) + decode_planes (128 B + 64 B) + a reduction by torch over both pictures (128 B
     read at best; eager torch runs it as a cast, a subtraction, a square and a block sum per
     plane, in fp32, where every partial sum is an exact integer below 2^24), through
     preallocated coefficient and picture buffers;
  A0 (for information, not gated) A's two launches alone, without the reduction;
  B  one dctq_distortion_planes launch: 64 B read + 4 B written per block, no buffer.
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events, medians; one pass each for q50 non-adaptive (fp32 inverse), q75 non-adaptive (fp64
inverse) and q50 adaptive.  Checks B against A over every block of the step (equal, not close)
and exits non-zero unless B is faster than A in every pass.

    python tools/distortion_ab.py [--rounds 10] [--launches 3] [--frames 64] [--kind uniform]
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
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--launches", type=int, default=3)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--kind", default="uniform")
args = ap.parse_args()

F = args.frames
shapes = [(F, 2160, 3840), (F, 1080, 1920), (F, 1080, 1920)]
planes = [dct_amd.synth(12345 + 50000 * k, args.kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
coefs = [torch.empty((n, 64), dtype=torch.int16, device="cuda") for n in nbs]
vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
pics = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes]
sse_b = torch.empty(nb, dtype=torch.int32, device="cuda")
print(f"{F} frames 4:2:0 4K, kind {args.kind}: {nb} blocks per step; device {torch.cuda.get_device_name(0)}")


def one_pass(quality: int, adaptive: int, label: str) -> bool:
    plan = dct_amd.Plan(quality, adaptive)
    result = {}

    def step_a0():
        plan.forward_quant_planes(planes, outs=coefs, var_nums=vns if adaptive else None)
        plan.decode_planes(coefs, outs=pics, var_nums=vns if adaptive else None)

    def step_a():
        step_a0()
        parts = []
        for px, pic, s in zip(planes, pics, shapes):
            d = px.to(torch.float32) - pic
            parts.append(d.mul_(d).reshape(s[0], s[1] // 8, 8, s[2] // 8, 8).sum((2, 4)).reshape(-1))
        result["a"] = parts

    def step_b():
        plan.distortion_planes(planes, out=sse_b)

    runs = {"A compose+reduce": step_a, "A0 compose only": step_a0, "B distortion_planes": step_b}
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
                times[k].append(e0.elapsed_time(e1) / args.launches * 1e-3)
    a = torch.cat(result["a"]).to(torch.int32)
    differ = int((a != sse_b).sum())
    total = int(sse_b.sum(dtype=torch.int64))
    bpb = {"A compose+reduce": 64 + 128 + 128 + 64 + 8 * adaptive + 128 + 4, "A0 compose only": 64 + 128 + 128 + 64 + 8 * adaptive,
           "B distortion_planes": 64 + 4}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, m in med.items():
        print(f"{label} {k:20s} median {m * 1e3:8.3f} ms/step  min {min(times[k]) * 1e3:8.3f}  max {max(times[k]) * 1e3:8.3f}  "
              f"{nb / m / 1e9:6.3f} Gblocks/s  {bpb[k]} B/block at best  {nb * bpb[k] / m / 8e12:6.3f} of 8 TB/s")
    ratio = med["B distortion_planes"] / med["A compose+reduce"]
    ok = ratio < 1.0 and differ == 0
    print(f"{label} B/A = {ratio:5.3f}  B/A0 = {med['B distortion_planes'] / med['A0 compose only']:5.3f}  blocks that differ: {differ} of {nb}  psnr_u8 {dct_amd.psnr_u8(total, 64 * nb):.3f} dB  "
          f"{'ok' if ok else 'FAIL'}")
    return ok


results = [one_pass(50, 0, "q50 a0"), one_pass(75, 0, "q75 a0"), one_pass(50, 1, "q50 a1")]
print("gate (B faster than A in every pass, every block equal):", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
