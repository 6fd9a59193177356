"""Same-box A/B of the two ways to a reconstruction, on the bench step's coefficients
(64 4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma stacks, q50):
  A  dctq_inverse over the three coefficient planes (three launches): unclamped fp32,
     block-major, 128 (+4 adaptive) B read + 256 B written per block;
  B  one dctq_decode_planes launch: clamped u8 pixels at their image position,
     128 (+4) B read + 64 B written per block.
Interleaved rounds, each sample `--launches` steps back to back after one untimed
step, device events; `--passes` non-adaptive passes plus one adaptive pass.  Prints ms
per step, blocks/s and the fraction of 8 TB/s each moves at its own bytes per block,
checks B against A's recon (|pix - clamp(recon)| <= 0.5 + 2e-4: both are within 1e-4 of
the reference) and exits non-zero unless B is faster than A in every pass.

    python tools/decode_ab.py [--rounds 10] [--passes 3] [--frames 64] [--kind uniform]
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
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--launches", type=int, default=3)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--kind", default="uniform")
args = ap.parse_args()

F = args.frames
shapes = [(F, 2160, 3840), (F, 1080, 1920), (F, 1080, 1920)]
planes = [dct_amd.synth(12345 + 50000 * k, args.kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
recs = [torch.empty((n, 64), dtype=torch.float32, device="cuda") for n in nbs]
outs = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes]
print(f"{F} frames 4:2:0 4K, kind {args.kind}: {nb} blocks per step; device {torch.cuda.get_device_name(0)}")


def one_pass(adaptive: int, label: str) -> bool:
    plan = dct_amd.Plan(50, adaptive)
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
    coefs = plan.forward_quant_planes(planes, var_nums=vns)
    va = vns if adaptive else [None] * 3

    def step_a():
        for c, v, r in zip(coefs, va, recs):
            plan.inverse(c, var_num=v, out=r)

    def step_b():
        plan.decode_planes(coefs, outs=outs, var_nums=vns if adaptive else None)

    runs = {"A inverse x3": step_a, "B decode_planes": step_b}
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
    # B against A's recon, every pixel of the step
    worst = 0.0
    for rec, out, s in zip(recs, outs, shapes):
        img = rec.clamp_(0, 255).reshape(s[0], s[1] // 8, s[2] // 8, 8, 8).permute(0, 1, 3, 2, 4).reshape(s)
        worst = max(worst, float((img - out.to(torch.float32)).abs().max()))
    bpb = {"A inverse x3": 128 + 256 + 4 * adaptive, "B decode_planes": 128 + 64 + 4 * adaptive}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, m in med.items():
        print(f"{label} {k:16s} median {m * 1e3:8.3f} ms/step  min {min(times[k]) * 1e3:8.3f}  max {max(times[k]) * 1e3:8.3f}  "
              f"{nb / m / 1e9:6.3f} Gblocks/s  {bpb[k]} B/block  {nb * bpb[k] / m / 8e12:6.3f} of 8 TB/s")
    ratio = med["B decode_planes"] / med["A inverse x3"]
    ok = ratio < 1.0 and worst <= 0.5 + 2e-4
    print(f"{label} B/A = {ratio:5.3f}  max |pix - clamp(A recon)| = {worst:.6f}  {'ok' if ok else 'FAIL'}")
    return ok


results = [one_pass(0, f"q50 a0 pass {i + 1}") for i in range(args.passes)]
results.append(one_pass(1, "q50 a1 pass 1"))
print("gate (B faster than A in every pass, outputs agree):", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
