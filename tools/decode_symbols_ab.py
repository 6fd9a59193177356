"""Same-box A/B of the two ways from run-length symbols to pixels, on the bench step's
geometry (64 4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma stacks, q50),
the symbols coming from encode_planes:
  A  rle_decode into a coefficient buffer of the whole step, then decode_planes (two
     launches): S + 4 + 128 + 128 + 64 B per block;
  B  one decode_symbols launch, no coefficient buffer: S + 4 + 64 B per block
(S = the block's symbols, measured as offsets[N] * W / N; + 4 B of var_num, adaptive).
Interleaved rounds, each sample `--launches` steps back to back after one untimed step,
device events, medians; four passes: uniform 2-byte, uniform 4-byte, smooth 2-byte,
uniform 2-byte adaptive.  Prints ms per step, blocks/s, the bytes per block each moves
and the fraction of 8 TB/s that is, checks B against A for equality over every pixel of
the step and exits non-zero unless B's median is below A's in every pass.

    python tools/decode_symbols_ab.py [--rounds 10] [--launches 3] [--frames 64]
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
args = ap.parse_args()

F = args.frames
shapes = [(F, 2160, 3840), (F, 1080, 1920), (F, 1080, 1920)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
print(f"{F} frames 4:2:0 4K, q50: {nb} blocks per step; device {torch.cuda.get_device_name(0)}")


def one_pass(kind: str, sb: int, adaptive: int) -> bool:
    label = f"{kind} {sb}-byte a{adaptive}"
    plan = dct_amd.Plan(50, adaptive)
    planes = [dct_amd.synth(12345 + 50000 * k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
    plan.forward_quant_planes(planes, var_nums=vns)
    coefs, off, sym = plan.encode_planes(planes, symbol_bytes=sb)
    del coefs, planes
    sym = sym.clone()  # the stream alone, not the worst-case allocation it was cut from
    torch.cuda.empty_cache()
    s_bytes = sym.numel() * sb / nb
    va = vns if adaptive else None
    cbuf = torch.empty((nb, 64), dtype=torch.int16, device="cuda")  # A's coefficient buffer: the whole step
    csplit, first = [], 0
    for n in nbs:
        csplit.append(cbuf[first:first + n])
        first += n
    outs_a = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes]
    outs_b = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes]

    def step_a():
        dct_amd.rle_decode(sym, off, out=cbuf)
        plan.decode_planes(csplit, outs=outs_a, var_nums=va)

    def step_b():
        plan.decode_symbols(sym, off, outs=outs_b, var_nums=va)

    runs = {"A rle_decode + decode_planes": step_a, "B decode_symbols": step_b}
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
    equal = all(torch.equal(a, b) for a, b in zip(outs_a, outs_b))
    bpb = {"A rle_decode + decode_planes": s_bytes + 4 + 128 + 128 + 64 + 4 * adaptive,
           "B decode_symbols": s_bytes + 4 + 64 + 4 * adaptive}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, m in med.items():
        print(f"{label:22s} {k:29s} median {m * 1e3:8.3f} ms/step  min {min(times[k]) * 1e3:8.3f}  "
              f"max {max(times[k]) * 1e3:8.3f}  {nb / m / 1e9:6.3f} Gblocks/s  {bpb[k]:6.1f} B/block  "
              f"{nb * bpb[k] / m / 8e12:6.3f} of 8 TB/s")
    ratio = med["B decode_symbols"] / med["A rle_decode + decode_planes"]
    ok = ratio < 1.0 and equal
    print(f"{label:22s} S = {s_bytes:6.2f} B/block  B/A = {ratio:5.3f}  every pixel equal: {equal}  "
          f"{'ok' if ok else 'FAIL'}")
    return ok


results = [one_pass("uniform", 2, 0), one_pass("uniform", 4, 0), one_pass("smooth", 2, 0), one_pass("uniform", 2, 1)]
print("gate (B's median below A's in every pass, every pixel equal):", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
