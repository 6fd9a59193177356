"""The container "frame v1" on the bench step's geometry (4K 4:2:0 frames: one 3840x2160 luma and
two 1920x1080 chroma stacks, q50; 60 frames, the most dctq_bits_pack admits of the step's 64).
  size    the container per block against what a caller held before: the payload, the uint32
          offsets (4 (N + 1) B) and, for an adaptive plan, the int32 var_num (4 N B)
  time    O  dctq_block_offsets: lengths -> offsets        (tile scan, scan of the totals, fix-up)
          L  dctq_block_lengths: offsets -> lengths        (memset of the maximum, one kernel)
          B  decode_bits on the packed bytes               (the decoder the offsets feed)
          P  dctq_bits_pack: 2-byte symbols -> bytes       (the packer the lengths follow)
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events, medians; three passes: uniform, smooth, uniform adaptive.  Gates only on equality: the
offsets rebuilt from the lengths equal the originals, and decompress(compress(x)) equals the
uncontained decode over every byte.

    python tools/frame_ab.py [--rounds 8] [--launches 3] [--frames 60]
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
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--launches", type=int, default=3)
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--width", type=int, default=3840)
ap.add_argument("--height", type=int, default=2160)
args = ap.parse_args()

F = args.frames
shapes = [(F, args.height, args.width), (F, args.height // 2, args.width // 2), (F, args.height // 2, args.width // 2)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
L = dct_amd.lib()
print(f"{F} frames 4:2:0 {args.width}x{args.height}, q50: {nb} blocks per step; device {torch.cuda.get_device_name(0)}")


def ptr(t):
    return C.c_void_p(t.data_ptr())


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


def one_pass(kind: str, adaptive: int) -> bool:
    label = f"{kind} a{adaptive}"
    plan = dct_amd.Plan(50, adaptive)
    planes = [dct_amd.synth(12345 + 50000 * k, kind, s[2], s[1], s[0]) for k, s in enumerate(shapes)]

    # the uncontained stream: bytes, offsets and (adaptive) var_num held side by side
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
    plan.forward_quant_planes(planes, var_nums=vns)
    _, off, sym = plan.encode_planes(planes, symbol_bytes=2)
    sym = sym.clone()
    torch.cuda.empty_cache()
    by, boff = dct_amd.bits_pack(sym, off)
    va = vns if adaptive else None
    want = plan.decode_bits(by, boff, shapes=shapes, var_nums=va)

    # the container, and back
    box = dct_amd.compress(planes, 50, bool(adaptive))
    got = dct_amd.decompress(box)
    equal = all(torch.equal(a, b) for a, b in zip(got, want))
    d = dct_amd.frame_unpack(box)
    equal = equal and torch.equal(d["offsets"], boff) and torch.equal(d["bytes"], by)
    lb = d["length_bytes"]
    del got, planes, d
    torch.cuda.empty_cache()
    loose = by.numel() + 4 * (nb + 1) + (4 * nb if adaptive else 0)
    print(f"{label:12s} container {box.numel() / nb:7.3f} B/block, payload + offsets{' + var_num' if adaptive else ''} "
          f"{loose / nb:7.3f} B/block ({box.numel() / loose:5.3f}); payload {by.numel() / nb:6.3f} B/block, "
          f"length_bytes {lb}")

    # the two conversions beside the decoder and the packer, on preallocated buffers
    lengths = torch.empty(nb, dtype=torch.uint8 if lb == 1 else torch.int16, device="cuda")
    mx = torch.empty(1, dtype=torch.int32, device="cuda")
    off2 = torch.empty_like(boff)
    ws = torch.empty(int(L.dctq_block_offsets_workspace_bytes(nb)) // 4 + 1, dtype=torch.int32, device="cuda")
    wsp = torch.empty(int(L.dctq_bits_workspace_bytes(nb)) // 4 + 1, dtype=torch.int32, device="cuda")
    out = torch.empty(by.numel() + 4, dtype=torch.uint8, device="cuda")
    boff2 = torch.empty_like(boff)
    s = dct_amd._stream_ptr()

    def step_l():
        dct_amd._check(L.dctq_block_lengths(ptr(boff), nb, lb, ptr(lengths), ptr(mx), s))

    def step_o():
        dct_amd._check(L.dctq_block_offsets(ptr(lengths), lb, nb, ptr(off2), ptr(ws), s))

    def step_p():
        dct_amd._check(L.dctq_bits_pack(ptr(sym), 2, ptr(off), nb, ptr(boff2), ptr(out), by.numel(), ptr(wsp), s))

    step_l()
    res = timed({"O block_offsets": step_o, "L block_lengths": step_l,
                 "B decode_bits": lambda: plan.decode_bits(by, boff, outs=want, var_nums=va),
                 "P bits_pack (from 2-byte)": step_p})
    longest = int(mx.item()) & 0xFFFFFFFF
    equal = equal and torch.equal(off2, boff) and torch.equal(boff2, boff) and torch.equal(out[:by.numel()], by)
    equal = equal and longest == int((boff[1:].long() - boff[:-1].long()).max().item())
    for k, (m, lo, hi) in res.items():
        print(f"{label:12s} {k:30s} median {m:8.3f} ms/step  min {lo:8.3f}  max {hi:8.3f}  "
              f"{nb / m / 1e6:7.3f} Gblocks/s")
    o, l_, b, p = (res[k][0] for k in res)
    print(f"{label:12s} longest block {longest} B; O/B = {o / b:5.3f}  L/P = {l_ / p:5.3f}  "
          f"(O + L) / (B + P) = {(o + l_) / (b + p):5.3f}  offsets, bytes and every pixel equal: {equal}")
    return equal


results = [one_pass("uniform", 0), one_pass("smooth", 0), one_pass("uniform", 1)]
print("equality in every pass:", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
