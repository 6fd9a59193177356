"""Same-box A/B of the bit-packed stream "bits v1" against the symbol stream it packs, on
the bench step's geometry (4K 4:2:0 frames: one 3840x2160 luma and two 1920x1080 chroma
stacks, q50).  60 frames by default, not the step's 64: dctq_bits_pack admits
368 * N < 2^32, N <= 11 671 106 blocks, and 64 frames are 12 441 600.
  decoders  S  decode_symbols on the 2-byte symbols          (the parent's fused decoder)
            B  decode_bits on the packed bytes               (one launch)
            C  bits_decode + decode_planes                   (two launches, a coefficient buffer)
  packers   E  dctq_rle_emit: coefficients -> 4-byte symbols (offsets given)
            P  dctq_bits_pack: 2-byte symbols -> bytes       (count, scan, fix-up, emit)
Interleaved rounds, each sample `--launches` steps back to back after one untimed step,
device events, medians; three passes: uniform, smooth, uniform adaptive.  Prints ms per step,
bytes per block and the ratios; checks B and C against S over every pixel and the packed
stream's round trip over every coefficient.  Reports; gates only on equality.

    python tools/bits_ab.py [--rounds 8] [--launches 3] [--frames 60]
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
args = ap.parse_args()

F = args.frames
shapes = [(F, 2160, 3840), (F, 1080, 1920), (F, 1080, 1920)]
nbs = [s[0] * (s[1] // 8) * (s[2] // 8) for s in shapes]
nb = sum(nbs)
L = dct_amd.lib()
print(f"{F} frames 4:2:0 4K, q50: {nb} blocks per step; device {torch.cuda.get_device_name(0)}")


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
    vns = [torch.empty(n, dtype=torch.int32, device="cuda") for n in nbs]
    plan.forward_quant_planes(planes, var_nums=vns)
    coefs, off, sym = plan.encode_planes(planes, symbol_bytes=2)
    coef = torch.cat(coefs)
    del coefs, planes
    sym = sym.clone()
    torch.cuda.empty_cache()
    by, boff = dct_amd.bits_pack(sym, off)
    s_bytes, p_bytes = sym.numel() * 2 / nb, by.numel() / nb
    va = vns if adaptive else None
    cbuf = torch.empty((nb, 64), dtype=torch.int16, device="cuda")
    csplit, first = [], 0
    for n in nbs:
        csplit.append(cbuf[first:first + n])
        first += n
    outs = {k: [torch.empty(s, dtype=torch.uint8, device="cuda") for s in shapes] for k in "SBC"}

    def step_c():
        dct_amd.bits_decode(by, boff, out=cbuf)
        plan.decode_planes(csplit, outs=outs["C"], var_nums=va)

    dec = timed({"S decode_symbols": lambda: plan.decode_symbols(sym, off, outs=outs["S"], var_nums=va),
                 "B decode_bits": lambda: plan.decode_bits(by, boff, outs=outs["B"], var_nums=va),
                 "C bits_decode + decode_planes": step_c})
    equal = all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(outs["S"], outs["B"], outs["C"]))
    equal = equal and torch.equal(cbuf, coef)
    del outs, cbuf, csplit
    torch.cuda.empty_cache()

    # the packers, on preallocated buffers (no read-back inside the timed region)
    off4, sym4 = dct_amd.rle_encode(coef)
    sym4 = sym4.clone()
    torch.cuda.empty_cache()
    out = torch.empty(by.numel() + 4, dtype=torch.uint8, device="cuda")
    boff2 = torch.empty_like(boff)
    ws = torch.empty(int(L.dctq_bits_workspace_bytes(nb)) // 4 + 1, dtype=torch.int32, device="cuda")
    s = dct_amd._stream_ptr()

    def step_e():
        dct_amd._check(L.dctq_rle_emit(ptr(coef), nb, ptr(off4), ptr(sym4), s))

    def step_p():
        dct_amd._check(L.dctq_bits_pack(ptr(sym), 2, ptr(off), nb, ptr(boff2), ptr(out), by.numel(), ptr(ws), s))

    pk = timed({"E rle_emit (4-byte symbols)": step_e, "P bits_pack (from 2-byte)": step_p})
    equal = equal and torch.equal(out[:by.numel()], by) and torch.equal(boff2, boff)
    for k, (m, lo, hi) in {**dec, **pk}.items():
        print(f"{label:12s} {k:30s} median {m:8.3f} ms/step  min {lo:8.3f}  max {hi:8.3f}  "
              f"{nb / m / 1e6:7.3f} Gblocks/s")
    b, sy, c = dec["B decode_bits"][0], dec["S decode_symbols"][0], dec["C bits_decode + decode_planes"][0]
    print(f"{label:12s} packed {p_bytes:6.2f} B/block, 2-byte symbols {s_bytes:6.2f} B/block ({p_bytes / s_bytes:5.3f}); "
          f"B/S = {b / sy:5.3f}  B/C = {b / c:5.3f}  P/E = {pk['P bits_pack (from 2-byte)'][0] / pk['E rle_emit (4-byte symbols)'][0]:5.3f}  "
          f"every pixel, coefficient and byte equal: {equal}")
    return equal


results = [one_pass("uniform", 0), one_pass("smooth", 0), one_pass("uniform", 1)]
print("equality in every pass:", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
