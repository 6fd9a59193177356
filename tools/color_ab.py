"""Same-box A/B of the colour stage on the bench step's geometry (4K frames, 4:2:0), each
direction and for interleaved RGB and planar pictures:
  A  the library launch: rgb_to_ycbcr (3 B read + 1.5 B written per pixel) / ycbcr_to_rgb (the
     reverse), into preallocated outputs;
  B  an eager torch restatement of the same integer arithmetic (int32 tensors, >> as an
     arithmetic shift, strided 2x2 sums, repeat_interleave on the way back), which must give
     equal bytes;
  C  one copy_ of a u8 buffer of 2.25 B per pixel: the same 4.5 B per pixel read + written,
     as the movement yardstick.
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events, medians.  Reports the times, A/B, and A's bytes per second as a fraction of C's and of
8 TB/s.  Exits non-zero unless every byte of A equals B, and A equals tools/color_ref.py on
frame 0; speed does not decide the exit status.

    python tools/color_ab.py [--rounds 10] [--launches 3] [--frames 16]
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
import color_ref  # noqa: E402
import dct_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--launches", type=int, default=3)
ap.add_argument("--frames", type=int, default=16)  # beside B's int32 temporaries: ~0.4 GB per frame
args = ap.parse_args()

F, H, W = args.frames, 2160, 3840
npix = F * H * W
i32, u8 = torch.int32, torch.uint8
print(f"{F} frames 4K 4:2:0: {npix} pixels per step, {4.5 * npix / 1e6:.1f} MB moved; "
      f"device {torch.cuda.get_device_name(0)}")


def eager_forward(rgb):
    c = rgb.to(i32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (8388608 + 32767)) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (8388608 + 32767)) >> 16

    def sub(p):
        return ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2).to(u8)
    return y.to(u8), sub(cb), sub(cr)


def eager_inverse(y, cb, cr, out):
    yy = y.to(i32)
    cb, cr = ((p.to(i32) - 128).repeat_interleave(2, 1).repeat_interleave(2, 2) for p in (cb, cr))
    out[..., 0] = (yy + ((91881 * cr + 32768) >> 16)).clamp_(0, 255)
    out[..., 1] = (yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)).clamp_(0, 255)
    out[..., 2] = (yy + ((116130 * cb + 32768) >> 16)).clamp_(0, 255)
    return out


def picture(planar):
    """Three synthetic planes of different seeds as the channels of an RGB stack."""
    chans = [dct_amd.synth(777 + 50000 * c, "uniform", W, H, F) for c in range(3)]
    if planar:
        return torch.stack(chans, 1).permute(0, 2, 3, 1)
    return torch.stack(chans, -1).contiguous()


def empty_like_picture(planar):
    if planar:
        return torch.empty((F, 3, H, W), dtype=u8, device="cuda").permute(0, 2, 3, 1)
    return torch.empty((F, H, W, 3), dtype=u8, device="cuda")


def one_pass(planar: bool) -> bool:
    label = "planar" if planar else "rgb   "
    rgb = picture(planar)
    outs = [torch.empty(s, dtype=u8, device="cuda") for s in ((F, H, W), (F, H // 2, W // 2), (F, H // 2, W // 2))]
    back_a, back_b = empty_like_picture(planar), empty_like_picture(planar)
    src_c = torch.empty(npix * 9 // 4, dtype=u8, device="cuda").random_(0, 256)
    dst_c = torch.empty_like(src_c)
    res = {}

    def fwd_a():
        dct_amd.rgb_to_ycbcr(rgb, "420", outs=outs)

    def fwd_b():
        res["fwd"] = eager_forward(rgb)

    def inv_a():
        dct_amd.ycbcr_to_rgb(*outs, out=back_a)

    def inv_b():
        eager_inverse(*outs, back_b)

    def copy_c():
        dst_c.copy_(src_c)

    runs = {"A forward  library": fwd_a, "B forward  eager": fwd_b, "A inverse  library": inv_a,
            "B inverse  eager": inv_b, "C copy_ 2.25 B/px": copy_c}
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
    med = {k: statistics.median(v) for k, v in times.items()}
    moved = 4.5 * npix
    for k, m in med.items():
        print(f"{label} {k:20s} median {m * 1e3:8.3f} ms/step  min {min(times[k]) * 1e3:8.3f}  max {max(times[k]) * 1e3:8.3f}  "
              f"{moved / m / 1e12:6.3f} TB/s  {moved / m / 8e12:6.3f} of 8 TB/s")
    differ_f = sum(int((a != b).sum()) for a, b in zip(outs, res["fwd"]))
    differ_i = int((back_a != back_b).sum())
    want = color_ref.forward(rgb[0].cpu().numpy(), "420")
    ref_f = all(np.array_equal(o[0].cpu().numpy(), w) for o, w in zip(outs, want))
    ref_i = np.array_equal(back_a[0].cpu().numpy(), color_ref.inverse(*want))
    ok = differ_f == 0 and differ_i == 0 and ref_f and ref_i
    c = med["C copy_ 2.25 B/px"]
    print(f"{label} forward A/B = {med['A forward  library'] / med['B forward  eager']:5.3f}  A's rate = "
          f"{c / med['A forward  library']:5.3f} of C's;  inverse A/B = "
          f"{med['A inverse  library'] / med['B inverse  eager']:5.3f}  A's rate = {c / med['A inverse  library']:5.3f} of C's;  "
          f"bytes that differ from B: {differ_f} + {differ_i}; frame 0 equals color_ref: {ref_f and ref_i}  "
          f"{'ok' if ok else 'FAIL'}")
    return ok


results = [one_pass(False), one_pass(True)]
print("gate (every byte of A equals B, and color_ref on frame 0):", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
