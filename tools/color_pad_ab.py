"""Same-box A/B of the padding colour stage on 1080p frames (4:2:0), each direction and for
interleaved RGB and planar pictures:
  A  the new launch on 1920 x 1080: rgb_to_ycbcr(pad=True) / ycbcr_to_rgb(size=(1080, 1920));
  B  the aligned launch on 1920 x 1088, the parent's kernels: the per-pixel yardstick (A and B
     both work on 1920 x 1088 extended pixels);
  C  what a user did before: an index-gather edge pad in torch (rgb[:, ys][:, :, xs]) plus the
     aligned launch; on the way back the aligned launch plus a cropping copy;
  D  the new launch on 1918 x 1078, contiguous: its row stride of 5754 B (1918 B planar) is no
     multiple of 4, so every row is misaligned differently.
Interleaved rounds, each sample `--launches` steps back to back after one untimed step, device
events, medians, and the min-max spread.  Reports the times, A/B, A/C and D/B per extended pixel,
and B's own spread.  Exits non-zero unless every byte of A and D equals tools/color_ref.py on a
sampled frame; speed does not decide the exit status.

    python tools/color_pad_ab.py [--rounds 10] [--launches 3] [--frames 64]
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
ap.add_argument("--frames", type=int, default=64)
args = ap.parse_args()

F, u8 = args.frames, torch.uint8
EH, EW = 1088, 1920
print(f"{F} frames 1080p 4:2:0, extended {EW} x {EH}; device {torch.cuda.get_device_name(0)}")


def picture(planar, h, w):
    """Three synthetic planes of different seeds as the channels of a contiguous RGB stack of h x w."""
    chans = [dct_amd.synth(777 + 50000 * c, "uniform", EW, EH, F)[:, :h, :w] for c in range(3)]
    if planar:
        return torch.stack(chans, 1).contiguous().permute(0, 2, 3, 1)
    return torch.stack(chans, -1).contiguous()


def empty_picture(planar, h, w):
    if planar:
        return torch.empty((F, 3, h, w), dtype=u8, device="cuda").permute(0, 2, 3, 1)
    return torch.empty((F, h, w, 3), dtype=u8, device="cuda")


def planes(h, w):
    return [torch.empty(s, dtype=u8, device="cuda") for s in ((F, h, w), (F, h // 2, w // 2), (F, h // 2, w // 2))]


def one_pass(planar: bool) -> bool:
    label = "planar" if planar else "rgb   "
    src_a, src_b, src_d = picture(planar, 1080, 1920), picture(planar, EH, EW), picture(planar, 1078, 1918)
    out_a, out_b, out_c, out_d = planes(EH, EW), planes(EH, EW), planes(EH, EW), planes(1088, 1920)
    back_a, back_b, back_d = empty_picture(planar, 1080, 1920), empty_picture(planar, EH, EW), empty_picture(planar, 1078, 1918)
    back_c, tmp_c = empty_picture(planar, 1080, 1920), empty_picture(planar, EH, EW)
    ys = torch.arange(EH, device="cuda").clamp_(max=1079)
    xs = torch.arange(EW, device="cuda").clamp_(max=1919)
    assert src_d.stride(1) % 4 != 0

    def fwd_c():
        padded = src_a[:, ys][:, :, xs]
        dct_amd.rgb_to_ycbcr(padded if not planar else padded.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1),
                             "420", outs=out_c)

    def inv_c():
        dct_amd.ycbcr_to_rgb(*out_a, out=tmp_c)
        back_c.copy_(tmp_c[:, :1080, :1920])

    runs = {
        "A forward  pad 1920x1080": lambda: dct_amd.rgb_to_ycbcr(src_a, "420", outs=out_a, pad=True),
        "B forward  aligned 1920x1088": lambda: dct_amd.rgb_to_ycbcr(src_b, "420", outs=out_b),
        "C forward  torch pad + aligned": fwd_c,
        "D forward  pad 1918x1078": lambda: dct_amd.rgb_to_ycbcr(src_d, "420", outs=out_d, pad=True),
        "A inverse  crop 1920x1080": lambda: dct_amd.ycbcr_to_rgb(*out_a, out=back_a, size=(1080, 1920)),
        "B inverse  aligned 1920x1088": lambda: dct_amd.ycbcr_to_rgb(*out_b, out=back_b),
        "C inverse  aligned + torch crop": inv_c,
        "D inverse  crop 1918x1078": lambda: dct_amd.ycbcr_to_rgb(*out_d, out=back_d, size=(1078, 1918)),
    }
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
    ext_px = F * EH * EW
    for k, m in med.items():
        print(f"{label} {k:32s} median {m * 1e3:8.3f} ms/step  min {min(times[k]) * 1e3:8.3f}  max {max(times[k]) * 1e3:8.3f}  "
              f"{m / ext_px * 1e12:7.3f} ps per extended pixel")
    ok = True
    for tag, src, outs, back, (h, w) in (("A", src_a, out_a, back_a, (1080, 1920)), ("D", src_d, out_d, back_d, (1078, 1918))):
        f = F // 2
        want = color_ref.forward_padded(src[f].cpu().numpy(), "420")
        ref_f = all(np.array_equal(o[f].cpu().numpy(), p) for o, p in zip(outs, want))
        ref_i = np.array_equal(back[f].cpu().numpy(), color_ref.inverse_cropped(*want, h, w))
        same_c = tag != "A" or (all(torch.equal(a, c) for a, c in zip(out_a, out_c)) and torch.equal(back_a, back_c))
        print(f"{label} {tag}: frame {f} equals color_ref forward {ref_f} inverse {ref_i}; equals C: {same_c}")
        ok = ok and ref_f and ref_i and same_c
    for d in ("forward", "inverse"):
        a, b, c, dd = (med[next(k for k in med if k.startswith(f"{t} {d}"))] for t in "ABCD")
        kb = next(k for k in med if k.startswith(f"B {d}"))
        spread = (max(times[kb]) - min(times[kb])) / b
        print(f"{label} {d}: A/B = {a / b:5.3f}  A/C = {a / c:5.3f}  D/B = {dd / b:5.3f} (per extended pixel; "
              f"B's min-max spread {spread:5.3f} of its median)")
    return ok


results = [one_pass(False), one_pass(True)]
print("gate (A and D equal color_ref on a sampled frame, A equals C):", "PASS" if all(results) else "FAIL")
sys.exit(0 if all(results) else 1)
