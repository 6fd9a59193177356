"""CPU: pictures of any size -- the definition of the edge padding and the crop
(tools/color_ref.py), the container "frame c1" that records the crop (tools/frame_ref.py), the
three new C symbols, and the proof that no kernel of the parent changed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import color_ref  # noqa: E402
import frame_ref  # noqa: E402

SIZES = [(1, 1), (7, 3), (17, 9), (33, 31)]  # W x H
NEW = ("dctq_rgb_to_ycbcr_pad_planes", "dctq_ycbcr_to_rgb_crop_planes", "dctq_pad_planes")


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


# ---- 1. color_ref ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("w,h", SIZES)
def test_forward_padded_is_forward_of_numpy_edge_padding(w, h, sub):
    m = 16 if sub == "420" else 8
    rng = np.random.default_rng(100 * w + h)
    x = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    eh, ew = -(-h // m) * m, -(-w // m) * m
    padded = np.pad(x, ((0, 0), (0, eh - h), (0, ew - w), (0, 0)), mode="edge")
    assert np.array_equal(color_ref.pad_edge(x, m), padded)
    got, want = color_ref.forward_padded(x, sub), color_ref.forward(padded, sub)
    assert [g.shape for g in got] == [(2, eh, ew)] + [(2, eh * 8 // m, ew * 8 // m)] * 2
    assert all(np.array_equal(g, v) for g, v in zip(got, want))
    # a picture of whole blocks is not changed
    assert color_ref.pad_edge(padded, m) is not None and np.array_equal(color_ref.pad_edge(padded, m), padded)


@pytest.mark.parametrize("sub", ["420", "444"])
@pytest.mark.parametrize("w,h", SIZES)
def test_inverse_cropped_is_the_crop_of_inverse(w, h, sub):
    m, s = (16, 2) if sub == "420" else (8, 1)
    eh, ew = -(-h // m) * m, -(-w // m) * m
    rng = np.random.default_rng(7 * w + h)
    y = rng.integers(0, 256, (2, eh, ew), dtype=np.uint8)
    cb, cr = (rng.integers(0, 256, (2, eh // s, ew // s), dtype=np.uint8) for _ in range(2))
    got = color_ref.inverse_cropped(y, cb, cr, h, w)
    assert got.shape == (2, h, w, 3) and got.dtype == np.uint8
    assert np.array_equal(got, color_ref.inverse(y, cb, cr)[:, :h, :w])


def test_pad_edge_refuses_an_empty_picture():
    with pytest.raises(ValueError):
        color_ref.pad_edge(np.zeros((0, 4, 3), np.uint8), 8)
    with pytest.raises(ValueError):
        color_ref.forward_padded(np.zeros((4, 4, 3), np.uint8), "422")


# ---- 2. frame_ref ------------------------------------------------------------------------------------------
def stream(shapes, seed=0):
    """A payload and offsets of the right block count (any bytes: the container does not look inside)."""
    n = sum(f * (h // 8) * (w // 8) for f, h, w in shapes)
    rng = np.random.default_rng(seed)
    ln = rng.integers(1, 40, n)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8).tobytes(), off, n


CONTAINERS = {
    "plain": ([(2, 16, 24), (1, 8, 8)], False, [(3, 2), (0, 7)]),
    "colour 420": ([(2, 32, 64), (2, 16, 32), (2, 16, 32)], True, [(2, 14), (0, 0), (0, 0)]),
    "colour 444": ([(1, 16, 24), (1, 16, 24), (1, 16, 24)], True, [(7, 0), (0, 0), (0, 0)]),
}


@pytest.mark.parametrize("name", list(CONTAINERS))
@pytest.mark.parametrize("adaptive", [False, True])
def test_crops_round_trip_and_no_crop_is_frame_v1(name, adaptive):
    shapes, colour, crops = CONTAINERS[name]
    payload, off, n = stream(shapes)
    vn = np.arange(n, dtype=np.int32) if adaptive else None
    box = frame_ref.pack(payload, off, shapes, 50, adaptive, vn, colour, crops=crops)
    assert box[:8] == b"DCTQFRC1"
    d = frame_ref.parse(box)
    assert d["crops"] == crops and d["shapes"] == shapes and d["payload"] == payload
    assert np.array_equal(d["offsets"], off) and d["colour"] == colour
    # everything but the magic and the fourth words is frame v1
    v1 = frame_ref.pack(payload, off, shapes, 50, adaptive, vn, colour)
    assert v1[:8] == b"DCTQFRM1" and frame_ref.parse(v1)["crops"] is None
    same = bytearray(box)
    same[:8] = v1[:8]
    for k in range(len(shapes)):
        same[60 + 16 * k:64 + 16 * k] = bytes(4)
    assert bytes(same) == v1
    # no crop, said either way, is today's container byte for byte
    assert frame_ref.pack(payload, off, shapes, 50, adaptive, vn, colour, crops=None) == v1
    assert frame_ref.pack(payload, off, shapes, 50, adaptive, vn, colour, crops=[(0, 0)] * len(shapes)) == v1


@pytest.mark.parametrize("name", list(CONTAINERS))
def test_every_refusal_of_a_cropped_container(name):
    shapes, colour, crops = CONTAINERS[name]
    payload, off, _ = stream(shapes)
    box = frame_ref.pack(payload, off, shapes, 50, colour=colour, crops=crops)
    cases = frame_ref.refusal_cases(box)
    rules = [r for r, _ in cases]
    assert len(set(rules)) == len(rules)
    for rule in ("pad_right above the most", "pad_bottom above the most", "no crop at all under the crop magic",
                 "the fourth words under the frame v1 magic", "bad magic"):
        assert rule in rules
    assert ("a chroma plane with a pad" in rules) == colour
    for rule, bad in cases:
        with pytest.raises(frame_ref.FrameError):
            frame_ref.parse(bad)
            pytest.fail(rule)


def test_pack_refuses_bad_crops():
    shapes, colour, _ = CONTAINERS["colour 420"]
    payload, off, _ = stream(shapes)
    for crops in ([(16, 0), (0, 0), (0, 0)], [(0, 1), (0, 1), (0, 0)], [(1, 1)], [(-1, 0), (0, 0), (0, 0)]):
        with pytest.raises(frame_ref.FrameError):
            frame_ref.pack(payload, off, shapes, 50, colour=colour, crops=crops)
    plain, _, _ = CONTAINERS["plain"]
    payload, off, _ = stream(plain)
    with pytest.raises(frame_ref.FrameError):
        frame_ref.pack(payload, off, plain, 50, crops=[(8, 0), (0, 0)])


def test_frame_v1_is_what_it_was():
    shapes, _, _ = CONTAINERS["plain"]
    payload, off, _ = stream(shapes)
    v1 = frame_ref.pack(payload, off, shapes, 50)
    cases = frame_ref.refusal_cases(v1)
    assert len(cases) == 20 and cases[3][1][:8] == b"DCTQFRM2"
    word = dict(cases)["plane record's fourth word set"]
    with pytest.raises(frame_ref.FrameError, match="fourth word"):
        frame_ref.parse(word)
    for rule, bad in cases:
        with pytest.raises(frame_ref.FrameError):
            frame_ref.parse(bad)
            pytest.fail(rule)


# ---- 3. ABI ------------------------------------------------------------------------------------------------
def test_abi_and_new_symbols(lib, tmp_path):
    from dct_amd.build import declared_functions, public_headers
    assert lib.dctq_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in header
    declared = declared_functions(public_headers())
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", "libdct_amd.so")],
                         capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW:
        assert name in declared and name in exported, name
        getattr(lib, name)
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\nint main(void){ int (*f)(const dctq_plane *, const dctq_plane *, int, void *) = '
                   "dctq_pad_planes; dctq_rgb r; (void)f; (void)r; return 0; }\n")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                         "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr


def test_no_work_without_valid_arguments(lib):
    """The refusals that need no device: NULLs and plane counts are refused before anything else."""
    import ctypes as C

    import dct_amd
    p = dct_amd._Plane(None, 8, 64, 8, 8, 1)
    assert lib.dctq_pad_planes(None, None, 1, None) == -1
    assert lib.dctq_pad_planes(C.byref(p), C.byref(p), 0, None) == -1
    assert lib.dctq_pad_planes(C.byref(p), C.byref(p), 5, None) == -1
    assert lib.dctq_pad_planes(C.byref(p), C.byref(p), 1, None) == -1      # NULL pixels
    assert lib.dctq_rgb_to_ycbcr_pad_planes(None, C.byref(p), C.byref(p), C.byref(p), None) == -1
    assert lib.dctq_ycbcr_to_rgb_crop_planes(C.byref(p), C.byref(p), C.byref(p), None, None) == -1


def test_color_pad_host_builds(lib):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "color_pad"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert os.access(os.path.join(ROOT, "host", "color_pad"), os.X_OK)
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    clean = mk.split("clean:")[1]
    assert "color_pad" in all_line.split() and "color_pad" in clean.split()


# ---- 4. the parent's colour kernels are unchanged ------------------------------------------------------------
@pytest.mark.parametrize("which,library", [("product", "libdct_amd.so"), ("diag", "libdct_amd_diag.so")])
def test_moving_code_to_color_core_left_the_colour_kernels_alone(lib, which, library):
    """This change moved the row loads and stores of color.hip into color_core.h; the twelve
    kernels of color.hip must have kept their machine code.  profiles/r15/isa_parent_*.json are
    the per-kernel digests of the parent's libraries (tools/isa_digest.py), isa_after_*.json this
    change's: the record says that only the thirteen new kernels differ.  The built library is
    held to the parent's digests of those twelve kernels when it comes from the compiler the
    record was made with (profiles/r15/toolchain.txt); with another compiler no digest can be
    compared, and the test only checks that old and new kernels are all there."""
    import isa_digest
    from dct_amd.build import build_info
    parent = json.load(open(os.path.join(ROOT, "profiles", "r15", f"isa_parent_{which}.json")))
    after = json.load(open(os.path.join(ROOT, "profiles", "r15", f"isa_after_{which}.json")))
    new = sorted(k for k in after if k not in parent)
    assert len(new) == 13 and all("pad_kernel" in k or "crop_kernel" in k or "pad_planes_kernel" in k for k in new)
    assert all(after[k] == v for k, v in parent.items()), "the record itself: no parent kernel changed"
    colour = [k for k in parent if "rgb_to_ycc_kernel" in k or "ycc_to_rgb_kernel" in k]
    assert len(colour) == 12
    built = isa_digest.digest(os.path.join(ROOT, "dct_amd", library))
    assert set(colour) <= set(built) and set(new) <= set(built)
    recorded = open(os.path.join(ROOT, "profiles", "r15", "toolchain.txt")).read().split("\n")[0].strip()
    if (build_info().get("hipcc") or [""])[0].strip() == recorded:
        assert {k: built[k] for k in colour} == {k: parent[k] for k in colour}
