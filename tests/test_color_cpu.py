"""CPU: the colour front and back end (dctq_rgb_to_ycbcr_planes / dctq_ycbcr_to_rgb_planes) is
declared, exported, bound and hosted; its kernels are in the product code object; the ABI
revision is unchanged; and the definition's plain-numpy statement (tools/color_ref.py, the GPU
tests' yardstick) is checked by itself: ranges over every colour, triples worked out by hand,
and the 4:4:4 round trip.  No compute is attempted without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import color_ref  # noqa: E402

NAMES = ["dctq_rgb_to_ycbcr_planes", "dctq_ycbcr_to_rgb_planes"]


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


# ---- the interface ----------------------------------------------------------------------------------
def test_declared_in_header():
    from dct_amd.build import declared_functions, public_headers
    assert set(NAMES) <= set(declared_functions([os.path.join(ROOT, "include", "dct_amd.h")]))
    assert set(NAMES) <= set(declared_functions(public_headers()))


def test_exported_from_both_libraries(lib):
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", name)],
                             capture_output=True, text=True).stdout
        got = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(NAMES) <= got, (name, set(NAMES) - got)


def test_bound(lib):
    import dct_amd
    vp, i = C.c_void_p, C.c_int
    pl, rgb = C.POINTER(dct_amd._Plane), C.POINTER(dct_amd._Rgb)
    want = {
        "dctq_rgb_to_ycbcr_planes": ([rgb, pl, pl, pl, vp], i),
        "dctq_ycbcr_to_rgb_planes": ([pl, pl, pl, rgb, vp], i),
    }
    for name, (args, res) in want.items():
        fn = getattr(dct_amd.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert [f[0] for f in dct_amd._Rgb._fields_] == ["pixels", "stride", "frame_stride", "channel_stride",
                                                     "pixel_step", "width", "height", "nframes"]
    assert C.sizeof(dct_amd._Rgb) == 48  # a pointer, three long long, four int
    assert callable(dct_amd.rgb_desc) and callable(dct_amd.rgb_to_ycbcr) and callable(dct_amd.ycbcr_to_rgb)


def test_abi_version_unchanged(lib):
    assert lib.dctq_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_header_compiles_as_c99_with_rgb(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " dctq_rgb r;\n"
                   " int (*f)(const dctq_rgb *, const dctq_plane *, const dctq_plane *, const dctq_plane *,\n"
                   "          void *) = dctq_rgb_to_ycbcr_planes;\n"
                   " int (*b)(const dctq_plane *, const dctq_plane *, const dctq_plane *, const dctq_rgb *,\n"
                   "          void *) = dctq_ycbcr_to_rgb_planes;\n"
                   " r.pixels = 0; r.stride = 0; r.frame_stride = 0; r.channel_stride = -1; r.pixel_step = 3;\n"
                   " r.width = r.height = r.nframes = 0;\n"
                   " (void)r; (void)f; (void)b; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_frame_rgb_host_builds(lib):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_rgb"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert os.access(os.path.join(ROOT, "host", "frame_rgb"), os.X_OK)
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    clean = mk[mk.index("clean:"):]
    assert "frame_rgb" in all_line.split() and "frame_rgb" in clean.split()


def test_kernels_in_product_code_object(lib, tmp_path):
    """rgb_to_ycc_kernel<STEP, S420> and ycc_to_rgb_kernel<STEP, S420> for STEP in {1, 3, 4} and
    both subsamplings: BGR orders are no instantiation of their own."""
    import glob
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    local = str(tmp_path / "libdct_amd.so")
    shutil.copy(os.path.join(ROOT, "dct_amd", "libdct_amd.so"), local)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", local], cwd=str(tmp_path), check=True,
                   capture_output=True)
    names = set()
    objs = glob.glob(local + ".*gfx950")
    assert objs, os.listdir(str(tmp_path))
    for obj in objs:
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--symbols", obj], capture_output=True,
                             text=True).stdout
        names |= {w for w in out.split() if w.startswith("_Z") and "." not in w}
    for key in ("rgb_to_ycc_kernel", "ycc_to_rgb_kernel"):
        got = {k[k.index(key):][:len(key) + 11] for k in names if key in k}
        assert got == {key + f"ILi{s}ELb{h}EEE" for s in (1, 3, 4) for h in (0, 1)}, (key, names)


# ---- tools/color_ref.py by itself ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def every():
    """Every colour once, and its unclamped (Y, Cb, Cr)."""
    rgb = color_ref.all_colours()
    return rgb, color_ref.ycc_pixels(rgb)


def test_all_colours_are_all_colours(every):
    rgb, _ = every
    n = (rgb[..., 0].astype(np.uint32) << 16 | rgb[..., 1].astype(np.uint32) << 8 | rgb[..., 2]).ravel()
    assert np.array_equal(n, np.arange(1 << 24, dtype=np.uint32))


def test_forward_needs_no_clamp(every):
    _, (y, cb, cr) = every
    for name, p in (("Y", y), ("Cb", cb), ("Cr", cr)):
        assert (int(p.min()), int(p.max())) == (0, 255), name


def test_forward_intermediates_fit_int32():
    """The largest sums of the three forward rows and the inverse's terms, from the coefficients' signs."""
    hi = max(19595 * 255 + 38470 * 255 + 7471 * 255 + 32768, 32768 * 255 + 8388608 + 32767)
    lo = min(-11059 * 255 - 21709 * 255 + 8388608 + 32767, -27439 * 255 - 5329 * 255 + 8388608 + 32767)
    assert 0 <= lo and hi < 2 ** 31
    assert max(116130 * 128, 22554 * 128 + 46802 * 128) + 32768 < 2 ** 31


@pytest.mark.parametrize("rgb,ycc", [
    ((0, 0, 0), (0, 128, 128)),          # (32768) >> 16; (8388608 + 32767) >> 16 = 128
    ((255, 255, 255), (255, 128, 128)),  # 65536 * 255 + 32768; the chroma rows sum to 0
    ((128, 128, 128), (128, 128, 128)),
    ((255, 0, 0), (76, 85, 255)),        # 5029493 >> 16; 5601330 >> 16; 16777215 >> 16
    ((0, 255, 0), (150, 44, 21)),        # 9842618 >> 16; 2885580 >> 16; 1424430 >> 16
    ((0, 0, 255), (29, 255, 107)),       # 1937873 >> 16; 16777215 >> 16; 7062480 >> 16
])
def test_forward_by_hand(rgb, ycc):
    px = np.array(rgb, np.uint8).reshape(1, 1, 3)
    assert tuple(int(p[0, 0]) for p in color_ref.forward(px, "444")) == ycc


def test_subsampling_rounds_by_hand():
    """Two black pixels over two blue ones: Cb 128 + 128 + 255 + 255 = 766, (766 + 2) >> 2 = 192
    (191 without the + 2); Cr 128 + 128 + 107 + 107 = 470, (470 + 2) >> 2 = 118 (117 without)."""
    patch = np.array([[[0, 0, 0], [0, 0, 0]], [[0, 0, 255], [0, 0, 255]]], np.uint8)
    y, cb, cr = color_ref.forward(patch, "420")
    assert y.tolist() == [[0, 0], [29, 29]] and cb.tolist() == [[192]] and cr.tolist() == [[118]]


def test_inverse_by_hand_clamps_both_sides():
    """(Y, Cb, Cr) = (128, 255, 0): cb = 127, cr = -128.
    R = 128 + ((-11760768 + 32768) >> 16) = 128 - 179 = -51 -> 0
    G = 128 + ((-2864358 + 5990656 + 32768) >> 16) = 128 + 48 = 176
    B = 128 + ((14748510 + 32768) >> 16) = 128 + 225 = 353 -> 255"""
    assert [int(v) for v in color_ref.rgb_pixels(128, 255, 0)] == [-51, 176, 353]
    one = lambda v: np.array([[v]], np.uint8)
    assert color_ref.inverse(one(128), one(255), one(0)).tolist() == [[[0, 176, 255]]]
    # 4:2:0: one chroma sample serves its 2x2 pixels
    y = np.array([[128, 0], [255, 128]], np.uint8)
    assert color_ref.inverse(y, one(255), one(0)).tolist() == [[[0, 176, 255], [0, 48, 225]],
                                                                [[76, 255, 255], [0, 176, 255]]]


def test_inverse_ranges(every):
    """Before the clamp: -1 .. 256 on forward-produced triples; on any (Y, Cb, Cr) -227 .. 480, both
    from B: 0 + ((116130 * -128 + 32768) >> 16) = -227 and 255 + ((116130 * 127 + 32768) >> 16) = 480
    (R alone spans -179 .. 433)."""
    rgb, (y, cb, cr) = every
    back = color_ref.rgb_pixels(y, cb, cr)
    assert (min(int(c.min()) for c in back), max(int(c.max()) for c in back)) == (-1, 256)
    anyt = color_ref.rgb_pixels(rgb[..., 0], rgb[..., 1], rgb[..., 2])  # every byte triple as (Y, Cb, Cr)
    assert (min(int(c.min()) for c in anyt), max(int(c.max()) for c in anyt)) == (-227, 480)
    assert (int(anyt[0].min()), int(anyt[0].max())) == (-179, 433)


def test_round_trip_444_within_one(every):
    rgb, _ = every
    back = color_ref.inverse(*color_ref.forward(rgb, "444"))
    assert int(np.abs(back.astype(np.int16) - rgb.astype(np.int16)).max()) == 1


# ---- rgb_desc: what can be checked without a device -----------------------------------------------------
def test_rgb_desc_refusals():
    import torch

    import dct_amd
    with pytest.raises(dct_amd.DctqError, match="uint8"):
        dct_amd.rgb_desc(torch.zeros((16, 16, 3), dtype=torch.float32))
    with pytest.raises(dct_amd.DctqError, match="uint8"):
        dct_amd.rgb_desc(np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(dct_amd.DctqError, match="HIP device"):
        dct_amd.rgb_desc(torch.zeros((16, 16, 3), dtype=torch.uint8))
    for shape in ((16, 16, 2), (16, 16, 5), (3, 16, 16), (16, 16), (1, 1, 16, 16, 3)):
        with pytest.raises(dct_amd.DctqError, match="C 3 or 4"):
            dct_amd.rgb_desc(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(dct_amd.DctqError):
        dct_amd.rgb_to_ycbcr(torch.zeros((16, 16, 3), dtype=torch.uint8))
