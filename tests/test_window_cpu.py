"""CPU: the window decoder (dctq_decode_bits_window_planes) is declared, exported, bound and in
the product code object; the ABI revision is unchanged; the library refuses every bad window
geometry before it looks at the plan or at a device, so these refusals are checked with no GPU
(the one refusal that needs a real plan, a missing var_num on an adaptive plan, is in
tests/test_window_gpu.py); tools/window_ref.py covers each window's blocks exactly once; and
decompress's region arithmetic is right on the host.  No compute is attempted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import window_ref  # noqa: E402

NAME = "dctq_decode_bits_window_planes"
EINVAL = -1
SHAPES = [(2, 32, 1056), (2, 16, 528), (2, 16, 528)]


def blk(f, y, x):
    return (f, (8 * y[0], 8 * y[1]), (8 * x[0], 8 * x[1]))


WINDOWS = {
    "whole": [((0, f), (0, h), (0, w)) for f, h, w in SHAPES],
    "last block": [blk((1, 2), (3, 4), (131, 132)), blk((1, 2), (1, 2), (65, 66)), blk((1, 2), (1, 2), (65, 66))],
    "first block": [blk((0, 1), (0, 1), (0, 1))] * 3,
    "65 from 1": [blk((0, 2), (0, 4), (1, 66)), blk((0, 2), (0, 2), (1, 66)), blk((0, 2), (0, 2), (1, 66))],
    "31 wide": [blk((0, 2), (0, 4), (2, 33)), blk((0, 2), (0, 2), (2, 33)), blk((0, 2), (0, 2), (2, 33))],
    "32 wide": [blk((0, 2), (0, 4), (2, 34)), blk((0, 2), (0, 2), (2, 34)), blk((0, 2), (0, 2), (2, 34))],
    "33 wide": [blk((0, 2), (0, 4), (2, 35)), blk((0, 2), (0, 2), (2, 35)), blk((0, 2), (0, 2), (2, 35))],
    "frame 1": [((1, 2), (0, h), (0, w)) for _, h, w in SHAPES],
    "rows 1..3": [blk((0, 2), (1, 4), (0, 132)), blk((0, 2), (1, 2), (0, 66)), blk((0, 2), (1, 2), (0, 66))],
    "unrelated": [blk((1, 2), (1, 4), (1, 66)), blk((1, 2), (0, 2), (0, 33)), blk((0, 1), (1, 2), (65, 66))],
}


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


# ---- the interface ----------------------------------------------------------------------------------
def test_declared_in_header():
    from dct_amd.build import declared_functions, public_headers
    assert NAME in declared_functions([os.path.join(ROOT, "include", "dct_amd.h")])
    assert NAME in declared_functions(public_headers())
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "typedef struct dctq_window {" in hdr and "} dctq_window;" in hdr
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_exported_bound_and_abi_unchanged(lib):
    import dct_amd
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", name)],
                             capture_output=True, text=True).stdout
        assert NAME in {l.split()[-1] for l in out.splitlines() if " T " in l}, name
    vp, i = C.c_void_p, C.c_int
    fn = getattr(lib, NAME)
    assert fn.restype is i
    assert list(fn.argtypes) == [vp, vp, vp, vp, C.POINTER(dct_amd._Window), C.POINTER(dct_amd._Plane), i, vp]
    assert [f for f, _ in dct_amd._Window._fields_] == ["width", "height", "nframes", "x0", "y0", "frame0"]
    assert C.sizeof(dct_amd._Window) == 24
    assert lib.dctq_abi_version() == 6
    assert callable(dct_amd.Plan.decode_bits_window)
    src = open(os.path.join(ROOT, "dct_amd", "build.py")).read()
    assert '"decode_window.hip"' in src


def test_header_compiles_as_c99_with_window(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " dctq_window w = {64, 32, 2, 8, 16, 1};\n"
                   " struct dctq_window *p = &w;\n"
                   " int (*f)(const dctq_plan *, const uint8_t *, const uint32_t *, const int32_t *const *,\n"
                   "          const dctq_window *, const dctq_plane *, int, void *) = dctq_decode_bits_window_planes;\n"
                   " (void)f; return p->width + p->height + p->nframes + p->x0 + p->y0 + p->frame0 == 123 ? 0 : 1; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_kernels_in_product_code_object(lib, tmp_path):
    """bits_window_to_pixels<ADAPTIVE, INV32> for fp64, fp32 and fp64 adaptive, next to an unchanged
    set of bits_to_pixels."""
    import glob
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    local = str(tmp_path / "libdct_amd.so")
    shutil.copy(os.path.join(ROOT, "dct_amd", "libdct_amd.so"), local)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", local], cwd=str(tmp_path), check=True,
                   capture_output=True)
    names = set()
    for obj in glob.glob(local + ".*gfx950"):
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--symbols", obj], capture_output=True,
                             text=True).stdout
        names |= {w for w in out.split() if w.startswith("_Z") and "." not in w}

    def inst(key, n):
        return {k[k.index(key):][:len(key) + n] for k in names if key in k}

    legal = ((0, 0), (0, 1), (1, 0))
    assert inst("bits_window_to_pixels", 11) == {f"bits_window_to_pixelsILb{a}ELb{f}EEE" for a, f in legal}, names
    assert inst("bits_to_pixels", 11) == {f"bits_to_pixelsILb{a}ELb{f}EEE" for a, f in legal}, names


# ---- refusals, with no device -------------------------------------------------------------------------
def call(lib, wins, dsts, nplanes=None, plan=None, null_win=False, null_dst=False):
    """The entry point on fake (never dereferenced) device pointers; returns (rc, message)."""
    import dct_amd
    n = len(wins)
    w = (dct_amd._Window * n)(*[dct_amd._Window(*v) for v in wins])
    d = (dct_amd._Plane * n)(*[dct_amd._Plane(0x10000, st, fst, wd, ht, nf) for (wd, ht, nf, st, fst) in dsts])
    rc = getattr(lib, NAME)(plan, C.c_void_p(0x20000), C.c_void_p(0x30000), None, None if null_win else w,
                            None if null_dst else d, n if nplanes is None else nplanes, None)
    return rc, lib.dctq_error_string(rc).decode()


def dst(wd, ht, nf):
    return (wd, ht, nf, wd, wd * ht)


GOOD = ((1056, 32, 2, 8, 8, 1), dst(520, 24, 1))


def test_a_good_window_gets_as_far_as_the_plan(lib):
    """With a NULL plan a geometry that passes is refused for the plan, and for nothing else: the
    cases below are refused for their geometry."""
    rc, msg = call(lib, [GOOD[0]], [GOOD[1]])
    assert rc == EINVAL and msg == "plan is NULL", msg
    rc, msg = call(lib, [GOOD[0], (528, 16, 2, 520, 8, 0), (528, 16, 2, 0, 0, 0)],
                   [GOOD[1], dst(8, 8, 2), dst(528, 16, 2)])
    assert rc == EINVAL and msg == "plan is NULL", msg


@pytest.mark.parametrize("win,d,why", [
    ((1056, 32, 2, 8, 8, 1), dst(520, 24, 2), "frame range"),       # frames 1..3 of 2
    ((1056, 32, 2, 8, 8, 2), dst(520, 24, 1), "frame range"),
    ((1056, 32, 2, 8, 8, -1), dst(520, 24, 1), "frame0"),
    ((1056, 32, 2, 544, 8, 0), dst(520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 8, 16, 0), dst(520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 2 ** 31 - 8, 0, 0), dst(520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 4, 8, 0), dst(520, 24, 1), "x0 and y0"),
    ((1056, 32, 2, 8, 12, 0), dst(520, 24, 1), "x0 and y0"),
    ((1056, 32, 2, -8, 8, 0), dst(520, 24, 1), "x0 and y0"),
    ((1056, 32, 2, 8, -8, 0), dst(520, 24, 1), "x0 and y0"),
    ((1052, 32, 2, 8, 8, 0), dst(520, 24, 1), "stored width and height"),
    ((1056, 36, 2, 8, 8, 0), dst(520, 24, 1), "stored width and height"),
    ((0, 32, 2, 0, 0, 0), dst(8, 8, 1), "stored width and height"),
    ((1056, 32, 0, 8, 8, 0), dst(520, 24, 1), "stored nframes"),
    ((1056, 32, 2, 8, 8, 0), dst(516, 24, 1), "multiples of 8"),     # the destination's own rules
    ((1056, 32, 2, 8, 8, 0), dst(520, 24, 0), "nframes"),
    ((8192, 8192, 64, 0, 0, 0), dst(8, 8, 1), "2^26"),                # N = 2^26 exactly
])
def test_refused_for_its_geometry(lib, win, d, why):
    rc, msg = call(lib, [win], [d])
    assert rc == EINVAL and why in msg, (rc, msg)


def test_refused_pointers_and_counts(lib):
    assert call(lib, [GOOD[0]], [GOOD[1]], null_win=True) == (EINVAL, "win/dst is NULL")
    assert call(lib, [GOOD[0]], [GOOD[1]], null_dst=True) == (EINVAL, "win/dst is NULL")
    for n in (0, 5, -1):
        rc, msg = call(lib, [GOOD[0]], [GOOD[1]], nplanes=n)
        assert rc == EINVAL and "nplanes" in msg, (n, msg)
    # the block limit counts every stored plane: 2^25 + 2^25
    half = (8192, 8192, 32, 0, 0, 0)
    rc, msg = call(lib, [half, half], [dst(8, 8, 1)] * 2)
    assert rc == EINVAL and "2^26" in msg, msg
    rc, msg = call(lib, [half, (8192, 8184, 32, 0, 0, 0)], [dst(8, 8, 1)] * 2)
    assert rc == EINVAL and msg == "plan is NULL", msg


# ---- the mapping's plain statement -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WINDOWS))
def test_runs_cover_the_window_once(name):
    windows = WINDOWS[name]
    runs = window_ref.runs(SHAPES, windows)
    per_plane = window_ref.blocks(SHAPES, windows)
    want = np.concatenate([b.ravel() for b in per_plane])
    got = np.concatenate([np.arange(s0, s0 + nb) for s0, nb in runs])
    assert np.array_equal(got, want), name            # raster order over the window, every block once
    assert len(set(got.tolist())) == len(got)
    assert runs[:, 1].min() >= 1 and runs[:, 1].max() <= 64
    # no run straddles a row: its blocks are one row's, consecutive
    nbs = [f * (h // 8) * (w // 8) for f, h, w in SHAPES]
    first = np.concatenate([[0], np.cumsum(nbs)])
    for s0, nb in runs:
        k = int(np.searchsorted(first, s0, side="right")) - 1
        bw = SHAPES[k][2] // 8
        assert (s0 - first[k]) // bw == (s0 + nb - 1 - first[k]) // bw and s0 + nb <= first[k + 1]
    # runs per row: ceil(wb / 64)
    assert len(runs) == sum(b.shape[0] * b.shape[1] * -(-b.shape[2] // 64) for b in per_plane)
    out = window_ref.outside(SHAPES, windows)
    assert len(out) + len(got) == sum(nbs) and not set(out.tolist()) & set(got.tolist())


def test_runs_by_hand():
    r = window_ref.runs([(2, 16, 1056)], [((1, 2), (8, 16), (8, 1056))]).tolist()
    # frame 1 starts at block 264, its row 1 at 396; columns 1..131 -> 64 + 64 + 3
    assert r == [[397, 64], [461, 64], [525, 3]]
    assert window_ref.runs(SHAPES, WINDOWS["last block"]).tolist() == [[1055, 1], [1319, 1], [1583, 1]]
    assert window_ref.blocks([(1, 16, 24)], [((0, 1), (0, 16), (8, 24))])[0].tolist() == [[[1, 2], [4, 5]]]
    for bad in ([((0, 1), (0, 16), (4, 24))], [((0, 2), (0, 16), (0, 24))], [((0, 1), (8, 8), (0, 24))]):
        with pytest.raises(ValueError):
            window_ref.runs([(1, 16, 24)], bad)


# ---- decompress's region arithmetic ---------------------------------------------------------------------
def test_region_windows_of_a_picture():
    import dct_amd
    rw = dct_amd._region_windows
    s420 = [(2, 80, 1056), (2, 40, 528), (2, 40, 528)]
    crops = [(10, 6), (0, 0), (0, 0)]                      # the true picture is 70 x 1050
    w, cuts = rw(s420, crops, True, ((3, 38), (5, 122)), (1, 2))
    assert w == [((1, 2), (0, 48), (0, 128)), ((1, 2), (0, 24), (0, 64)), ((1, 2), (0, 24), (0, 64))]
    assert cuts == [(3, 5, 35, 117)]
    w, cuts = rw(s420, crops, True, ((61, 70), (1037, 1050)), None)   # the true bottom-right corner
    assert w[0] == ((0, 2), (48, 80), (1024, 1056)) and w[1] == w[2] == ((0, 2), (24, 40), (512, 528))
    assert cuts == [(13, 13, 9, 13)]
    w, cuts = rw(s420, crops, True, None, (0, 1))
    assert w[0] == ((0, 1), (0, 80), (0, 1056)) and cuts == [(0, 0, 70, 1050)]
    w, cuts = rw(s420, None, True, ((16, 32), (32, 64)), None)         # aligned: nothing to cut
    assert w[0] == ((0, 2), (16, 32), (32, 64)) and w[1] == ((0, 2), (8, 16), (16, 32)) and cuts == [(0, 0, 16, 32)]
    s444 = [(1, 40, 136)] * 3
    w, cuts = rw(s444, None, True, ((9, 17), (7, 9)), None)
    assert w == [((0, 1), (8, 24), (0, 16))] * 3 and cuts == [(1, 7, 8, 2)]
    for region, frames in ((((0, 71), (0, 8)), None), (((0, 8), (0, 1051)), None), (((8, 8), (0, 8)), None),
                           (((9, 8), (0, 8)), None), (((-1, 8), (0, 8)), None), (None, (0, 3)), (None, (2, 2)),
                           (None, (-1, 1)), ([((0, 8), (0, 8))] * 3, None), (((0, 8),), None), (5, None),
                           (((0, 8), (0, 8), (0, 8)), None), (None, 3)):
        with pytest.raises(dct_amd.DctqError):
            rw(s420, crops, True, region, frames)


def test_region_windows_of_plain_planes():
    import dct_amd
    rw = dct_amd._region_windows
    shapes, crops = [(2, 32, 1056), (2, 32, 104)], [(0, 0), (5, 4)]    # true sizes 32 x 1056 and 27 x 100
    regions = [((9, 30), (100, 1001)), ((0, 27), (93, 100))]
    w, cuts = rw(shapes, crops, False, regions, (1, 2))
    assert w == [((1, 2), (8, 32), (96, 1008)), ((1, 2), (0, 32), (88, 104))]
    assert cuts == [(1, 4, 21, 901), (0, 5, 27, 7)]
    with pytest.raises(dct_amd.DctqError):
        rw(shapes, crops, False, ((0, 8), (0, 8)), None)     # two true sizes: one region is not enough
    with pytest.raises(dct_amd.DctqError):
        rw(shapes, crops, False, regions[:1], None)
    with pytest.raises(dct_amd.DctqError):
        rw(shapes, crops, False, [regions[0], ((0, 28), (0, 8))], None)
    same = [(3, 48, 208), (2, 48, 208)]
    w, cuts = rw(same, [(3, 5)] * 2, False, ((44, 45), (1, 203)), None)  # frames: what every plane has
    assert w == [((0, 2), (40, 48), (0, 208))] * 2 and cuts == [(4, 1, 1, 202)] * 2
    with pytest.raises(dct_amd.DctqError):
        rw(same, None, False, None, (2, 3))


def test_decompress_without_region_takes_the_old_path(monkeypatch):
    """region=None and frames=None: frame_unpack, decode_bits over the stored shapes and nothing of
    the window path (stubbed decode: no device)."""
    import dct_amd
    seen = []

    class StubPlan:
        def decode_bits(self, b, o, shapes=None, var_nums=None, stream=None):
            seen.append(("decode_bits", shapes))
            return ["y", "cb"]

        def decode_bits_window(self, b, o, shapes, windows, var_nums=None, stream=None):
            seen.append(("decode_bits_window", windows))
            return [np.zeros((f1 - f0, y1 - y0, x1 - x0), np.uint8) for (f0, f1), (y0, y1), (x0, x1) in windows]

    class Bytes:
        device = "cpu"

    parts = {"quality": 50, "adaptive": False, "colour": False, "shapes": [(2, 16, 24), (2, 8, 8)], "offsets": None,
             "bytes": Bytes(), "var_nums": None, "crops": None}
    monkeypatch.setattr(dct_amd, "frame_unpack", lambda buf, stream=None: parts)
    monkeypatch.setattr(dct_amd, "_frame_plan", lambda q, a, dev: StubPlan())
    assert dct_amd.decompress(b"") == ["y", "cb"] and seen == [("decode_bits", parts["shapes"])]
    got = dct_amd.decompress(b"", region=[((3, 9), (5, 6)), ((0, 8), (7, 8))], frames=(1, 2))
    assert seen[1] == ("decode_bits_window", [((1, 2), (0, 16), (0, 8)), ((1, 2), (0, 8), (0, 8))])
    assert [g.shape for g in got] == [(1, 6, 1), (1, 8, 1)]
    with pytest.raises(dct_amd.DctqError):
        dct_amd.decompress(b"", region=((0, 8), (0, 8)))
    assert len(seen) == 2
