"""CPU: the reduced-size decoder (dctq_decode_bits_window_scaled_planes, Plan.decode_bits_scaled,
decompress(scale=)).  The definition of tools/scaled_ref.py is checked on its own terms (its
matrices are orthonormal, a constant block comes back, an independent fp64 evaluation agrees);
the symbol is declared, exported, bound and in the product code object, six kernels next to an
unchanged set; the ABI revision is unchanged; and the library refuses every bad argument before
it looks at the plan or at a device, so these refusals are checked with no GPU.  No compute is
attempted."""
import ctypes as C
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scaled_ref  # noqa: E402

NAME = "dctq_decode_bits_window_scaled_planes"
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


def table(q, adaptive):
    """The plan's quantization table, from the library's host tables (no device)."""
    import dct_amd
    return dct_amd.debug_tables(q, adaptive)[3].reshape(8, 8)


# ---- the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4])
def test_dn_literals_are_orthonormal(n):
    """Dn Dn^T = I within 2e-16, the products and sums taken exactly (rationals), so the figure is the
    literals' own and not the arithmetic's."""
    d = [[Fraction(float(v)) for v in row] for row in scaled_ref.D[n]]
    worst = max(abs(sum(d[i][k] * d[j][k] for k in range(n)) - (1 if i == j else 0))
                for i in range(n) for j in range(n))
    print(f"n = {n}: max |Dn Dn^T - I| = {float(worst):.3e}")
    assert worst <= Fraction(2e-16), float(worst)
    assert scaled_ref.D[2][0, 0] == float.fromhex("0x1.6a09e667f3bcdp-1")
    assert scaled_ref.D[4][1, 0] == float.fromhex("0x1.4e7ae9144f0fcp-1")
    assert scaled_ref.D[4][1, 1] == float.fromhex("0x1.1517a7bdb3896p-2")


def test_constant_blocks_come_back_at_scale_8(lib):
    """A block of constant pixel value p at q50 adaptive: its only coefficient is the DC, 8 (p - 128)
    quantized by Q[0][0] = 16 (the DC is never adjusted by an adaptive plan), so every p with an even
    p - 128 is a multiple of the quantizer's step and must come back as p, whatever var_num says;
    an odd one comes back as the neighbour its tie rounded to."""
    import dct_amd
    Q = table(50, True)
    assert Q[0, 0] == 16.0
    dc = np.zeros(256, np.int16)
    assert dct_amd.diag().dctq_debug_dc_table(50, dc.ctypes.data) == 0
    q = np.zeros((256, 64), np.int16)
    q[:, 0] = dc
    for vn in (0, 4096 * 1000, 2 ** 31 - 1):
        got = scaled_ref.blocks(q, Q, 8, True, np.full(256, vn, np.int64))[:, 0, 0].astype(int)
        p = np.arange(256)
        even = (p - 128) % 2 == 0
        assert np.array_equal(got[even], p[even]), vn
        assert np.abs(got - p).max() <= 1 and np.array_equal(got, 128 + 2 * dc.astype(int)), vn
    # ... and at every scale a DC-only block is flat
    for s in (2, 4):
        px = scaled_ref.blocks(q, Q, s, True, np.zeros(256, np.int64))
        assert (px == px[:, :1, :1]).all() and np.array_equal(px[:, 0, 0].astype(int), 128 + 2 * dc.astype(int)), s


def cos_matrix(n):
    """The n-point orthonormal DCT-II matrix through cos: Dn[u][i] = c(u) cos((2 i + 1) u pi / (2 n))."""
    u, i = np.arange(n)[:, None], np.arange(n)[None, :]
    c = np.where(u == 0, np.sqrt(1.0 / n), np.sqrt(2.0 / n))
    return c * np.cos((2 * i + 1) * u * np.pi / (2 * n))


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("scale", [2, 4, 8])
def test_against_an_independent_evaluation(lib, scale, adaptive):
    """out = Dn^-1 x Dn^-T with Dn built through cos and inverted by numpy.linalg, the dequantization
    restated here: within 1e-9 of scaled_ref before rounding.  Corners are seeded uniform int16 in
    [-2048, 2047], which holds every coefficient a u8 picture quantizes to (|c| <= 1024); there
    the sums' terms stay below 2048 * 29 * 1.9 * 16 * 0.43 * 0.5 = 4e5 in all, so a handful of
    roundings of 1.1e-16 relative each is 5e-10 at the very most.  var_num sits on both clamp
    edges (0.1 and 1.0 of the scale factor's argument), just inside and just outside each."""
    n = 8 // scale
    rng = np.random.default_rng(100 * scale + adaptive)
    N = 4096
    q = np.zeros((N, 8, 8), np.int16)
    q[:, :n, :n] = rng.integers(-2048, 2048, (N, n, n))
    q[:, n:, :] = rng.integers(-2048, 2048, (N, 8 - n, 8))   # outside the corner: must not matter
    edges = [0, 409599, 409600, 409601, 4095999, 4096000, 4096001, 2 ** 31 - 1]   # var = 100 and 1000
    vn = np.array(edges * (N // len(edges)), np.int64)
    Q = table(50, adaptive)
    got = scaled_ref.unrounded(q.reshape(N, 64), Q, scale, adaptive, vn)
    # the restatement
    c = q[:, :n, :n].astype(np.float64)
    if adaptive:
        nv = np.clip(vn / 4096.0 / 1000.0, 0.1, 1.0)
        x = c * Q[:n, :n] * (2.0 - nv)[:, None, None]
        x[:, 0, 0] = c[:, 0, 0] * Q[0, 0]
    else:
        x = c / Q[:n, :n]
    inv = np.linalg.inv(cos_matrix(n))
    want = np.einsum("iu,buv,jv->bij", inv, x, inv) * (n / 8.0) + 128.0
    worst = np.abs(got - want).max()
    print(f"scale {scale} adaptive {adaptive}: max |scaled_ref - independent| = {worst:.3e}")
    assert worst <= 1e-9, worst
    clean = q.copy()
    clean[:, n:, :] = 0
    clean[:, :n, n:] = 0
    assert np.array_equal(got, scaled_ref.unrounded(clean.reshape(N, 64), Q, scale, adaptive, vn))
    # any int16 is decoded: the extremes agree to the same relative accuracy (16 x the magnitudes)
    q[:, :n, :n] = rng.choice(np.array([-32768, -32767, 32767, 1, 0], np.int16), (N, n, n))
    got = scaled_ref.unrounded(q.reshape(N, 64), Q, scale, adaptive, vn)
    c = q[:, :n, :n].astype(np.float64)
    x = c / Q[:n, :n]
    if adaptive:
        x = c * Q[:n, :n] * (2.0 - nv)[:, None, None]
        x[:, 0, 0] = c[:, 0, 0] * Q[0, 0]
    want = np.einsum("iu,buv,jv->bij", inv, x, inv) * (n / 8.0) + 128.0
    assert np.abs(got - want).max() <= 16e-9


def test_planes_places_blocks():
    """planes(): block (f, r, c) of a stored plane lands at rows r n.., columns c n.. of frame f, and a
    window is the slice of the whole."""
    shapes = [(2, 16, 24), (1, 8, 8)]
    nb = 2 * 2 * 3 + 1
    q = np.zeros((nb, 64), np.int16)
    q[:, 0] = np.arange(nb) * 8 - 40                  # DC only, Q = 1: pixel = 128 + DC / 8
    Q = np.ones((8, 8))
    whole = scaled_ref.planes(q, shapes, Q, 4, False)
    assert [p.shape for p in whole] == [(2, 4, 6), (1, 2, 2)]
    assert np.array_equal(whole[0][:, ::2, ::2].ravel(), 128 + np.arange(12) - 5)
    assert (whole[0][:, 1::2, 1::2] == whole[0][:, ::2, ::2]).all() and int(whole[1][0, 0, 0]) == 128 + 12 - 5
    win = scaled_ref.planes(q, shapes, Q, 4, False, windows=[((1, 2), (8, 16), (8, 24)), ((0, 1), (0, 8), (0, 8))])
    assert np.array_equal(win[0], whole[0][1:2, 2:4, 2:6]) and np.array_equal(win[1], whole[1])
    with pytest.raises(ValueError):
        scaled_ref.planes(q[:-1], shapes, Q, 4, False)
    with pytest.raises(ValueError):
        scaled_ref.blocks(q, Q, 3, False)
    with pytest.raises(ValueError):
        scaled_ref.blocks(q, Q, 2, True)             # adaptive without var_num


# ---- the interface ----------------------------------------------------------------------------------
def test_declared_exported_bound_and_abi_unchanged(lib):
    import dct_amd
    from dct_amd.build import declared_functions, public_headers
    assert NAME in declared_functions([os.path.join(ROOT, "include", "dct_amd.h")])
    assert NAME in declared_functions(public_headers())
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr
    for lit in ("0x1.6a09e667f3bcdp-1", "0x1.4e7ae9144f0fcp-1", "0x1.1517a7bdb3896p-2"):
        assert lit in hdr, lit                        # the definition is stated in the header too
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", name)],
                             capture_output=True, text=True).stdout
        assert NAME in {l.split()[-1] for l in out.splitlines() if " T " in l}, name
    vp, i = C.c_void_p, C.c_int
    fn = getattr(lib, NAME)
    assert fn.restype is i
    assert list(fn.argtypes) == [vp, vp, vp, vp, C.POINTER(dct_amd._Window), C.POINTER(dct_amd._Plane), i, i, vp]
    assert lib.dctq_abi_version() == 6
    assert callable(dct_amd.Plan.decode_bits_scaled)
    src = open(os.path.join(ROOT, "dct_amd", "build.py")).read()
    assert '"decode_scaled.hip"' in src and '"window_core.h"' in src


def test_header_compiles_as_c99_with_the_scaled_call(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " int (*f)(const dctq_plan *, const uint8_t *, const uint32_t *, const int32_t *const *,\n"
                   "          const dctq_window *, const dctq_plane *, int, int, void *)\n"
                   "     = dctq_decode_bits_window_scaled_planes;\n"
                   " (void)f; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_kernels_in_product_code_object(lib, tmp_path):
    """bits_window_to_scaled_pixels<ADAPTIVE, LOG2S>: six instantiations, next to the unchanged three
    of bits_window_to_pixels and of bits_to_pixels (whose own tests look for their names inside every
    kernel's name, which is why this kernel's name holds neither)."""
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

    assert inst("bits_window_to_scaled_pixelsI", 10) == {f"bits_window_to_scaled_pixelsILb{a}ELi{l}EEE"
                                                         for a in (0, 1) for l in (1, 2, 3)}, names
    legal = ((0, 0), (0, 1), (1, 0))
    assert inst("bits_window_to_pixelsI", 10) == {f"bits_window_to_pixelsILb{a}ELb{f}EEE" for a, f in legal}, names
    assert inst("bits_to_pixelsI", 10) == {f"bits_to_pixelsILb{a}ELb{f}EEE" for a, f in legal}, names


@pytest.mark.parametrize("which", ["product", "diag"])
def test_the_record_says_only_new_kernels_differ(which):
    """profiles/r18/isa_parent_*.json are the per-kernel digests of the parent's libraries
    (tools/isa_digest.py), isa_after_*.json this change's: every parent kernel kept its machine code
    (bits_rebuild_half gained a template parameter whose default is what it did), and the six scaled
    kernels are all that is new."""
    parent = json.load(open(os.path.join(ROOT, "profiles", "r18", f"isa_parent_{which}.json")))
    after = json.load(open(os.path.join(ROOT, "profiles", "r18", f"isa_after_{which}.json")))
    new = sorted(k for k in after if k not in parent)
    assert len(new) == 6 and all("bits_window_to_scaled_pixels" in k for k in new), new
    assert all(after.get(k) == v for k, v in parent.items())
    res = open(os.path.join(ROOT, "profiles", "r18", "resources.txt")).read()
    assert res.count("ScratchSize [bytes/lane]: 0") == 6 and res.count("Function Name:") == 6


# ---- refusals, with no device -------------------------------------------------------------------------
def call(lib, wins, dsts, log2_scale, nplanes=None, plan=None, null_win=False, null_dst=False, pixels=0x10000):
    """The entry point on fake (never dereferenced) device pointers; returns (rc, message)."""
    import dct_amd
    n = len(wins)
    w = (dct_amd._Window * n)(*[dct_amd._Window(*v) for v in wins])
    d = (dct_amd._Plane * n)(*[dct_amd._Plane(pixels, st, fst, wd, ht, nf) for (wd, ht, nf, st, fst) in dsts])
    rc = getattr(lib, NAME)(plan, C.c_void_p(0x20000), C.c_void_p(0x30000), None, None if null_win else w,
                            None if null_dst else d, n if nplanes is None else nplanes, log2_scale, None)
    return rc, lib.dctq_error_string(rc).decode()


def dst(wd, ht, nf, st=None, fst=None):
    st = wd if st is None else st
    return (wd, ht, nf, st, st * ht if fst is None else fst)


STORED = (1056, 32, 2)


def test_good_geometries_get_as_far_as_the_plan(lib):
    """With a NULL plan a geometry that passes is refused for the plan, and for nothing else: the
    cases below are refused for what they say."""
    for l in (1, 2, 3):
        n = 8 >> l
        # the whole plane; one block; a window at an origin; widths that are no multiple of 8
        for win, d in (((*STORED, 0, 0, 0), dst(1056 >> l, 32 >> l, 2)),
                       ((*STORED, 1048, 24, 1), dst(n, n, 1)),
                       ((*STORED, 8, 8, 1), dst(65 * n, 3 * n, 1)),
                       ((*STORED, 8, 8, 0), dst(33 * n, n, 2, 33 * n + n, (33 * n + n) * n + n))):
            rc, msg = call(lib, [win], [d], l, pixels=0x10000 + n)
            assert rc == EINVAL and msg == "plan is NULL", (l, win, d, msg)
    rc, msg = call(lib, [(*STORED, 0, 0, 0), (528, 16, 2, 520, 8, 0), (528, 16, 2, 0, 0, 0)],
                   [dst(132, 4, 2), dst(1, 1, 2), dst(66, 2, 2)], 3)
    assert rc == EINVAL and msg == "plan is NULL", msg


def test_refused_log2_scale_comes_first(lib):
    for l in (0, 4, -1, 8):
        rc, msg = call(lib, [(*STORED, 0, 0, 0)], [dst(528, 16, 2)], l, null_win=True)
        assert rc == EINVAL and "log2_scale" in msg, (l, msg)


@pytest.mark.parametrize("l", [1, 2, 3])
def test_refused_destinations(lib, l):
    n = 8 >> l
    win = (*STORED, 8, 8, 0)
    w, h = 33 * n, 2 * n
    bad = [
        (dst(0, h, 1), "positive multiples"), (dst(w, 0, 1), "positive multiples"), (dst(-n, h, 1), "positive multiples"),
        (dst(w, h, 0), "nframes"),
        (dst(w, h, 1, w - n), "stride"),                                   # stride below the width
        (dst(w, h, 2, w, w * h - n), "frame_stride smaller"),
    ]
    if n > 1:
        bad += [(dst(w + 1, h, 1, w + n), "positive multiples"), (dst(w, h + 1, 1), "positive multiples"),
                (dst(w, h, 1, w + 1), "stride"), (dst(w, h, 2, w, w * h + 1), "aligned")]
    for d, why in bad:
        rc, msg = call(lib, [win], [d], l)
        assert rc == EINVAL and why in msg, (l, d, msg)
    if n > 1:
        rc, msg = call(lib, [win], [dst(w, h, 1)], l, pixels=0x10000 + n // 2)
        assert rc == EINVAL and "aligned" in msg, msg
    rc, msg = call(lib, [win], [dst(w, h, 1)], l, pixels=0)
    assert rc == EINVAL and "NULL" in msg, msg


@pytest.mark.parametrize("l", [1, 2, 3])
@pytest.mark.parametrize("win,blocks,why", [
    ((1056, 32, 2, 8, 8, 1), (65, 3, 2), "frame range"),             # frames 1..3 of 2
    ((1056, 32, 2, 8, 8, 2), (65, 3, 1), "frame range"),
    ((1056, 32, 2, 8, 8, -1), (65, 3, 1), "frame0"),
    ((1056, 32, 2, 544, 8, 0), (65, 3, 1), "leaves the stored plane"),
    ((1056, 32, 2, 8, 16, 0), (65, 3, 1), "leaves the stored plane"),
    ((1056, 32, 2, 2 ** 31 - 8, 0, 0), (65, 3, 1), "leaves the stored plane"),
    ((1056, 32, 2, 0, 0, 0), (133, 4, 1), "leaves the stored plane"),
    ((1056, 32, 2, 4, 8, 0), (65, 3, 1), "x0 and y0"),
    ((1056, 32, 2, 8, 12, 0), (65, 3, 1), "x0 and y0"),
    ((1056, 32, 2, -8, 8, 0), (65, 3, 1), "x0 and y0"),
    ((1056, 32, 2, 8, -8, 0), (65, 3, 1), "x0 and y0"),
    ((1052, 32, 2, 8, 8, 0), (65, 3, 1), "stored width and height"),
    ((1056, 36, 2, 8, 8, 0), (65, 3, 1), "stored width and height"),
    ((0, 32, 2, 0, 0, 0), (1, 1, 1), "stored width and height"),
    ((1056, 32, 0, 8, 8, 0), (65, 3, 1), "stored nframes"),
    ((8192, 8192, 64, 0, 0, 0), (1, 1, 1), "2^26"),                   # N = 2^26 exactly
])
def test_refused_for_what_the_window_call_refuses(lib, l, win, blocks, why):
    """Every geometry dctq_decode_bits_window_planes refuses (tests/test_window_cpu.py), the window's
    extent given in blocks: the destination is that many n x n pixels."""
    n = 8 >> l
    rc, msg = call(lib, [win], [dst(blocks[0] * n, blocks[1] * n, blocks[2])], l)
    assert rc == EINVAL and why in msg, (rc, msg)


def test_refused_pointers_and_counts(lib):
    good = ((*STORED, 8, 8, 1), dst(65 * 2, 3 * 2, 1))
    assert call(lib, [good[0]], [good[1]], 2, null_win=True) == (EINVAL, "win/dst is NULL")
    assert call(lib, [good[0]], [good[1]], 2, null_dst=True) == (EINVAL, "win/dst is NULL")
    for n in (0, 5, -1):
        rc, msg = call(lib, [good[0]], [good[1]], 2, nplanes=n)
        assert rc == EINVAL and "nplanes" in msg, (n, msg)
    half = (8192, 8192, 32, 0, 0, 0)
    rc, msg = call(lib, [half, half], [dst(1, 1, 1)] * 2, 3)
    assert rc == EINVAL and "2^26" in msg, msg
    rc, msg = call(lib, [half, (8192, 8184, 32, 0, 0, 0)], [dst(1, 1, 1)] * 2, 3)
    assert rc == EINVAL and msg == "plan is NULL", msg
    # the unscaled call's own rules are what they were: its destinations are whole 8 x 8 blocks
    import dct_amd
    w = (dct_amd._Window * 1)(dct_amd._Window(*good[0]))
    d = (dct_amd._Plane * 1)(dct_amd._Plane(0x10000, 132, 132 * 6, 130, 6, 1))
    rc = lib.dctq_decode_bits_window_planes(None, C.c_void_p(0x20000), C.c_void_p(0x30000), None, w, d, 1, None)
    assert rc == EINVAL and "multiples of 8" in lib.dctq_error_string(rc).decode()


# ---- what Python refuses, quoted --------------------------------------------------------------------
def test_python_refusals_are_quoted():
    import dct_amd
    for bad in (1, 3, 16, 0, -2, 2.5, "2", None, True):
        with pytest.raises(dct_amd.DctqError, match=r"scale must be 2, 4 or 8, got"):
            dct_amd._log2_scale(bad)
    assert [dct_amd._log2_scale(s) for s in (2, 4, 8)] == [1, 2, 3]
    # decompress refuses before it looks at the buffer
    with pytest.raises(dct_amd.DctqError, match=r"scale must be 2, 4 or 8, got 3"):
        dct_amd.decompress(b"", scale=3)
    with pytest.raises(dct_amd.DctqError, match=r"scale together with region is not supported"):
        dct_amd.decompress(b"", scale=2, region=((0, 8), (0, 8)))
    sw = dct_amd._stored_windows
    with pytest.raises(dct_amd.DctqError, match=r"windows needs one entry per plane \(2\), got 1"):
        sw([(1, 8, 8)] * 2, [((0, 1), (0, 8), (0, 8))])
    with pytest.raises(dct_amd.DctqError, match=r"rows and columns must be multiples of 8"):
        sw([(1, 16, 16)], [((0, 1), (4, 12), (0, 8))])
    with pytest.raises(dct_amd.DctqError, match=r"is empty or leaves the stored plane"):
        sw([(1, 16, 16)], [((0, 2), (0, 8), (0, 8))])
    with pytest.raises(dct_amd.DctqError, match=r"must be \(\(f0, f1\), \(y0, y1\), \(x0, x1\)\)"):
        sw([(1, 16, 16)], [((0, 1), (0, 8))])
    with pytest.raises(dct_amd.DctqError, match=r"height and width must be multiples of 8"):
        sw([(1, 12, 16)], [((0, 1), (0, 8), (0, 8))])
    with pytest.raises(dct_amd.DctqError, match=r"more than 2\^26 - 1 blocks"):
        sw([(64, 8192, 8192)], [((0, 1), (0, 8), (0, 8))])
    wins, wshapes, nbs = sw([(2, 16, 24), (8, 8)], [((1, 2), (8, 16), (0, 24)), ((0, 1), (0, 8), (0, 8))])
    assert wshapes == [(1, 8, 24), (1, 8, 8)] and nbs == [12, 1]
    assert (wins[0].width, wins[0].height, wins[0].nframes, wins[0].x0, wins[0].y0, wins[0].frame0) == (24, 16, 2, 0, 8, 1)


def test_decompress_scaled_arithmetic(monkeypatch):
    """decompress(scale=): the windows, the reduced sizes and the views, with a stubbed decode (no device)."""
    import dct_amd
    seen = []

    class StubPlan:
        def decode_bits_scaled(self, b, o, shapes, scale, windows=None, outs=None, var_nums=None, stream=None):
            seen.append((scale, windows))
            return [np.zeros((f1 - f0, (y1 - y0) // scale, (x1 - x0) // scale), np.uint8)
                    for (f0, f1), (y0, y1), (x0, x1) in windows]

    class Bytes:
        device = "cpu"

    parts = {"quality": 50, "adaptive": False, "colour": False, "shapes": [(3, 32, 104), (3, 8, 8)], "offsets": None,
             "bytes": Bytes(), "var_nums": None, "crops": [(5, 4), (0, 1)]}     # true sizes 27 x 100 and 8 x 7
    monkeypatch.setattr(dct_amd, "frame_unpack", lambda buf, stream=None: parts)
    monkeypatch.setattr(dct_amd, "_frame_plan", lambda q, a, dev: StubPlan())
    got = dct_amd.decompress(b"", scale=4, frames=(1, 3))
    assert seen == [(4, [((1, 3), (0, 32), (0, 104)), ((1, 3), (0, 8), (0, 8))])]
    assert [g.shape for g in got] == [(2, 7, 25), (2, 2, 2)]             # ceil(27 / 4) x ceil(100 / 4), 2 x ceil(7 / 4)
    got = dct_amd.decompress(b"", scale=8)
    assert [g.shape for g in got] == [(3, 4, 13), (3, 1, 1)]
    with pytest.raises(dct_amd.DctqError, match=r"frames \(0, 4\) is empty or outside the 3 frames"):
        dct_amd.decompress(b"", scale=2, frames=(0, 4))
    assert len(seen) == 2
