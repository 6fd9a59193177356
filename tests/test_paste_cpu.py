"""CPU: the stream paste (dctq_bits_paste_offsets, dctq_bits_paste_copy) is declared, exported and
bound and the ABI revision is unchanged; both calls refuse every bad geometry, the 2^32 payload sum
and every bad pointer before they look at a device; frame_paste's and frame_tile's host rules are
right on the host; and tools/paste_ref.py agrees with tools/extract_ref.py, tools/frame_ref.py and
an independent per-block rebuild.  No compute is attempted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bits_ref  # noqa: E402
import extract_ref  # noqa: E402
import frame_ref  # noqa: E402
import paste_ref  # noqa: E402
import window_ref  # noqa: E402

NAMES = ("dctq_bits_paste_workspace_bytes", "dctq_bits_paste_offsets", "dctq_bits_paste_copy")
EINVAL = -1
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 40, 368)


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


# ---- the interface ----------------------------------------------------------------------------------
def test_declared_in_header():
    from dct_amd.build import declared_functions, public_headers
    for name in NAMES:
        assert name in declared_functions(public_headers())
    assert "#define DCTQ_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "dct_amd.h")).read()


def test_exported_bound_and_abi_unchanged(lib):
    import dct_amd
    for so in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", so)],
                             capture_output=True, text=True).stdout
        assert set(NAMES) <= {l.split()[-1] for l in out.splitlines() if " T " in l}, so
    vp, i, z = C.c_void_p, C.c_int, C.c_size_t
    W, E = C.POINTER(dct_amd._Window), C.POINTER(dct_amd._Extent)
    assert list(lib.dctq_bits_paste_offsets.argtypes) == [vp, vp, vp, vp, z, z, W, E, i, vp, vp, vp, vp]
    assert list(lib.dctq_bits_paste_copy.argtypes) == [vp, vp, vp, vp, W, E, i, vp, vp, z, vp]
    assert lib.dctq_bits_paste_offsets.restype is i and lib.dctq_bits_paste_copy.restype is i
    assert lib.dctq_abi_version() == 6
    assert all(callable(getattr(dct_amd, f)) for f in ("bits_paste", "frame_paste", "frame_blank", "frame_tile"))
    assert '"paste.hip"' in open(os.path.join(ROOT, "dct_amd", "build.py")).read()
    assert lib.dctq_bits_paste_workspace_bytes(1000) == lib.dctq_bits_workspace_bytes(1000)
    assert lib.dctq_bits_paste_workspace_bytes(0) == lib.dctq_bits_paste_workspace_bytes(1) > 0


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " int (*f)(const uint32_t *, const int32_t *const *, const uint32_t *, const int32_t *const *, size_t,\n"
                   "          size_t, const dctq_window *, const dctq_extent *, int, uint32_t *, int32_t *, void *,\n"
                   "          void *) = dctq_bits_paste_offsets;\n"
                   " int (*g)(const uint8_t *, const uint32_t *, const uint8_t *, const uint32_t *, const dctq_window *,\n"
                   "          const dctq_extent *, int, const uint32_t *, uint8_t *, size_t, void *) = dctq_bits_paste_copy;\n"
                   " size_t (*h)(long long) = dctq_bits_paste_workspace_bytes;\n"
                   " (void)f; (void)g; (void)h; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_new_kernel_names_contain_no_existing_kernel_name():
    """tests/test_window_cpu.py finds kernels by substring."""
    import re
    csrc = os.path.join(ROOT, "dct_amd", "csrc")
    names = {}
    for f in os.listdir(csrc):
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(csrc, f)).read(), flags=re.S):
            names.setdefault(m.group(1), f)
    new = {k for k, f in names.items() if f == "paste.hip"}
    assert new == {"paste_lengths_kernel", "paste_copy_kernel"}
    for n in new:
        assert not [o for o in names if o not in new and (o in n or n in o)], n


# ---- refusals, with no device -------------------------------------------------------------------------
P = {"offsets": 0x30000, "patch_offsets": 0x34000, "out_offsets": 0x40000, "workspace": 0x50000, "bytes": 0x20001,
     "patch_bytes": 0x28002, "out_bytes": 0x60003, "out_var_num": 0x70000}
GOOD = ((1056, 32, 2, 8, 8, 1), (520, 24, 1))


def structs(wins, exts):
    import dct_amd
    n = len(wins)
    return ((dct_amd._Window * n)(*[dct_amd._Window(*v) for v in wins]),
            (dct_amd._Extent * n)(*[dct_amd._Extent(*v) for v in exts]), n)


def call_offsets(lib, wins, exts, nplanes=None, null=(), var=None, pvar=None, payload=1000, patch_payload=1000, **ptrs):
    """dctq_bits_paste_offsets on fake (never dereferenced) device pointers -> (rc, message)."""
    w, e, n = structs(wins, exts)
    p = dict(P, **ptrs)
    p.update({k: None for k in null})
    vn = None if var is None else (C.c_void_p * len(var))(*var)
    pv = None if pvar is None else (C.c_void_p * len(pvar))(*pvar)
    rc = lib.dctq_bits_paste_offsets(p["offsets"], vn, p["patch_offsets"], pv, payload, patch_payload,
                                     None if "win" in null else w, None if "ext" in null else e,
                                     n if nplanes is None else nplanes, p["out_offsets"], p["out_var_num"],
                                     p["workspace"], None)
    return rc, lib.dctq_error_string(rc).decode()


def call_copy(lib, wins, exts, nplanes=None, null=(), **ptrs):
    """dctq_bits_paste_copy likewise."""
    w, e, n = structs(wins, exts)
    p = dict(P, **ptrs)
    p.update({k: None for k in null})
    rc = lib.dctq_bits_paste_copy(p["bytes"], p["offsets"], p["patch_bytes"], p["patch_offsets"],
                                  None if "win" in null else w, None if "ext" in null else e,
                                  n if nplanes is None else nplanes, p["out_offsets"], p["out_bytes"], 1 << 20, None)
    return rc, lib.dctq_error_string(rc).decode()


GEOMETRY = [
    ((1056, 32, 2, 8, 8, 1), (520, 24, 2), "frame range"),
    ((1056, 32, 2, 8, 8, -1), (520, 24, 1), "frame0"),
    ((1056, 32, 2, 544, 8, 0), (520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 8, 16, 0), (520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 4, 8, 0), (520, 24, 1), "x0 and y0"),
    ((1052, 32, 2, 8, 8, 0), (520, 24, 1), "stored width and height"),
    ((1056, 32, 0, 8, 8, 0), (520, 24, 1), "stored nframes"),
    ((1056, 32, 2, 8, 8, 0), (516, 24, 1), "multiples of 8"),
    ((1056, 32, 2, 8, 8, 0), (520, 24, 0), "nframes"),
]


@pytest.mark.parametrize("win,ext,word", GEOMETRY)
def test_geometry_refused_with_the_window_decoders_messages(lib, win, ext, word):
    """The geometry goes through the window decoder's check: its refusals and messages, and before
    anything else is looked at (every pointer is NULL here too)."""
    everything = ("offsets", "patch_offsets", "out_offsets", "workspace", "bytes", "patch_bytes", "out_bytes")
    for call in (call_offsets, call_copy):
        for null in ((), everything):
            rc, msg = call(lib, [win], [ext], null=null)
            assert rc == EINVAL and word in msg, (call.__name__, msg)


def test_nplanes_win_ext_refused(lib):
    for call in (call_offsets, call_copy):
        for n in (0, 5, -1):
            rc, msg = call(lib, [GOOD[0]], [GOOD[1]], nplanes=n)
            assert rc == EINVAL and "nplanes" in msg
        for null in ("win", "ext"):
            rc, msg = call(lib, [GOOD[0]], [GOOD[1]], null=(null,))
            assert rc == EINVAL and "win/ext" in msg
    big = (8 * 8192, 8 * 8192, 1, 0, 0, 0)   # 2^26 blocks
    rc, msg = call_offsets(lib, [big], [(8, 8, 1)])
    assert rc == EINVAL and "2^26" in msg


def test_payload_sum_refused_after_geometry_before_pointers(lib):
    for a, b in ((1 << 32, 0), (0, 1 << 32), ((1 << 31), (1 << 31)), ((1 << 32) - 1, 1), (1 << 63, 1 << 63)):
        rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], payload=a, patch_payload=b, null=("offsets", "workspace"))
        assert rc == EINVAL and "2^32" in msg and "paste" in msg, (a, b, msg)
    # geometry comes first
    rc, msg = call_offsets(lib, [GEOMETRY[0][0]], [GEOMETRY[0][1]], payload=1 << 32)
    assert rc == EINVAL and "frame range" in msg
    # the largest legal sum passes this check: the next refusal is the NULL pointer's
    rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], payload=(1 << 31), patch_payload=(1 << 31) - 1, null=("offsets",))
    assert rc == EINVAL and "NULL" in msg


def test_pointers_refused(lib):
    for null in ("offsets", "patch_offsets", "out_offsets"):
        rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], null=(null,))
        assert rc == EINVAL and "NULL" in msg, null
        rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], **{null: P[null] + 2})
        assert rc == EINVAL and "4-byte aligned" in msg, null
    rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], null=("workspace",))
    assert rc == EINVAL and "workspace" in msg
    for null in ("bytes", "offsets", "patch_bytes", "patch_offsets", "out_offsets", "out_bytes"):
        rc, msg = call_copy(lib, [GOOD[0]], [GOOD[1]], null=(null,))
        assert rc == EINVAL and "NULL" in msg, null
    for name in ("offsets", "patch_offsets", "out_offsets"):
        rc, msg = call_copy(lib, [GOOD[0]], [GOOD[1]], **{name: P[name] + 1})
        assert rc == EINVAL and "4-byte aligned" in msg, name


def test_var_num_both_or_neither(lib):
    rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], var=[0x80000])
    assert rc == EINVAL and "both" in msg
    rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], pvar=[0x80000])
    assert rc == EINVAL and "both" in msg
    rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], var=[0x80000], pvar=[0x90000], null=("out_var_num",))
    assert rc == EINVAL and "out_var_num" in msg
    for var, pvar in (([0], [0x90000]), ([0x80000], [0]), ([0x80002], [0x90000]), ([0x80000], [0x90002])):
        rc, msg = call_offsets(lib, [GOOD[0]], [GOOD[1]], var=var, pvar=pvar)
        assert rc == EINVAL and "var_num[k]" in msg


# ---- tools/paste_ref.py against the other definitions ----------------------------------------------------
def random_stream(rng, n):
    """Random bytes in blocks of the issue's lengths -> (bytes uint8, offsets uint32 [n + 1])."""
    ln = rng.choice(LENGTHS, n)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


CASES = {
    "a": ([(1, 16, 24)], [((0, 1), (8, 16), (8, 16))]),
    "b": ([(4, 40, 24)], [((1, 3), (8, 32), (8, 16))]),
    "c": ([(1, 16, 1040)], [((0, 1), (0, 16), (240, 800))]),
    "d": ([(2, 32, 48), (2, 16, 24), (2, 16, 24)],
          [((0, 2), (8, 24), (16, 40)), ((1, 2), (0, 8), (8, 24)), ((0, 1), (8, 16), (0, 8))]),
    "e": ([(1, 16, 16), (2, 8, 24), (1, 24, 8), (3, 8, 8)],
          [((0, 1), (8, 16), (0, 16)), ((1, 2), (0, 8), (8, 16)), ((0, 1), (8, 16), (0, 8)), ((2, 3), (0, 8), (0, 8))]),
    "f": ([(2, 32, 48), (2, 16, 24), (2, 16, 24)],
          [((0, 2), (0, 32), (0, 48)), ((0, 2), (0, 16), (0, 24)), ((0, 2), (0, 16), (0, 24))]),
    "g": ([(2, 32, 48), (2, 16, 24), (2, 16, 24)],
          [((0, 1), (0, 8), (0, 8)), ((0, 1), (0, 8), (0, 8)), ((1, 2), (8, 16), (16, 24))]),
}


def rebuild(data, off, shapes, windows, pdata, poff, var, pvar):
    """The definition once more, with per-block lists and explicit loops over coordinates."""
    blocks = [bytes(data[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    vn = [int(v) for plane in var for v in plane]
    pblocks = [bytes(pdata[poff[i]:poff[i + 1]]) for i in range(len(poff) - 1)]
    pvn = [int(v) for plane in pvar for v in plane]
    first = d = 0
    for (f, h, w), ((f0, f1), (y0, y1), (x0, x1)) in zip(shapes, windows):
        bh, bw = h // 8, w // 8
        for ff in range(f0, f1):
            for yy in range(y0 // 8, y1 // 8):
                for xx in range(x0 // 8, x1 // 8):
                    s = first + (ff * bh + yy) * bw + xx
                    blocks[s], vn[s] = pblocks[d], pvn[d]
                    d += 1
        first += f * bh * bw
    assert d == len(pblocks)
    return b"".join(blocks), [0] + list(np.cumsum([len(b) for b in blocks])), vn


@pytest.mark.parametrize("case", list(CASES))
def test_paste_stream_is_the_per_block_rebuild_and_inverts_window_stream(case):
    shapes, windows = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    nbs = [f * (h // 8) * (w // 8) for f, h, w in shapes]
    wnbs = [b.size for b in window_ref.blocks(shapes, windows)]
    data, off = random_stream(rng, sum(nbs))
    pdata, poff = random_stream(rng, sum(wnbs))
    var = [rng.integers(-5, 1000, n).astype(np.int32) for n in nbs]
    pvar = [rng.integers(2000, 3000, n).astype(np.int32) for n in wnbs]
    out, new, ovar = paste_ref.paste_stream(data, off, shapes, windows, pdata, poff, var, pvar)
    wb, wo, wv = rebuild(data, off, shapes, windows, pdata, poff, var, pvar)
    assert bytes(out) == wb and new.tolist() == wo and np.concatenate(ovar).tolist() == wv
    assert new.dtype == np.uint32 and new[0] == 0
    # the window of the result is the patch; pasting the base's own window back gives the base
    gb, go, gv = extract_ref.window_stream(out, new, shapes, windows, ovar)
    assert bytes(gb) == bytes(pdata) and go.tolist() == poff.tolist()
    assert all(np.array_equal(a, b) for a, b in zip(gv, pvar))
    cb, co, cv = extract_ref.window_stream(data, off, shapes, windows, var)
    back, boff, bvar = paste_ref.paste_stream(data, off, shapes, windows, cb, co, var, cv)
    assert bytes(back) == bytes(data) and boff.tolist() == off.tolist()
    assert all(np.array_equal(a, b) for a, b in zip(bvar, var))
    # without var_nums
    o2, n2, v2 = paste_ref.paste_stream(data, off, shapes, windows, pdata, poff)
    assert bytes(o2) == wb and n2.tolist() == wo and v2 is None


def test_paste_stream_lengths_are_exact_mod_2_32_and_refusals():
    shapes, windows = CASES["a"]
    # a 1000-byte block is not clamped to 368
    off = (np.array([0, 5, 5, 1005, 1006, 1010, 1011]) + 0x80000000).astype(np.uint32)
    with pytest.raises(ValueError):   # the reference holds bytes from 0: such offsets leave them
        paste_ref.paste_stream(np.zeros(0, np.uint8), off, shapes, windows, np.zeros(700, np.uint8), [0, 700])
    off = np.array([0, 5, 5, 1005, 1006, 1010, 1011], np.uint32)
    rng = np.random.default_rng(1)
    data, pdata = rng.integers(0, 256, 1011, dtype=np.uint8), rng.integers(0, 256, 700, dtype=np.uint8)
    out, new, _ = paste_ref.paste_stream(data, off, shapes, windows, pdata, [0, 700])
    assert new.tolist() == [0, 5, 5, 1005, 1006, 1706, 1707] and bytes(out[1006:1706]) == bytes(pdata)
    with pytest.raises(ValueError):
        paste_ref.paste_stream(data, off, shapes, windows, pdata, [0, 700], var_nums=[np.zeros(6, np.int32)])
    with pytest.raises(ValueError):
        paste_ref.paste_stream(data, off, shapes, windows, pdata, [0, 300, 700])
    with pytest.raises(ValueError):
        paste_ref.paste_stream(data, off[:-1], shapes, windows, pdata, [0, 700])


# ---- containers on the host ----------------------------------------------------------------------------
def coded(rng, n):
    """n blocks of valid codes (bits_ref) -> (payload, offsets)."""
    blocks = [[(int(rng.integers(-40, 40)) or 1, int(rng.integers(0, 3)))] * int(rng.integers(0, 6)) for _ in range(n)]
    return bits_ref.pack(blocks)


def container(rng, shapes, adaptive=False, colour=False, crops=None, quality=50):
    n = sum(f * (h // 8) * (w // 8) for f, h, w in shapes)
    data, off = coded(rng, n)
    var = rng.integers(0, 5000, n).astype(np.int32) if adaptive else None
    return frame_ref.pack(data, off, shapes, quality, adaptive, var, colour, crops=crops)


@pytest.mark.parametrize("adaptive", [False, True])
def test_frame_paste_of_frame_window_is_the_identity(adaptive):
    rng = np.random.default_rng(7)
    # plain planes with a crop, a 4:2:0 picture with a crop, a 4:4:4 picture
    for shapes, colour, crops, region, at in (
            ([(3, 40, 48), (3, 24, 24)], False, [(2, 2), (0, 5)], [((8, 38), (16, 46)), ((8, 16), (0, 19))], [(8, 16), (8, 0)]),
            ([(2, 48, 64), (2, 24, 32), (2, 24, 32)], True, [(10, 2), (0, 0), (0, 0)], ((16, 38), (32, 62)), (16, 32)),
            ([(2, 48, 64), (2, 24, 32), (2, 24, 32)], True, [(10, 2), (0, 0), (0, 0)], ((0, 16), (16, 48)), (0, 16)),
            ([(2, 24, 32)] * 3, True, None, ((8, 24), (8, 16)), (8, 8))):
        b = container(rng, shapes, adaptive, colour, crops)
        for frames in ((0, shapes[0][0]), (1, 2)):
            w = extract_ref.frame_window(b, region=region, frames=frames)
            assert paste_ref.frame_paste(b, w, at=at, frame=frames[0]) == b
        # and a different patch of the same geometry lands where the window says
        other = extract_ref.frame_window(container(rng, shapes, adaptive, colour, crops), region=region, frames=(1, 2))
        got = paste_ref.frame_paste(b, other, at=at, frame=1)
        assert got != b and extract_ref.frame_window(got, region=region, frames=(1, 2)) == other
        assert extract_ref.frame_window(got, frames=(0, 1)) == extract_ref.frame_window(b, frames=(0, 1))
        p = frame_ref.parse(got)
        assert p["shapes"] == shapes and p["crops"] == frame_ref.parse(b)["crops"]


def test_frame_paste_refusals_on_the_host():
    import dct_amd
    rng = np.random.default_rng(3)
    base = container(rng, [(2, 40, 48)], crops=[(2, 2)])            # true 38 x 46
    col = container(rng, [(2, 48, 64), (2, 24, 32), (2, 24, 32)], colour=True, crops=[(10, 2), (0, 0), (0, 0)])  # 38 x 62

    def both(buf, patch, **kw):
        """paste_ref refuses, and so do the package's host rules on the same headers."""
        with pytest.raises(ValueError):
            paste_ref.frame_paste(buf, patch, **kw)
        hb, hp = (dct_amd._frame_header(x[:112], len(x)) for x in (buf, patch))
        with pytest.raises(dct_amd.DctqError):
            dct_amd._paste_windows(hb, hp, kw.get("at", (0, 0)), kw.get("frame", 0))

    def fine(buf, patch, **kw):
        paste_ref.frame_paste(buf, patch, **kw)
        hb, hp = (dct_amd._frame_header(x[:112], len(x)) for x in (buf, patch))
        return dct_amd._paste_windows(hb, hp, kw.get("at", (0, 0)), kw.get("frame", 0))

    tile = container(rng, [(1, 16, 16)])
    assert fine(base, tile, at=(8, 16), frame=1) == [((1, 2), (8, 24), (16, 32))]
    both(base, container(rng, [(1, 16, 16)], quality=60), at=(8, 16))
    both(base, container(rng, [(1, 16, 16)], adaptive=True), at=(8, 16))
    both(base, container(rng, [(1, 16, 16)] * 3, colour=True), at=(8, 16))
    both(base, container(rng, [(1, 16, 16)] * 2), at=(8, 16))
    both(col, container(rng, [(1, 16, 16)] * 3, colour=True), at=(16, 16))      # 4:4:4 into 4:2:0
    both(base, tile, at=(4, 16))
    both(base, tile, at=(8, 12))
    both(base, tile, at=(-8, 16))
    both(col, container(rng, [(1, 16, 16), (1, 8, 8), (1, 8, 8)], colour=True), at=(8, 16))   # m is 16
    both(base, tile, at=(8, 16), frame=2)
    both(base, tile, at=(8, 16), frame=-1)
    both(base, container(rng, [(3, 16, 16)]), at=(8, 16))
    # the two conditions per axis, on the 38 x 46 picture
    both(base, tile, at=(24, 16))                                               # rows 24..40 leave 38, no crop
    both(base, tile, at=(8, 32))                                                # columns 32..48 leave 46
    both(base, container(rng, [(1, 16, 16)], crops=[(2, 0)]), at=(8, 16))       # a crop that ends inside
    both(base, container(rng, [(1, 16, 16)], crops=[(3, 0)]), at=(24, 16))      # true rows end at 37, not 38
    assert fine(base, container(rng, [(1, 16, 16)], crops=[(2, 0)]), at=(24, 16)) == [((0, 1), (24, 40), (16, 32))]
    assert fine(base, container(rng, [(1, 16, 16)], crops=[(2, 2)]), at=(24, 32)) == [((0, 1), (24, 40), (32, 48))]
    both(base, container(rng, [(1, 16, 16)], crops=[(0, 2)]), at=(24, 32))      # columns fine, rows not
    both(base, container(rng, [(1, 48, 16)]), at=(0, 16))                       # taller than the picture
    # a picture: one at, on plane 0; plain planes of different sizes: a list
    assert fine(col, container(rng, [(1, 32, 16), (1, 16, 8), (1, 16, 8)], colour=True, crops=[(10, 0), (0, 0), (0, 0)]),
                at=(16, 32)) == [((0, 1), (16, 48), (32, 48)), ((0, 1), (8, 24), (16, 24)), ((0, 1), (8, 24), (16, 24))]
    both(col, container(rng, [(1, 16, 16), (1, 8, 8), (1, 8, 8)], colour=True), at=[(16, 16)] * 3)
    two = container(rng, [(1, 32, 32), (1, 16, 16)])
    both(two, container(rng, [(1, 8, 8), (1, 8, 8)]), at=(8, 8))
    both(two, container(rng, [(1, 8, 8), (1, 8, 8)]), at=[(8, 8)])
    assert fine(two, container(rng, [(1, 8, 8), (1, 8, 8)]), at=[(16, 8), (8, 0)]) == \
        [((0, 1), (16, 24), (8, 16)), ((0, 1), (8, 16), (0, 8))]


@pytest.mark.parametrize("adaptive", [False, True])
def test_frame_blank(adaptive):
    shapes = [(2, 16, 24), (2, 8, 16)]
    b = paste_ref.frame_blank(shapes, 70, adaptive, crops=[(3, 0), (0, 1)])
    p = frame_ref.parse(b)
    assert p["shapes"] == shapes and p["quality"] == 70 and p["adaptive"] == adaptive and p["crops"] == [(3, 0), (0, 1)]
    assert len(p["payload"]) == 0 and not p["lengths"].any() and p["length_bytes"] == 1
    assert (p["var_nums"] is None) if not adaptive else not p["var_nums"].any()
    assert not bits_ref.unpack(p["payload"], p["offsets"]).any()     # an empty block is zero coefficients
    assert frame_ref.parse(paste_ref.frame_blank([(8, 8)], 50))["crops"] is None


@pytest.mark.parametrize("colour", [False, True])
def test_frame_tile_on_the_host(colour):
    import dct_amd
    rng = np.random.default_rng(11)
    m = 16 if colour else 8
    hs, ws = [m, 2 * m, m], [2 * m, m]          # true sizes; the last row and column end off-grid
    cut_h, cut_w = 5, 3

    def tile(r, c):
        h, w = hs[r], ws[c]
        crop = (cut_h if r == 2 else 0, cut_w if c == 1 else 0)
        if colour:
            return container(rng, [(2, h, w), (2, h // 2, w // 2), (2, h // 2, w // 2)], True, True,
                             [crop, (0, 0), (0, 0)] if any(crop) else None)
        return container(rng, [(2, h, w), (2, h, w)], True, False, [crop, crop] if any(crop) else None)

    grid = [[tile(r, c) for c in range(2)] for r in range(3)]
    got = paste_ref.frame_tile(grid)
    p = frame_ref.parse(got)
    H, W = sum(hs), sum(ws)
    assert p["shapes"][0] == (2, H, W) and p["crops"][0] == (cut_h, cut_w)
    y = 0
    for r in range(3):
        x = 0
        for c in range(2):
            region = ((y, y + hs[r] - (cut_h if r == 2 else 0)), (x, x + ws[c] - (cut_w if c == 1 else 0)))
            assert extract_ref.frame_window(got, region=region) == grid[r][c], (r, c)
            x += ws[c]
        y += hs[r]
    # the package's layout rules give the same geometry from the headers alone
    heads = [[dct_amd._frame_header(b[:112], len(b)) for b in row] for row in grid]
    shapes, crops, ats = dct_amd._tile_layout(heads)
    rs, rc, ra = paste_ref.tile_layout([[frame_ref.parse(b) for b in row] for row in grid])
    assert (shapes, crops) == (rs, rc) == (p["shapes"], p["crops"]) and ats == ra
    # refusals
    for bad in ([grid[0], grid[1][:1]],                               # ragged
                [grid[2], grid[0]],                                   # a bottom crop that is not last
                [[row[1], row[0]] for row in grid],                   # a right crop that is not last
                [[grid[0][0], grid[1][1]]],                           # heights differ along a row
                [[grid[0][0]], [grid[0][1]]]):                        # widths differ along a column
        with pytest.raises(ValueError):
            paste_ref.frame_tile(bad)
        with pytest.raises(dct_amd.DctqError):
            dct_amd._tile_layout([[dct_amd._frame_header(b[:112], len(b)) for b in row] for row in bad])
    other = container(rng, [(2, m, 2 * m)] * (1 if not colour else 3), True, colour, quality=51)
    for bad in ([[grid[0][0], other]], [[grid[0][0]], [other]]):
        with pytest.raises(ValueError):
            paste_ref.frame_tile(bad)
        with pytest.raises(dct_amd.DctqError):
            dct_amd._tile_layout([[dct_amd._frame_header(b[:112], len(b)) for b in row] for row in bad])


def test_python_refusals_need_no_device():
    """bits_paste checks its arguments before it touches the library's device side."""
    import dct_amd
    with pytest.raises(dct_amd.DctqError):
        dct_amd.bits_paste(None, None, [(1, 16, 24)], [((0, 1), (8, 16), (8, 12))], None, None)
    with pytest.raises(dct_amd.DctqError):
        dct_amd.bits_paste(None, None, [(1, 16, 24)], [((0, 1), (8, 16), (8, 16))], None, None)   # bytes is no tensor
