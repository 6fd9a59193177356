"""CPU: the stream extraction (dctq_bits_window_offsets, dctq_bits_window_gather) is declared,
exported and bound and the ABI revision is unchanged; both calls refuse every bad geometry and
pointer before they look at a device, through the window decoder's own check; frame_window's
region rules are right on the host; and tools/extract_ref.py agrees with independent statements
of what it defines.  No compute is attempted."""
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
import window_ref  # noqa: E402

NAMES = ("dctq_bits_window_workspace_bytes", "dctq_bits_window_offsets", "dctq_bits_window_gather")
EINVAL = -1


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
        assert name in declared_functions([os.path.join(ROOT, "include", "dct_amd.h")])
        assert name in declared_functions(public_headers())
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "typedef struct dctq_extent {" in hdr and "} dctq_extent;" in hdr
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_exported_bound_and_abi_unchanged(lib):
    import dct_amd
    for so in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", so)],
                             capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(NAMES) <= exported, so
    vp, i = C.c_void_p, C.c_int
    W, E = C.POINTER(dct_amd._Window), C.POINTER(dct_amd._Extent)
    assert list(lib.dctq_bits_window_offsets.argtypes) == [vp, vp, W, E, i, vp, vp, vp, vp]
    assert list(lib.dctq_bits_window_gather.argtypes) == [vp, vp, W, E, i, vp, vp, C.c_size_t, vp]
    assert lib.dctq_bits_window_offsets.restype is i and lib.dctq_bits_window_gather.restype is i
    assert lib.dctq_bits_window_workspace_bytes.restype is C.c_size_t
    assert [f for f, _ in dct_amd._Extent._fields_] == ["width", "height", "nframes"]
    assert C.sizeof(dct_amd._Extent) == 12
    assert lib.dctq_abi_version() == 6
    assert all(callable(getattr(dct_amd, f)) for f in ("bits_window", "frame_window", "frame_concat"))
    assert '"extract.hip"' in open(os.path.join(ROOT, "dct_amd", "build.py")).read()
    # the scan's workspace, as the other offset scans state it
    assert lib.dctq_bits_window_workspace_bytes(1000) == lib.dctq_bits_workspace_bytes(1000)
    assert lib.dctq_bits_window_workspace_bytes(0) == lib.dctq_bits_window_workspace_bytes(1) > 0


def test_header_compiles_as_c99_with_extent(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " dctq_extent e = {64, 32, 2};\n"
                   " struct dctq_extent *p = &e;\n"
                   " int (*f)(const uint32_t *, const int32_t *const *, const dctq_window *, const dctq_extent *, int,\n"
                   "          uint32_t *, int32_t *, void *, void *) = dctq_bits_window_offsets;\n"
                   " int (*g)(const uint8_t *, const uint32_t *, const dctq_window *, const dctq_extent *, int,\n"
                   "          const uint32_t *, uint8_t *, size_t, void *) = dctq_bits_window_gather;\n"
                   " size_t (*h)(long long) = dctq_bits_window_workspace_bytes;\n"
                   " (void)f; (void)g; (void)h; return p->width + p->height + p->nframes == 98 ? 0 : 1; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ---- refusals, with no device -------------------------------------------------------------------------
P = {"offsets": 0x30000, "win_offsets": 0x40000, "workspace": 0x50000, "bytes": 0x20000, "win_bytes": 0x60001,
     "win_var_num": 0x70000}


def structs(wins, exts):
    import dct_amd
    n = len(wins)
    return ((dct_amd._Window * n)(*[dct_amd._Window(*v) for v in wins]),
            (dct_amd._Extent * n)(*[dct_amd._Extent(*v) for v in exts]), n)


def call_offsets(lib, wins, exts, nplanes=None, null=(), var=None, **ptrs):
    """dctq_bits_window_offsets on fake (never dereferenced) device pointers -> (rc, message)."""
    w, e, n = structs(wins, exts)
    p = dict(P, **ptrs)
    p.update({k: None for k in null})
    vn = None if var is None else (C.c_void_p * len(var))(*var)
    rc = lib.dctq_bits_window_offsets(p["offsets"], vn, None if "win" in null else w, None if "ext" in null else e,
                                      n if nplanes is None else nplanes, p["win_offsets"], p["win_var_num"],
                                      p["workspace"], None)
    return rc, lib.dctq_error_string(rc).decode()


def call_gather(lib, wins, exts, nplanes=None, null=(), **ptrs):
    """dctq_bits_window_gather likewise."""
    w, e, n = structs(wins, exts)
    p = dict(P, **ptrs)
    p.update({k: None for k in null})
    rc = lib.dctq_bits_window_gather(p["bytes"], p["offsets"], None if "win" in null else w,
                                     None if "ext" in null else e, n if nplanes is None else nplanes,
                                     p["win_offsets"], p["win_bytes"], 1 << 20, None)
    return rc, lib.dctq_error_string(rc).decode()


GOOD = ((1056, 32, 2, 8, 8, 1), (520, 24, 1))

GEOMETRY = [
    ((1056, 32, 2, 8, 8, 1), (520, 24, 2), "frame range"),       # frames 1..3 of 2
    ((1056, 32, 2, 8, 8, 2), (520, 24, 1), "frame range"),
    ((1056, 32, 2, 8, 8, -1), (520, 24, 1), "frame0"),
    ((1056, 32, 2, 544, 8, 0), (520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 8, 16, 0), (520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 2 ** 31 - 8, 0, 0), (520, 24, 1), "leaves the stored plane"),
    ((1056, 32, 2, 4, 8, 0), (520, 24, 1), "x0 and y0"),
    ((1056, 32, 2, 8, 12, 0), (520, 24, 1), "x0 and y0"),
    ((1056, 32, 2, -8, 8, 0), (520, 24, 1), "x0 and y0"),
    ((1056, 32, 2, 8, -8, 0), (520, 24, 1), "x0 and y0"),
    ((1052, 32, 2, 8, 8, 0), (520, 24, 1), "stored width and height"),
    ((1056, 36, 2, 8, 8, 0), (520, 24, 1), "stored width and height"),
    ((0, 32, 2, 0, 0, 0), (8, 8, 1), "stored width and height"),
    ((1056, 32, 0, 8, 8, 0), (520, 24, 1), "stored nframes"),
    ((1056, 32, 2, 8, 8, 0), (516, 24, 1), "multiples of 8"),     # the extent's own rules
    ((1056, 32, 2, 8, 8, 0), (520, 20, 1), "multiples of 8"),
    ((1056, 32, 2, 8, 8, 0), (0, 24, 1), "multiples of 8"),
    ((1056, 32, 2, 8, 8, 0), (520, -8, 1), "multiples of 8"),
    ((1056, 32, 2, 8, 8, 0), (520, 24, 0), "nframes"),
    ((8192, 8192, 64, 0, 0, 0), (8, 8, 1), "2^26"),                # N = 2^26 exactly
]


def test_a_good_window_gets_as_far_as_the_launch_arguments(lib):
    """With a NULL offsets pointer a geometry that passes is refused for that pointer, and for nothing
    else: the cases below are refused for their geometry, whatever the pointers are."""
    three = ([GOOD[0], (528, 16, 2, 520, 8, 0), (528, 16, 2, 0, 0, 0)], [GOOD[1], (8, 8, 2), (528, 16, 2)])
    for wins, exts in (([GOOD[0]], [GOOD[1]]), three):
        assert call_offsets(lib, wins, exts, null=("offsets",)) == (EINVAL, "offsets/win_offsets is NULL")
        assert call_gather(lib, wins, exts, null=("offsets",)) == (EINVAL, "bytes/offsets/win_offsets/win_bytes is NULL")


@pytest.mark.parametrize("call", [call_offsets, call_gather])
@pytest.mark.parametrize("win,ext,why", GEOMETRY)
def test_refused_for_its_geometry(lib, call, win, ext, why):
    for null in ((), ("offsets", "win_offsets", "bytes", "win_bytes", "workspace")):   # the geometry comes first
        rc, msg = call(lib, [win], [ext], null=null)
        assert rc == EINVAL and why in msg, (rc, msg)


@pytest.mark.parametrize("call", [call_offsets, call_gather])
def test_refused_counts(lib, call):
    assert call(lib, [GOOD[0]], [GOOD[1]], null=("win",)) == (EINVAL, "win/ext is NULL")
    assert call(lib, [GOOD[0]], [GOOD[1]], null=("ext",)) == (EINVAL, "win/ext is NULL")
    for n in (0, 5, -1):
        rc, msg = call(lib, [GOOD[0]], [GOOD[1]], nplanes=n)
        assert rc == EINVAL and "nplanes" in msg, (n, msg)
    # the block limit counts every stored plane: 2^25 + 2^25
    half = (8192, 8192, 32, 0, 0, 0)
    rc, msg = call(lib, [half, half], [(8, 8, 1)] * 2)
    assert rc == EINVAL and "2^26" in msg, msg
    rc, msg = call(lib, [half, (8192, 8184, 32, 0, 0, 0)], [(8, 8, 1)] * 2, null=("offsets",))
    assert rc == EINVAL and "is NULL" in msg and "2^26" not in msg, msg


def test_refused_pointers(lib):
    g = ([GOOD[0]], [GOOD[1]])
    for name in ("offsets", "win_offsets"):
        assert call_offsets(lib, *g, null=(name,)) == (EINVAL, "offsets/win_offsets is NULL")
        rc, msg = call_offsets(lib, *g, **{name: P[name] + 2})
        assert rc == EINVAL and "4-byte aligned" in msg, msg
    assert call_offsets(lib, *g, null=("workspace",)) == (EINVAL, "workspace is NULL")
    rc, msg = call_offsets(lib, *g, workspace=P["workspace"] + 1)
    assert rc == EINVAL and "workspace must be 4-byte aligned" in msg, msg
    # var_num: every plane's, 4-byte aligned, and somewhere to put the gathered ones
    for bad in (dict(var=[None]), dict(var=[0x80002]), dict(var=[0x80000], null=("win_var_num",)),
                dict(var=[0x80000], win_var_num=P["win_var_num"] + 1)):
        rc, msg = call_offsets(lib, *g, **bad)
        assert rc == EINVAL and "var_num" in msg, (bad, msg)
    for name in ("bytes", "offsets", "win_offsets", "win_bytes"):
        assert call_gather(lib, *g, null=(name,)) == (EINVAL, "bytes/offsets/win_offsets/win_bytes is NULL")
    for name in ("offsets", "win_offsets"):
        rc, msg = call_gather(lib, *g, **{name: P[name] + 1})
        assert rc == EINVAL and "4-byte aligned" in msg, msg


# ---- frame_window's region rules, as host arithmetic --------------------------------------------------
def test_window_crops_of_a_picture():
    import dct_amd
    wc = dct_amd._window_crops
    s420 = [(2, 80, 1056), (2, 40, 528), (2, 40, 528)]
    crops = [(10, 6), (0, 0), (0, 0)]                      # the true picture is 70 x 1050
    w, ws, c = wc(s420, crops, True, ((16, 38), (32, 122)), (1, 2))
    assert w == [((1, 2), (16, 48), (32, 128)), ((1, 2), (8, 24), (16, 64)), ((1, 2), (8, 24), (16, 64))]
    assert ws == [(1, 32, 96), (1, 16, 48), (1, 16, 48)] and c == [(10, 6), (0, 0), (0, 0)]
    w, ws, c = wc(s420, crops, True, ((48, 70), (1040, 1050)), None)   # to the true bottom-right corner
    assert w[0] == ((0, 2), (48, 80), (1040, 1056)) and c == crops
    w, ws, c = wc(s420, crops, True, None, (0, 1))                     # frames only: the container's own crops
    assert ws == [(1, 80, 1056), (1, 40, 528), (1, 40, 528)] and c == crops
    w, ws, c = wc(s420, crops, True, ((0, 64), (16, 48)), None)        # ends on multiples of 16: no crop
    assert c == [(0, 0)] * 3 and ws[0] == (2, 64, 32)
    w, ws, c = wc(s420, crops, True, ((0, 1), (0, 1)), None)           # the largest crop there is
    assert c == [(15, 15), (0, 0), (0, 0)] and ws == [(2, 16, 16), (2, 8, 8), (2, 8, 8)]
    s444 = [(1, 40, 136)] * 3
    w, ws, c = wc(s444, None, True, ((8, 17), (24, 33)), None)         # 4:4:4: m is 8
    assert w == [((0, 1), (8, 24), (24, 40))] * 3 and c == [(7, 7), (0, 0), (0, 0)]
    # a start that is not a multiple of m is refused: 8 is not enough in 4:2:0
    for region in (((8, 38), (32, 122)), ((16, 38), (8, 122)), ((3, 38), (32, 122)), ((16, 38), (33, 122))):
        with pytest.raises(dct_amd.DctqError, match="start"):
            wc(s420, crops, True, region, None)
    with pytest.raises(dct_amd.DctqError, match="start"):
        wc(s444, None, True, ((4, 17), (24, 33)), None)
    for region, frames in ((((0, 71), (0, 8)), None), (((16, 16), (0, 8)), None), (None, (0, 3)), (None, (1, 1))):
        with pytest.raises(dct_amd.DctqError):                         # decompress's own refusals
            wc(s420, crops, True, region, frames)


def test_window_crops_of_plain_planes():
    import dct_amd
    wc = dct_amd._window_crops
    shapes, crops = [(2, 32, 1056), (2, 32, 104)], [(0, 0), (5, 4)]    # true sizes 32 x 1056 and 27 x 100
    w, ws, c = wc(shapes, crops, False, [((8, 30), (96, 1001)), ((0, 27), (88, 100))], (1, 2))
    assert w == [((1, 2), (8, 32), (96, 1008)), ((1, 2), (0, 32), (88, 104))]
    assert ws == [(1, 24, 912), (1, 32, 16)] and c == [(2, 7), (5, 4)]
    with pytest.raises(dct_amd.DctqError, match="start"):
        wc(shapes, crops, False, [((8, 30), (96, 1001)), ((0, 27), (93, 100))], None)
    same = [(3, 48, 208), (2, 48, 208)]
    w, ws, c = wc(same, None, False, ((40, 48), (0, 208)), None)        # no crop at all: frame v1
    assert ws == [(2, 8, 208)] * 2 and c == [(0, 0)] * 2
    # every crop frame_window can compute is one frame c1 takes, and none gives frame v1
    for crops_ in ([(7, 7), (0, 3)], [(0, 0), (0, 0)]):
        data, off = bits_ref.pack([[(1, 0)]] * 4)
        buf = frame_ref.pack(data, off, [(1, 8, 16), (1, 8, 16)], 50, crops=crops_)
        assert (buf[:8] == frame_ref.MAGIC) == (not any(map(any, crops_)))
        assert frame_ref.parse(buf)["crops"] == (crops_ if any(map(any, crops_)) else None)


def test_frame_window_refuses_a_start_before_anything_is_launched(monkeypatch):
    """The header is all frame_window reads before it refuses: no offsets are rebuilt."""
    import dct_amd
    h = {"shapes": [(2, 32, 64)], "crops": None, "colour": False}
    monkeypatch.setattr(dct_amd, "_frame_open", lambda buf, stream: (buf, h))
    monkeypatch.setattr(dct_amd, "_frame_parts", lambda *a: pytest.fail("launched"))
    with pytest.raises(dct_amd.DctqError, match="start"):
        dct_amd.frame_window(b"", region=((4, 32), (0, 64)))


# ---- extract_ref against independent statements ---------------------------------------------------------
def stream(shapes, seed):
    """A stream built block by block: per block its (value, run) symbols, bytes and coefficients."""
    rng = np.random.default_rng(seed)
    n = sum(f * (h // 8) * (w // 8) for f, h, w in shapes)
    blocks = []
    for b in range(n):
        k = int(rng.integers(0, 7))
        blocks.append([(int(rng.integers(-300, 300)) or 1, int(rng.integers(0, 6))) for _ in range(k)])
    each = [bits_ref.pack([s])[0] for s in blocks]
    data, off = bits_ref.pack(blocks)
    return blocks, each, data, off


SHAPES = [(3, 16, 40), (2, 8, 24), (2, 8, 24)]
WINDOWS = {
    "whole": [((0, f), (0, h), (0, w)) for f, h, w in SHAPES],
    "frames": [((1, 3), (0, 16), (0, 40)), ((0, 1), (0, 8), (0, 24)), ((1, 2), (0, 8), (0, 24))],
    "region": [((0, 3), (8, 16), (8, 32)), ((0, 2), (0, 8), (16, 24)), ((1, 2), (0, 8), (0, 8))],
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_window_stream_is_the_blocks_in_window_order(name):
    blocks, each, data, off = stream(SHAPES, 7)
    windows = WINDOWS[name]
    nbs = [f * (h // 8) * (w // 8) for f, h, w in SHAPES]
    var = [np.arange(1000 * k, 1000 * k + nb, dtype=np.int32) for k, nb in enumerate(nbs)]
    out, new, wvar = extract_ref.window_stream(data, off, SHAPES, windows, var)
    order = [b.reshape(-1) for b in window_ref.blocks(SHAPES, windows)]
    flat = np.concatenate(order)
    want = np.concatenate([each[s] for s in flat] + [np.zeros(0, np.uint8)])
    assert out.dtype == np.uint8 and np.array_equal(out, want)
    assert new.dtype == np.uint32 and new[0] == 0 and new[-1] == len(want) <= len(data)
    assert np.array_equal(np.diff(new.astype(np.int64)), [len(each[s]) for s in flat])
    # decoding the window's stream gives the selected blocks' coefficients
    coef = bits_ref.unpack(data, off)
    assert np.array_equal(bits_ref.unpack(out, new), coef[flat])
    first = np.concatenate([[0], np.cumsum(nbs)])
    for k, o in enumerate(order):
        assert wvar[k].dtype == np.int32 and np.array_equal(wvar[k], 1000 * k + (o - first[k]))
    if name == "whole":
        assert np.array_equal(out, data) and np.array_equal(new, off)
    assert extract_ref.window_stream(data, off, SHAPES, windows)[2] is None


def test_window_stream_takes_any_bytes_and_exact_lengths():
    """Foreign offsets: lengths above 368 are copied whole (no clamp), zero lengths give nothing."""
    shapes, windows = [(1, 8, 32)], [((0, 1), (0, 8), (8, 32))]
    off = np.array([0, 5, 5, 605, 606], np.uint32)
    data = (np.arange(700) % 251).astype(np.uint8)
    out, new, _ = extract_ref.window_stream(data, off, shapes, windows)
    assert new.tolist() == [0, 0, 600, 601] and np.array_equal(out, data[5:606])
    assert extract_ref.run_alignments(off, shapes, windows) == {(1, 0)}
    assert extract_ref.run_alignments(off, shapes, windows, src_base=2, dst_base=3) == {(3, 3)}
    with pytest.raises(ValueError):
        extract_ref.window_stream(data[:600], off, shapes, windows)
    with pytest.raises(ValueError):
        extract_ref.window_stream(data, off[::-1].copy(), shapes, windows)


def container(length_bytes, adaptive=False, colour=False):
    """A hand-built container: three frames, every block its own bytes; length_bytes 2 through one
    block of 300 bytes in frame 2 (so a window of frames 0..2 fits one byte a length)."""
    shapes = [(3, 16, 32), (3, 8, 16), (3, 8, 16)] if colour else [(3, 16, 24), (3, 8, 40)]
    n = sum(f * (h // 8) * (w // 8) for f, h, w in shapes)
    rng = np.random.default_rng(length_bytes)
    ln = rng.integers(1, 40, n)
    if length_bytes == 2:
        ln[(shapes[0][1] // 8) * (shapes[0][2] // 8) * 2 + 1] = 300
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    data = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    var = rng.integers(0, 1 << 20, n).astype(np.int32) if adaptive else None
    crops = [(9, 3), (0, 0), (0, 0)] if colour else [(0, 5), (2, 0)]
    buf = frame_ref.pack(data, off, shapes, 77, adaptive, var, colour, crops=crops)
    assert frame_ref.parse(buf)["length_bytes"] == length_bytes
    return buf


@pytest.mark.parametrize("length_bytes", [1, 2])
@pytest.mark.parametrize("adaptive,colour", [(False, False), (True, False), (True, True)])
def test_split_then_concat_is_the_identity(length_bytes, adaptive, colour):
    buf = container(length_bytes, adaptive, colour)
    whole = frame_ref.parse(buf)
    for a in (1, 2):
        parts = [extract_ref.frame_window(buf, frames=(0, a)), extract_ref.frame_window(buf, frames=(a, 3))]
        ps = [frame_ref.parse(p) for p in parts]                       # every reader check passes
        assert [p["shapes"][0][0] for p in ps] == [a, 3 - a]
        for p in ps:
            assert (p["quality"], p["adaptive"], p["colour"], p["crops"]) == (77, adaptive, colour, whole["crops"])
        # length_bytes is the window's own: the 300-byte block is in frame 2
        assert [p["length_bytes"] for p in ps] == [1, length_bytes]
        assert extract_ref.frame_concat(parts) == buf
    three = [extract_ref.frame_window(buf, frames=(f, f + 1)) for f in range(3)]
    assert extract_ref.frame_concat(three) == buf
    assert extract_ref.frame_window(buf) == buf


def test_frame_window_of_a_region_parses_and_holds_the_blocks():
    buf = container(2, adaptive=True, colour=True)                     # stored 16 x 32, true 7 x 29, 4:2:0
    whole = frame_ref.parse(buf)
    out = frame_ref.parse(extract_ref.frame_window(buf, region=((0, 5), (16, 29)), frames=(1, 3)))
    assert out["shapes"] == [(2, 16, 16), (2, 8, 8), (2, 8, 8)] and out["crops"] == [(11, 3), (0, 0), (0, 0)]
    windows = [((1, 3), (0, 16), (16, 32)), ((1, 3), (0, 8), (8, 16)), ((1, 3), (0, 8), (8, 16))]
    flat = np.concatenate([b.reshape(-1) for b in window_ref.blocks(whole["shapes"], windows)])
    off = whole["offsets"].astype(np.int64)
    assert out["payload"] == b"".join(whole["payload"][off[s]:off[s + 1]] for s in flat)
    assert np.array_equal(out["var_nums"], whole["var_nums"][flat])
    for bad in (dict(region=((0, 5), (8, 29))), dict(region=((0, 8), (0, 30))), dict(frames=(2, 4))):
        with pytest.raises(ValueError):
            extract_ref.frame_window(buf, **bad)
    # plain planes carry a crop each; a window with no crop at all is frame v1
    c1 = extract_ref.frame_window(container(1), region=[((0, 16), (8, 16)), ((0, 6), (8, 33))])
    assert c1[:8] == frame_ref.MAGIC_CROP and frame_ref.parse(c1)["crops"] == [(0, 0), (2, 7)]
    plain = frame_ref.pack(*bits_ref.pack([[(1, 0)]] * 8), [(2, 16, 16)], 50)
    cut = extract_ref.frame_window(plain, region=((8, 16), (0, 16)), frames=(1, 2))
    assert cut[:8] == frame_ref.MAGIC and frame_ref.parse(cut)["shapes"] == [(1, 8, 16)]


def test_frame_concat_refuses_disagreement():
    data, off = bits_ref.pack([[(1, 0)]] * 4)
    base = dict(shapes=[(1, 8, 16), (1, 8, 16)], quality=50)
    a = frame_ref.pack(data, off, **base)
    var = np.zeros(4, np.int32)
    for other in (frame_ref.pack(data, off, [(1, 8, 16), (1, 8, 16)], 51),
                  frame_ref.pack(data, off, [(1, 8, 16), (1, 8, 16)], 50, True, var),
                  frame_ref.pack(data, off, [(1, 16, 8), (1, 8, 16)], 50),
                  frame_ref.pack(data, off, [(1, 8, 32)], 50),
                  frame_ref.pack(data, off, [(1, 8, 16), (1, 8, 16)], 50, crops=[(0, 1), (0, 0)])):
        with pytest.raises(ValueError):
            extract_ref.frame_concat([a, other])
    with pytest.raises(ValueError):
        extract_ref.frame_concat([a])
    assert frame_ref.parse(extract_ref.frame_concat([a, a, a]))["shapes"] == [(3, 8, 16), (3, 8, 16)]
