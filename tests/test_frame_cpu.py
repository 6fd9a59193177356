"""CPU: the container "frame v1" and the two conversions it rests on are declared, exported and
bound; their kernels are in the product code object; the ABI revision is unchanged; and the
format's plain-Python statement (tools/frame_ref.py, the GPU tests' yardstick) is checked by
itself: a container worked out by hand, round trips, the length clamp, every refusal, and the
size against the offsets it replaces.  No compute is attempted without a GPU."""
import ctypes as C
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bits_ref  # noqa: E402
import frame_ref  # noqa: E402

NAMES = ["dctq_block_lengths", "dctq_block_offsets_workspace_bytes", "dctq_block_offsets"]


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
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "DCTQFRM1" in hdr and "frame v1" in hdr


def test_exported_from_both_libraries(lib):
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", name)],
                             capture_output=True, text=True).stdout
        got = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(NAMES) <= got, (name, set(NAMES) - got)


def test_bound(lib):
    import dct_amd
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    want = {
        "dctq_block_lengths": ([vp, ll, i, vp, vp, vp], i),
        "dctq_block_offsets_workspace_bytes": ([ll], C.c_size_t),
        "dctq_block_offsets": ([vp, i, ll, vp, vp, vp], i),
    }
    for name, (args, res) in want.items():
        fn = getattr(dct_amd.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for name in ("block_lengths", "block_offsets", "frame_pack", "frame_unpack", "compress", "decompress"):
        assert callable(getattr(dct_amd, name)), name
    assert lib.dctq_block_offsets_workspace_bytes(1) > 0
    assert lib.dctq_block_offsets_workspace_bytes(1 << 20) >= 4 * (1 << 14)  # one total per 64-block tile


def test_abi_version_unchanged(lib):
    assert lib.dctq_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_header_compiles_as_c99_with_frame(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " int (*l)(const uint32_t *, long long, int, void *, uint32_t *, void *) = dctq_block_lengths;\n"
                   " size_t (*w)(long long) = dctq_block_offsets_workspace_bytes;\n"
                   " int (*o)(const void *, int, long long, uint32_t *, void *, void *) = dctq_block_offsets;\n"
                   " (void)l; (void)w; (void)o; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_kernels_in_product_code_object(lib, tmp_path):
    """block_lengths_kernel<W> and block_offsets_kernel<W> for W in {1, 2}."""
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
    for key in ("block_lengths_kernel", "block_offsets_kernel"):
        got = {k[k.index(key):][:len(key) + 7] for k in names if key in k}
        assert got == {f"{key}ILi{w}EEE" for w in (1, 2)}, names


def test_source_is_listed_and_has_no_knobs():
    import re
    from dct_amd.build import SOURCES
    assert "frame.hip" in SOURCES
    src = open(os.path.join(ROOT, "dct_amd", "csrc", "frame.hip")).read()
    assert "getenv" not in src
    assert not re.findall(r"^#\s*(?:ifndef|ifdef|if|elif)\b.*DCTQ_\w+", src, flags=re.M)


# ---- the reference container by itself ------------------------------------------------------------------
A = [(5, 0), (-3, 2), (0, 60)]   # 4 bytes (tests/test_bits_cpu.py test_reference_byte_totals_by_hand)
B = [(0, 64)]                    # 2 bytes


def hand_container():
    data, off = bits_ref.pack([A, B])
    assert off.tolist() == [0, 4, 6]
    return frame_ref.pack(data, off, [(8, 16)], 50), data


def test_container_by_hand():
    """One plain 16x8 plane (two blocks) at q50: 64 B of header, 2 B of lengths, 14 B of padding,
    6 B of payload."""
    buf, data = hand_container()
    want = (b"DCTQFRM1"
            + bytes([64, 0, 0, 0])                       # header_bytes = 48 + 16
            + bytes([50, 0, 1, 1, 0])                    # quality, adaptive, nplanes, length_bytes, colour
            + bytes(7)                                   # reserved
            + bytes([2, 0, 0, 0, 0, 0, 0, 0])            # nblocks
            + bytes([6, 0, 0, 0, 0, 0, 0, 0])            # payload_bytes
            + bytes([86, 0, 0, 0, 0, 0, 0, 0])           # total_bytes
            + bytes([16, 0, 0, 0, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0])  # width, height, nframes, 0
            + bytes([4, 2]) + bytes(14)                  # lengths, padding to 80
            + bytes([0b10001010, 0b01100111, 0b00000111, 0b10110000, 0b00000010, 0b00001100]))
    assert len(want) == 86 and buf == want
    p = frame_ref.parse(buf)
    assert (p["quality"], p["adaptive"], p["colour"], p["length_bytes"], p["nblocks"]) == (50, False, False, 1, 2)
    assert p["shapes"] == [(1, 8, 16)] and p["offsets"].tolist() == [0, 4, 6] and p["payload"] == bytes(data)
    assert p["var_nums"] is None
    assert frame_ref.parse(buf + b"trailing bytes are not the container's")["payload"] == bytes(data)


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("length_bytes", [1, 2])
@pytest.mark.parametrize("adaptive", [False, True])
def test_parse_of_pack_is_identity(adaptive, length_bytes, colour):
    rng = np.random.default_rng(7 + 4 * adaptive + 2 * length_bytes + colour)
    shapes = [(2, 16, 32), (2, 8, 16), (2, 8, 16)] if colour else [(1, 8, 24), (3, 16, 8)]
    n = sum(f * (h // 8) * (w // 8) for f, h, w in shapes)
    ln = rng.integers(0, 256 if length_bytes == 1 else 369, n)
    if length_bytes == 2:
        ln[n // 2] = 368
    off = frame_ref.offsets_from_lengths(ln)
    payload = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    vn = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32) if adaptive else None
    buf = frame_ref.pack(payload, off, shapes, 77, adaptive, vn, colour, length_bytes=length_bytes)
    p = frame_ref.parse(buf)
    assert (p["quality"], p["adaptive"], p["colour"], p["length_bytes"]) == (77, adaptive, colour, length_bytes)
    assert p["shapes"] == shapes and p["nblocks"] == n
    assert np.array_equal(p["lengths"], ln) and np.array_equal(p["offsets"], off)
    assert p["payload"] == payload.tobytes()
    assert (p["var_nums"] is None) if not adaptive else np.array_equal(p["var_nums"], vn)
    hb = 48 + 16 * len(shapes)
    assert struct.unpack_from("<Q", buf, 40)[0] == len(buf)
    end = hb + n * length_bytes  # the lengths section starts right after the header; its padding is 0
    assert not any(buf[end:frame_ref.align16(end)])


def test_offsets_from_lengths_clamps():
    ln = np.array([0, 1, 368, 369, 1000, 65535, 255], np.int64)
    assert frame_ref.offsets_from_lengths(ln).tolist() == [0, 0, 1, 369, 737, 1105, 1473, 1728]
    every = frame_ref.offsets_from_lengths(np.arange(369, 65536))
    assert int(every[-1]) == 368 * (65536 - 369)
    assert np.array_equal(frame_ref.lengths_from_offsets(frame_ref.offsets_from_lengths(np.arange(369))), np.arange(369))
    # differences are taken mod 2^32: a decreasing pair is a huge length
    assert frame_ref.lengths_from_offsets(np.array([0, 8, 4], np.uint32)).tolist() == [8, 2 ** 32 - 4]


def test_pack_refuses_what_it_cannot_state():
    data, off = bits_ref.pack([A, B])
    for bad in (dict(shapes=[(8, 12)]), dict(shapes=[(8, 16)], quality=0), dict(shapes=[(8, 16)], adaptive=True),
                dict(shapes=[(8, 16)], colour=True), dict(shapes=[(8, 24)])):
        kw = dict(quality=50)
        kw.update(bad)
        with pytest.raises(frame_ref.FrameError):
            frame_ref.pack(data, off, **kw)
    big, boff = bits_ref.pack([[(-32768, 64)] * 64, B])
    with pytest.raises(frame_ref.FrameError):
        frame_ref.pack(big, boff, [(8, 16)], 50, length_bytes=1)
    assert frame_ref.parse(frame_ref.pack(big, boff, [(8, 16)], 50))["length_bytes"] == 2


def test_every_refusal():
    buf, _ = hand_container()
    cases = frame_ref.refusal_cases(buf)
    assert len(cases) >= 12
    for rule, bad in cases:
        with pytest.raises(frame_ref.FrameError):
            frame_ref.parse(bad)
            pytest.fail(rule)
    # colour says Y, Cb, Cr: three planes, chroma of 4:4:4 or 4:2:0
    n = 2 * 2 + 1 + 1
    off = frame_ref.offsets_from_lengths(np.ones(n, np.int64))
    ok = frame_ref.pack(bytes(n), off, [(16, 16), (8, 8), (8, 8)], 50, colour=True)
    assert frame_ref.parse(ok)["colour"]
    off = frame_ref.offsets_from_lengths(np.ones(n + 1, np.int64))
    bad = bytearray(frame_ref.pack(bytes(n + 1), off, [(16, 16), (8, 16), (8, 8)], 50))  # Cb is not Cr
    assert frame_ref.parse(bytes(bad))["shapes"] == [(1, 16, 16), (1, 8, 16), (1, 8, 8)]
    bad[16] = 1
    with pytest.raises(frame_ref.FrameError):
        frame_ref.parse(bytes(bad))


# ---- size ---------------------------------------------------------------------------------------------------
W, H = 64, 64


@functools.lru_cache(maxsize=None)
def oracle_stream(kind, q):
    """bits_ref.pack of the oracle's forward, quantize and RLE of a 64x64 synthetic plane."""
    import oracle as O
    coef = O.forward_plane(O.synth_plane(31, O.KINDS[kind], W, H), q, 0)
    blocks = []
    for c in coef:
        v, r = O.rle_encode(c.reshape(8, 8))
        blocks.append([(int(a), int(b)) for a, b in zip(v, r)])
    return bits_ref.pack(blocks)


@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_container_is_smaller_than_stream_plus_offsets(kind):
    data, off = oracle_stream(kind, 50)
    n = len(off) - 1
    buf = frame_ref.pack(data, off, [(H, W)], 50)
    loose = len(data) + 4 * (n + 1)
    print(f"{kind} q50: container {len(buf) / n:.2f} B/block, payload + uint32 offsets {loose / n:.2f} B/block "
          f"(payload {len(data) / n:.2f})")
    assert len(buf) < loose, (kind, len(buf), loose)
    p = frame_ref.parse(buf)
    assert p["payload"] == bytes(data) and np.array_equal(p["offsets"], off)
