"""CPU: the bit-packed coefficient stream "bits v1" is declared, exported, bound and hosted;
its kernels are in the product code object and the pinned decoder instantiations are
unchanged; the ABI revision is unchanged; and the format's plain-Python statement
(tools/bits_ref.py, the GPU tests' yardstick) is checked by itself against the oracle's
run-length coder and against byte totals worked out by hand.  No compute is attempted
without a GPU."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bits_ref  # noqa: E402

NAMES = ["dctq_bits_workspace_bytes", "dctq_bits_pack", "dctq_bits_decode", "dctq_decode_bits_planes"]


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
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    want = {
        "dctq_bits_workspace_bytes": ([ll], C.c_size_t),
        "dctq_bits_pack": ([vp, i, vp, ll, vp, vp, ll, vp, vp], i),
        "dctq_bits_decode": ([vp, vp, ll, vp, vp], i),
        "dctq_decode_bits_planes": ([vp, vp, vp, vp, C.POINTER(dct_amd._Plane), i, vp], i),
    }
    for name, (args, res) in want.items():
        fn = getattr(dct_amd.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert callable(dct_amd.bits_pack) and callable(dct_amd.bits_decode)
    assert callable(dct_amd.Plan.decode_bits) and callable(dct_amd.Plan.encode_bits_planes)
    assert lib.dctq_bits_workspace_bytes(1) > 0
    assert lib.dctq_bits_workspace_bytes(1 << 20) >= 4 * (1 << 14)  # one total per 64-block tile


def test_abi_version_unchanged(lib):
    assert lib.dctq_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_header_compiles_as_c99_with_bits(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){\n"
                   " size_t (*w)(long long) = dctq_bits_workspace_bytes;\n"
                   " int (*p)(const void *, int, const uint32_t *, long long, uint32_t *, uint8_t *, long long,\n"
                   "          void *, void *) = dctq_bits_pack;\n"
                   " int (*d)(const uint8_t *, const uint32_t *, long long, int16_t *, void *) = dctq_bits_decode;\n"
                   " int (*f)(const dctq_plan *, const uint8_t *, const uint32_t *, const int32_t *const *,\n"
                   "          const dctq_plane *, int, void *) = dctq_decode_bits_planes;\n"
                   " (void)w; (void)p; (void)d; (void)f; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_frame_bits_host_builds(lib):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_bits"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert os.access(os.path.join(ROOT, "host", "frame_bits"), os.X_OK)
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    clean = mk[mk.index("clean:"):]
    assert "frame_bits" in all_line.split() and "frame_bits" in clean.split()


def test_kernels_in_product_code_object(lib, tmp_path):
    """bits_count_kernel<W> and bits_emit_kernel<W> for W in {2, 4}, bits_to_coef, and
    bits_to_pixels<ADAPTIVE, INV32> for fp64, fp32 and fp64 adaptive; the instantiations of
    decode8, symbols_to_pixels and distortion8 are what they were."""
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

    def inst(key, n):
        return {k[k.index(key):][:len(key) + n] for k in names if key in k}

    assert inst("bits_count_kernel", 7) == {f"bits_count_kernelILi{w}EEE" for w in (2, 4)}, names
    assert inst("bits_emit_kernel", 7) == {f"bits_emit_kernelILi{w}EEE" for w in (2, 4)}, names
    assert any("bits_to_coef" in k for k in names), names
    assert inst("bits_to_pixels", 11) == {f"bits_to_pixelsILb{a}ELb{f}EEE" for a, f in ((0, 0), (0, 1), (1, 0))}, names
    key = "symbols_to_pixels"
    assert inst(key, 15) == {key + f"ILi{w}ELb{a}ELb{f}EEE" for w in (2, 4) for a, f in ((0, 0), (0, 1), (1, 0))}, names
    assert inst("decode8", 11) == {"decode8ILb0ELb0EEE", "decode8ILb0ELb1EEE", "decode8ILb1ELb0EEE"}, names
    assert inst("distortion8", 11) == {"distortion8ILb0ELb0EEE", "distortion8ILb0ELb1EEE", "distortion8ILb1ELb0EEE"}, names


# ---- the reference packer by itself ---------------------------------------------------------------------
W, H = 64, 64


@functools.lru_cache(maxsize=None)
def oracle_blocks(kind, q):
    """The oracle's forward, quantize and RLE of a 64x64 synthetic plane: per block [(value, run)]."""
    import oracle as O
    coef = O.forward_plane(O.synth_plane(31, O.KINDS[kind], W, H), q, 0)
    out = []
    for c in coef:
        v, r = O.rle_encode(c.reshape(8, 8))
        out.append([(int(a), int(b)) for a, b in zip(v, r)])
    return coef, out


@pytest.mark.parametrize("q", [10, 50, 90, 100])
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_reference_round_trip_on_oracle_symbols(kind, q):
    import oracle as O
    coef, blocks = oracle_blocks(kind, q)
    data, off = bits_ref.pack(blocks)
    got = bits_ref.unpack(data, off)
    for b, sym in enumerate(blocks):
        want = O.rle_decode([v for v, _ in sym], [r for _, r in sym]).ravel()
        assert np.array_equal(got[b], want), (kind, q, b)
    assert np.array_equal(got, coef)  # and RLE itself is lossless


def test_reference_hand_cases():
    import oracle as O
    cases = [[(0, 64)], [(32767, 0)], [(-32767, 0)], [(-32768, 0)], [(9, 63)],
             [(32767, 0), (-32768, 61), (-32767, 0)], [(1, 0)] * 64]
    data, off = bits_ref.pack(cases)
    got = bits_ref.unpack(data, off)
    for b, sym in enumerate(cases):
        want = O.rle_decode([v for v, _ in sym], [r for _, r in sym]).ravel()
        assert np.array_equal(got[b], want), sym
    assert got[3, 0] == -32768 and got[4, 63] == 9 and not got[0].any()
    # more than 64 symbols: the first 64 are written; a clamped run lands past the block either way
    long = [(1, 0)] * 64 + [(5, 0)] * 6
    assert np.array_equal(*[bits_ref.unpack(*bits_ref.pack([s]))[0] for s in (long, long[:64])])
    assert np.array_equal(*[bits_ref.unpack(*bits_ref.pack([s]))[0] for s in ([(4, 3), (7, 70000)], [(4, 3), (7, 64)])])
    # bad codes end a block; anything decodes
    assert not bits_ref.unpack(np.zeros(8, np.uint8), [0, 8]).any()
    assert not bits_ref.unpack(np.zeros(0, np.uint8), [0, 0]).any()
    assert bits_ref.unpack(np.full(16, 0xFF, np.uint8), [0, 16])[0].tolist().count(0) == 64  # (0, 0) x 64


def test_reference_byte_totals_by_hand():
    """ue(k) takes 2n - 1 bits, n the bit length of k + 1.
    Block A = (5, 0), (-3, 2), (0, 60):
      (5, 0):  ue(0) = '1' (1 bit);        m = 9:  x = 10 = 1010b,  n = 4 -> 7 bits   ->  8
      (-3, 2): ue(2): x = 3, n = 2 (3);    m = 6:  x = 7,  n = 3 -> 5 bits            ->  8
      (0, 60): ue(60): x = 61, n = 6 (11); m = 0:  1 bit                              -> 12
      28 bits -> 4 bytes: 1 0001010 | 011 00111 | 00000111 101 1 0000
    Block B = (0, 64): ue(64): x = 65, n = 7 (13 bits); ue(0): 1 bit -> 14 bits -> 2 bytes:
      0000001000001 1 00
    Block C = (-32768, 64) x 64: 13 + 33 bits each -> 64 * 46 / 8 = 368 bytes, the worst case."""
    a = [(5, 0), (-3, 2), (0, 60)]
    data, off = bits_ref.pack([a, [(0, 64)], [(-32768, 64)] * 64])
    assert off.tolist() == [0, 4, 6, 374]
    assert data[:6].tolist() == [0b10001010, 0b01100111, 0b00000111, 0b10110000, 0b00000010, 0b00001100]
    assert bits_ref.ue(0) == "1" and bits_ref.ue(1) == "010" and bits_ref.ue(64) == "0000001000001"
    assert len(bits_ref.symbol_bits(-32768, 64)) == 46 and len(bits_ref.symbol_bits(-32768, 99999)) == 46


# ---- size ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_packed_stream_is_smaller_than_two_byte_symbols(kind, q):
    _, blocks = oracle_blocks(kind, q)
    _, off = bits_ref.pack(blocks)
    nsym = sum(len(b) for b in blocks)
    print(f"{kind} q{q}: {int(off[-1]) / len(blocks):.1f} packed B/block, {2 * nsym / len(blocks):.1f} B/block in 2-byte symbols")
    assert int(off[-1]) < 2 * nsym, (kind, q, int(off[-1]), 2 * nsym)
