"""CPU: the fused symbol decoder (dctq_decode_symbols_planes) is declared, exported,
bound and hosted; its six kernels are in the product code object beside the three of
decode8; the ABI revision is unchanged.  No compute is attempted without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dctq_decode_symbols_planes"


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


def test_declared_in_header():
    from dct_amd.build import declared_functions, public_headers
    assert NAME in declared_functions([os.path.join(ROOT, "include", "dct_amd.h")])
    assert NAME in declared_functions(public_headers())


def test_exported_from_both_libraries(lib):
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", name)],
                             capture_output=True, text=True).stdout
        assert any(l.split()[-1] == NAME and " T " in l for l in out.splitlines()), name


def test_bound(lib):
    import ctypes as C

    import dct_amd
    fn = getattr(dct_amd.lib(), NAME)
    vp, i = C.c_void_p, C.c_int
    assert fn.restype is i
    assert list(fn.argtypes) == [vp, vp, i, vp, vp, C.POINTER(dct_amd._Plane), i, vp]
    assert callable(dct_amd.Plan.decode_symbols)


def test_abi_version_unchanged(lib):
    assert lib.dctq_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_symbols_decode_host_builds(lib):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "symbols_decode"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert os.access(os.path.join(ROOT, "host", "symbols_decode"), os.X_OK)
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    clean = mk[mk.index("clean:"):]
    assert "symbols_decode" in all_line.split() and "symbols_decode" in clean.split()


def test_header_compiles_as_c99_with_symbol_decoder(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){ int (*f)(const dctq_plan *, const void *, int, const uint32_t *,\n"
                   "                         const int32_t *const *, const dctq_plane *, int, void *)\n"
                   "                    = dctq_decode_symbols_planes; (void)f; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_kernels_in_product_code_object(lib, tmp_path):
    """Six instantiations of symbols_to_pixels<W, ADAPTIVE, INV32>: W in {2, 4} x (fp64
    non-adaptive, fp32, fp64 adaptive); and still exactly the three of decode8."""
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
    key = "symbols_to_pixels"
    fused = {n[n.index(key):][:len(key) + 15] for n in names if key in n}
    assert fused == {key + f"ILi{w}ELb{a}ELb{f}EEE" for w in (2, 4) for a, f in ((0, 0), (0, 1), (1, 0))}, names
    dec = {n[n.index("decode8"):][:18] for n in names if "decode8" in n}
    assert dec == {"decode8ILb0ELb0EEE", "decode8ILb0ELb1EEE", "decode8ILb1ELb0EEE"}, names
    assert not [n for n in names if key in n and "decode8" in n]
