"""CPU: the pixel decoder (dctq_decode_planes) is declared, exported, bound and
hosted; the ABI revision is unchanged.  No compute is attempted without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dct_amd.build import build
    build()
    import dct_amd
    return dct_amd.lib()


def test_decode_planes_declared_in_header():
    from dct_amd.build import declared_functions, public_headers
    assert "dctq_decode_planes" in declared_functions([os.path.join(ROOT, "include", "dct_amd.h")])
    assert "dctq_decode_planes" in declared_functions(public_headers())


def test_decode_planes_exported(lib):
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "dct_amd", name)],
                             capture_output=True, text=True).stdout
        assert any(l.split()[-1] == "dctq_decode_planes" and " T " in l for l in out.splitlines()), name


def test_decode_planes_bound(lib):
    import ctypes as C

    import dct_amd
    fn = dct_amd.lib().dctq_decode_planes
    assert fn.restype is C.c_int and len(fn.argtypes) == 6
    assert fn.argtypes[3] == C.POINTER(dct_amd._Plane)
    assert callable(dct_amd.Plan.decode_planes) and callable(dct_amd.Plan.decode)


def test_abi_version_unchanged(lib):
    assert lib.dctq_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_frame_decode_host_builds(lib):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_decode"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert os.access(os.path.join(ROOT, "host", "frame_decode"), os.X_OK)
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    clean = mk[mk.index("clean:"):]
    assert "frame_decode" in all_line.split() and "frame_decode" in clean.split()


def test_header_compiles_as_c99_with_decoder(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){ int (*f)(const dctq_plan *, const int16_t *const *, const int32_t *const *,\n"
                   "                         const dctq_plane *, int, void *) = dctq_decode_planes; (void)f; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_decode_kernels_in_product_code_object(lib, tmp_path):
    """Three instantiations: fp64 non-adaptive, fp32 (plans the bound admits), fp64 adaptive."""
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
        names |= {w for w in out.split() if w.startswith("_Z") and "." not in w and "decode8" in w}
    inst = {n[n.index("decode8"):][:18] for n in names}
    assert inst == {"decode8ILb0ELb0EEE", "decode8ILb0ELb1EEE", "decode8ILb1ELb0EEE"}, names
