"""CPU: the per-block distortion (dctq_distortion_planes) is declared, exported, bound and
hosted; its three kernels are in the product code object; the ABI revision is unchanged.
No compute is attempted without a GPU."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dctq_distortion_planes"


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
    assert list(fn.argtypes) == [vp, C.POINTER(dct_amd._Plane), i, vp, vp]
    assert callable(dct_amd.Plan.distortion_planes)
    assert callable(dct_amd.Plan.rate_distortion_planes)
    assert callable(dct_amd.psnr_u8)


def test_psnr_u8():
    import dct_amd
    assert dct_amd.psnr_u8(0, 64) == math.inf
    assert abs(dct_amd.psnr_u8(64, 64) - 10.0 * math.log10(65025.0)) <= 1e-12
    # the worst block (64 * 255^2) is 0 dB; a tensor-like sum (anything float() takes) is accepted
    assert abs(dct_amd.psnr_u8(64 * 255 * 255, 64)) <= 1e-12
    import numpy as np
    assert abs(dct_amd.psnr_u8(np.int64(640), np.int64(6400)) - 10.0 * math.log10(650250.0)) <= 1e-12


def test_abi_version_unchanged(lib):
    assert lib.dctq_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "dct_amd.h")).read()
    assert "#define DCTQ_ABI_VERSION 6" in hdr


def test_frame_rd_host_builds(lib):
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "frame_rd"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert os.access(os.path.join(ROOT, "host", "frame_rd"), os.X_OK)
    mk = open(os.path.join(ROOT, "host", "Makefile")).read()
    all_line = next(l for l in mk.splitlines() if l.startswith("all:"))
    clean = mk[mk.index("clean:"):]
    assert "frame_rd" in all_line.split() and "frame_rd" in clean.split()


def test_header_compiles_as_c99_with_distortion(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "dct_amd.h"\n'
                   "int main(void){ int (*f)(const dctq_plan *, const dctq_plane *, int, uint32_t *, void *)\n"
                   "                    = dctq_distortion_planes; (void)f; return 0; }\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                          "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def _device_kernels(path, tmp):
    import glob
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    os.makedirs(tmp, exist_ok=True)
    local = os.path.join(tmp, os.path.basename(path))
    shutil.copy(path, local)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", local], cwd=tmp, check=True,
                   capture_output=True)
    names = set()
    objs = glob.glob(local + ".*gfx950")
    assert objs, os.listdir(tmp)
    for obj in objs:
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--symbols", obj], capture_output=True,
                             text=True).stdout
        names |= {w for w in out.split() if w.startswith("_Z") and "." not in w}
    return names


def test_kernels_in_product_code_object(lib, tmp_path):
    """Exactly the three instantiations of distortion8<ADAPTIVE, INV32> the dispatch uses (it has
    no other template parameter): fp64 non-adaptive, fp32, fp64 adaptive.  The diagnostic library
    holds the same three."""
    key = "distortion8"
    want = {key + f"ILb{a}ELb{f}EEE" for a, f in ((0, 0), (0, 1), (1, 0))}
    for name in ("libdct_amd.so", "libdct_amd_diag.so"):
        names = _device_kernels(os.path.join(ROOT, "dct_amd", name), str(tmp_path / name))
        got = {n[n.index(key):][:len(key) + 11] for n in names if key in n}
        assert got == want, (name, sorted(n for n in names if key in n))
        # the names the existing tests count as substrings are not part of the new kernel's
        assert not [n for n in names if key in n and ("decode8" in n or "symbols_to_pixels" in n)]
