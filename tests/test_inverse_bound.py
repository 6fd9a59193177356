"""CPU: the rigorous error bound that admits a plan to the fused round trip's
fp32 inverse (roundtrip8_f32).

tools/inv_bound.py tracks the kernel's inverse (fp32 scale, the transposed AAN
graph over columns then rows, + 128) as linear forms with rounding bounds that
are linear in the per-coefficient input magnitudes, and generates
dct_amd/csrc/idct8_bound.h; plan_tables.hip evaluates it per plan.  Here:
  * the committed header is exactly the generator's output;
  * the library's per-plan bound (host-only diag entry point) equals the
    generator's for every standard quality, and admits exactly q <= 71;
  * an fp32 simulation of the kernel's operation sequence on blocks that maximise
    each coefficient (and on noise) stays within the bound against the oracle's
    fp64 reference inverse (src/dct.c:80-105, src/quantization.c:133-151);
  * on coefficients outside that range (a decoder's input is the caller's) the same
    bound at each block's own magnitudes holds, and no constant does.
The simulation itself is tools/inv_model.py.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inv_bound as IB  # noqa: E402
from aan_model import aan8t, scales, C4, C6, C2mC6, C2pC6  # noqa: E402,F401
import coef_families as CF  # noqa: E402
from inv_model import F32, kernel_inverse as _kernel_inverse  # noqa: E402,F401


@pytest.fixture(scope="module")
def GL():
    G, L = IB.bound()
    IB.check_linear(L)
    return G, L


def test_header_is_generated(GL):
    with open(os.path.join(ROOT, "dct_amd", "csrc", "idct8_bound.h")) as f:
        assert f.read() == IB.header(*GL)


def test_library_bound_equals_generator(GL):
    import dct_amd
    admitted = []
    for q in range(1, 101):
        b, a = dct_amd.inverse_bound(q, 0)
        want = IB.plan_error(q, *GL)[0]
        assert abs(b - want) <= 1e-9 * want, (q, b, want)
        assert a == (b <= 5e-5)
        assert dct_amd.inverse_bound(q, 1)[1] is False
        if a:
            admitted.append(q)
    assert admitted == list(range(1, 72)), admitted


def _basis_sign_blocks():
    import oracle as O
    D = O.dct_matrix(8)
    out = []
    for u in range(8):
        for v in range(8):
            sg = np.where(np.outer(D[u], D[v]) >= 0, 1, -1)
            out += [128 + 127 * sg, 128 - 128 * sg]
    return np.clip(np.array(out), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("q", [1, 10, 25, 50, 71])
def test_fp32_inverse_simulation_within_bound(GL, q):
    import oracle as O
    rng = np.random.default_rng(q)
    blocks = np.concatenate([_basis_sign_blocks(), rng.integers(0, 256, (4000, 8, 8)).astype(np.uint8),
                             rng.choice([0, 255], (2000, 8, 8)).astype(np.uint8)])
    plane = np.ascontiguousarray(blocks.transpose(1, 0, 2).reshape(8, -1))
    coef = O.forward_plane(plane, q, 0)
    want = O.inverse_plane(coef, q, 0) + 128.0
    S = np.array(scales())
    iscale32 = (O.dequant_matrix(O.quant_matrix(8, q)).ravel() * np.outer(S, S).ravel()).astype(np.float32)
    got = _kernel_inverse(coef, iscale32).astype(np.float64)
    err = float(np.abs(got - want).max())
    bound = IB.plan_error(q, *GL)[0]
    assert err <= bound, (q, err, bound)
    assert bound <= 5e-5


@pytest.mark.parametrize("q", [10, 50, 71])
def test_fp32_inverse_foreign_coefficients(GL, q):
    """Coefficients no forward produced (tools/coef_families.py: any int16, +-511, multiples
    of the plan's range, its edge, one-hot, saturated, sparse).  The fp32 inverse's error
    is bounded by tools/inv_bound.py block_error -- the plan's bound at each block's own
    magnitudes -- on every block; that bound is within kInvTol = 5e-5 on every block inside
    the plan's forward range; and the constant 1e-4 does NOT hold outside it (q50, q71 on
    32768 blocks of uniform int16, seed 7: about 5.5e-4 and 9.2e-4), which is why
    include/dct_amd.h states the decoders' bound per input domain."""
    import oracle as O
    G, L = GL
    iscale32 = (O.dequant_matrix(O.quant_matrix(8, q)).ravel() * np.outer(scales(), scales()).ravel()).astype(np.float32)
    qm = CF.qmax(q)
    assert IB.plan_error(q, G, L)[0] <= 5e-5
    for name in CF.NAMES:
        coef = CF.family(name, q)
        want = O.inverse_plane(coef, q, 0) + 128.0
        got = _kernel_inverse(coef, iscale32).astype(np.float64)
        e = IB.block_error(q, coef, G, L)
        err = np.abs(got - want)
        inside = (np.abs(coef.astype(np.int32)) <= qm[None, :]).all(axis=1)
        print(f"q{q} {name}: {int(inside.sum())}/{len(coef)} blocks in range, max err {err.max():.3e}, "
              f"max err/bound {(err / e).max():.3f}, max bound in range {e[inside].max() if inside.any() else 0.0:.3e}")
        assert (err <= e).all(), (q, name, float((err / e).max()))
        assert (e[inside] <= 5e-5).all(), (q, name, float(e[inside].max()))
    assert CF.family("range_x1", q).shape[0] == int(
        (np.abs(CF.family("range_x1", q).astype(np.int32)) <= qm[None, :]).all(axis=1).sum())
    if q in (50, 71):
        coef = CF.family("int16", q, n=32768, seed=7)
        err = np.abs(_kernel_inverse(coef, iscale32).astype(np.float64) - (O.inverse_plane(coef, q, 0) + 128.0))
        print(f"q{q} int16 x 32768: max err {err.max():.3e}")
        assert err.max() > 1e-4, (q, float(err.max()))
        assert (err <= IB.block_error(q, coef, G, L)).all()


def test_symbol_format_bound():
    """dctq_plan_symbol_bytes: 2-byte symbols exactly when the plan bounds every |quantized
    coefficient| by 511 (128 * L1(D[u]) * L1(D[v]) / Q_uv rounded, Q from
    src/quantization.c:51-77) -- standard tables q <= 90; and the bound holds on the
    oracle's forward of blocks built to hit it (each coefficient's sign pattern at +-128/127)."""
    import dct_amd
    import oracle as O
    got = [dct_amd.symbol_bytes(q) for q in range(1, 101)]
    want = [2 if np.floor(IB.coef_max() / IB.quant_table(q) + 0.5).max() <= 511 else 4 for q in range(1, 101)]
    assert got == want
    assert got == [2] * 90 + [4] * 10
    assert all(dct_amd.symbol_bytes(q, True) == got[q - 1] for q in (1, 50, 90, 91, 100))
    D = O.dct_matrix(8)
    blocks = []
    for u in range(8):
        for v in range(8):
            s = np.sign(np.outer(D[u], D[v]))
            blocks += [np.where(s >= 0, 127, -128) + 128, np.where(s >= 0, -128, 127) + 128]
    px = np.concatenate([np.concatenate(blocks[i:i + 8], axis=1) for i in range(0, 128, 8)], axis=0).astype(np.uint8)
    for q in (50, 90, 91, 100):
        m = int(np.abs(O.forward_plane(px, q, 0).astype(np.int32)).max())
        assert m <= np.floor(IB.coef_max() / IB.quant_table(q) + 0.5).max()
        if q <= 90:
            assert m <= 511
