"""GPU: the window decoder (dctq_decode_bits_window_planes) and the scaled decoder
(dctq_decode_bits_window_scaled_planes) on blocks, var_num and tables no forward of ours produced.
The inputs, their layouts and the conditions against a vacuous pass are built and asserted on the
CPU in tests/test_window_scaled_foreign_cpu.py (W), whose docstring describes them; every stream is
packed by tools/bits_ref.py and the expected coefficients are its CPU decode of the same bytes.

Yardsticks.  Window decoder: (i) bit for bit the same region of Plan.decode_bits on the same
stream (the equivalence include/dct_amd.h states), and (ii) that full decode within the full-size
decoders' bound of the fp64 oracle (TF.check_pixels: TF.pixel_bound for standard plans, max(fp64
bound, 1e-4) for caller tables), so that (i) is not two wrong answers agreeing.  Scaled decoder:
byte for byte tools/scaled_ref.py planes() of the CPU-decoded coefficients, Q the plan's table.

  1. the catalogue at the early-stop edges, full grid and one workgroup, three windows;
  2. every family of tools/coef_families.py, a whole-plane and an interior window;
  3. var_num the caller made up (TF.VAR_NUMS), through a window whose first frame, row and column
     are not 0, on a plane 128 blocks wide;
  4. caller tables (Plan.from_table): pictures' coefficients and corner blocks;
  5. exact rounding ties of the scaled sink at n = 1 and n = 4, the nearest misses at n = 2."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coef_families as CF  # noqa: E402
import scaled_ref  # noqa: E402
import test_custom_tables_gpu as TC  # noqa: E402
import test_decode_foreign_gpu as TF  # noqa: E402
import test_window_scaled_foreign_cpu as W  # noqa: E402

SCALES = W.SCALES


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import dct_amd
    dct_amd.lib()
    return torch


@pytest.fixture(scope="module")
def dm(T):
    import dct_amd
    return dct_amd


def gpu(T, a):
    return T.from_numpy(np.array(a)).cuda()  # a copy: the cached arrays are read-only


def device_stream(T, data, off):
    return gpu(T, data if len(data) else np.zeros(4, np.uint8)), gpu(T, np.asarray(off).view(np.int32))


@contextlib.contextmanager
def workgroups(dm, one):
    """one: every persistent launch inside runs as ONE workgroup; yields a check of that."""
    if not one:
        yield lambda: None
        return

    def check():
        assert dm.last_grid() == 1

    with dm.grid_limit(1):
        yield check


GRIDS = [pytest.param(False, id="full grid"), pytest.param(True, id="one workgroup")]


@functools.lru_cache(maxsize=None)
def std_table(q, ad):
    import dct_amd
    t = dct_amd.debug_tables(q, ad)[3].reshape(8, 8)
    assert np.array_equal(t, W.std_table(q))
    return t


def cut(full, windows, scale=1):
    return [p[f0:f1, y0 // scale:y1 // scale, x0 // scale:x1 // scale]
            for p, ((f0, f1), (y0, y1), (x0, x1)) in zip(full, windows)]


def assert_same(T, got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        w = w if T.is_tensor(w) else T.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == T.uint8 and tuple(g.shape) == tuple(w.shape), (what, k, tuple(g.shape), tuple(w.shape))
        g, w = g.cpu(), w.cpu()
        assert T.equal(g, w), (what, f"plane {k}", int((g != w).sum()), "pixels differ", T.nonzero(g != w)[:4].tolist())


def pixel_blocks(planes):
    """u8 tensors [F, H, W], one plane after the other -> [n, 64] in stored block order."""
    return np.concatenate([TF.blocks_of(f) for p in planes for f in p.cpu().numpy()])


def run_both(T, plan, by, boff, shapes, windows, coef, Q, ad, vns, what, check=lambda: None, scales=SCALES):
    """The two decoders on one stream through the named windows: (i) and the scaled definition.
    Returns the full decode for (ii)."""
    gv = [gpu(T, v) for v in vns] if ad else None
    full = plan.decode_bits(by, boff, shapes=shapes, var_nums=gv)
    check()
    whole = {}
    for name, win in windows.items():
        got = plan.decode_bits_window(by, boff, shapes, win, var_nums=gv)
        check()
        assert_same(T, got, cut(full, win), (*what, "window", name))
        for scale in scales:
            if scale not in whole:
                whole[scale] = scaled_ref.planes(coef, shapes, Q, scale, ad, vns if ad else None)
            got = plan.decode_bits_scaled(by, boff, shapes, scale, win, var_nums=gv)
            check()
            assert_same(T, got, cut(whole[scale], win, scale), (*what, "scale", scale, name))
    return full


# ---- 1. the catalogue ------------------------------------------------------------------------------
@pytest.mark.parametrize("one", GRIDS)
@pytest.mark.parametrize("q,ad", list(W.MAG))
def test_catalogue(T, dm, q, ad, one):
    s = W.catalogue_stream(W.MAG[q, ad])
    shapes = [W.catalogue_shape()]
    n = s["coef"].shape[0]
    vns = [TF.plain_var_num(n)]
    by, boff = device_stream(T, s["bytes"], s["off"])
    Q = std_table(q, ad)
    with workgroups(dm, one) as check:
        full = run_both(T, dm.Plan(q, ad), by, boff, shapes, W.catalogue_windows(), s["coef"], Q, ad, vns,
                        ("catalogue", q, ad), check)
    if not one:
        want, e = W.oracle_ref(s["coef"], Q, ad, vns[0])
        TF.check_pixels(pixel_blocks(full), want, e, f"catalogue q{q} a{ad}")
        for scale in SCALES:  # the pictures span the range: a block in the wrong place shows
            px = scaled_ref.planes(s["coef"], shapes, Q, scale, ad, vns)[0]
            assert int(px.max()) - int(px.min()) > 64, (scale, int(px.min()), int(px.max()))


# ---- 2. coefficient families -------------------------------------------------------------------------
def family_case(T, dm, q, ad, scales):
    plan = dm.Plan(q, ad)
    shares = {}
    for name in CF.NAMES:
        coef, vn, want, _ = TF.reference(name, q, ad)
        data, off, back = W.family_stream(name, q)
        assert np.array_equal(back, coef), name
        h, w = CF.plane_shape(coef.shape[0])
        by, boff = device_stream(T, data, off)
        full = run_both(T, plan, by, boff, [(1, h, w)], W.family_windows((h, w)), back, std_table(q, ad), ad, [vn],
                        ("family", name, q, ad), scales=scales)
        shares[name] = TF.check_pixels(pixel_blocks(full), want, TF.pixel_bound(name, q, ad), f"q{q} a{ad} {name}")
    return shares


@pytest.mark.parametrize("q,ad", TF.PLANS)
def test_families(T, dm, q, ad):
    """Window decoder: every plan of TF.PLANS.  Scaled decoder: the plans of W.SCALED_PLANS, all scales
    (their in-range condition is asserted on the CPU, W.test_family_shares)."""
    shares = family_case(T, dm, q, ad, SCALES if (q, ad) in W.SCALED_PLANS else ())
    assert max(shares[name] for name in CF.RANDOM) >= 0.05, shares


def test_scaled_plans_are_all_run():
    assert set(W.SCALED_PLANS) <= set(TF.PLANS)


# ---- 3. var_num the caller made up -------------------------------------------------------------------
@pytest.mark.parametrize("q,ad", TF.ADAPTIVE_PLANS)
def test_foreign_var_num(T, dm, q, ad):
    plan = dm.Plan(q, ad)
    windows = {"inner": W.VAR_WINDOW, "whole": [tuple((0, v) for v in W.VAR_SHAPE)]}
    for name in W.VAR_FAMILIES:
        coef, vn, want, tol = TF.reference(name, q, ad, True)
        data, off, back = W.family_stream(name, q)
        assert np.array_equal(back, coef)
        by, boff = device_stream(T, data, off)
        full = run_both(T, plan, by, boff, [W.VAR_SHAPE], windows, back, std_table(q, ad), ad, [vn],
                        ("foreign var_num", name, q))
        TF.check_pixels(pixel_blocks(full), want, tol, f"q{q} a{ad} {name}, foreign var_num")


# ---- 4. caller tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ad", [0, 1])
@pytest.mark.parametrize("tname", W.TABLES)
def test_caller_tables(T, dm, tname, ad):
    Q = TC.tables()[tname]
    plan = dm.Plan.from_table(Q, ad)
    shares = {}
    for kind in W.TABLE_KINDS:
        s = W.table_stream(tname, ad, kind)
        by, boff = device_stream(T, s["bytes"], s["off"])
        nbs = np.cumsum([f * (h // 8) * (w // 8) for f, h, w in W.TABLE_SHAPES])[:-1]
        vns = np.split(s["vn"], nbs)
        full = run_both(T, plan, by, boff, W.TABLE_SHAPES, W.TABLE_WINDOWS, s["coef"], Q, ad, vns,
                        ("table", tname, ad, kind))
        pb = pixel_blocks(full)
        k = s["npic"]
        shares[kind] = TF.check_pixels(pb[:k], s["want"][:k], s["e"][:k], f"{tname} a{ad} {kind}")
        TF.check_pixels(pb[k:], s["want"][k:], s["e"][k:], f"{tname} a{ad} corner blocks")
    assert max(shares.values()) > 0.05, (tname, ad, shares)


# ---- 5. ties in the scaled sink ----------------------------------------------------------------------
def scaled_row(T, plan, coef, scale, ad, one_grid=None):
    """The blocks as one row of a plane, decoded at 1 / scale: u8 [N, n, n]."""
    data, off, back = W.pack_coef(coef)
    assert np.array_equal(back, coef)
    by, boff = device_stream(T, data, off)
    N, n = len(coef), 8 // scale
    vns = [gpu(T, np.full(N, 2 ** 31 - 1, np.int32))] if ad else None   # nv = 1: the adaptive factor is 1.0
    got = plan.decode_bits_scaled(by, boff, [(1, 8, 8 * N)], scale, var_nums=vns)[0].cpu().numpy()
    return got.reshape(n, N, n).transpose(1, 0, 2)


@pytest.mark.parametrize("ad", [0, 1])
@pytest.mark.parametrize("q00", [1.0, 2.0])
def test_ties_n1(T, dm, q00, ad):
    """R = DC / (8 Q00) + 128 (adaptive: DC Q00 / 8 + 128) exactly: the stated pixel, the even neighbour."""
    Q = TC.tables()["edge512"] if q00 == 2.0 else None
    plan = dm.Plan.from_table(Q, ad) if q00 == 2.0 else dm.Plan(100, ad)
    coef, pix = W.ties_n1(q00, ad)
    got = scaled_row(T, plan, coef, 8, ad)[:, 0, 0]
    bad = np.flatnonzero(got != pix)
    assert np.array_equal(got, pix), [(int(coef[b, 0]), int(got[b]), int(pix[b])) for b in bad[:8]]


@pytest.mark.parametrize("ad", [0, 1])
def test_ties_n4(T, dm, ad):
    coef, pix = W.ties_n4()
    got = scaled_row(T, dm.Plan(100, ad), coef, 2, ad)
    bad = np.flatnonzero((got != pix).any(axis=(1, 2)))
    assert np.array_equal(got, pix), [(coef[b, [0, 2, 16, 18]].tolist(), got[b].tolist(), pix[b].tolist()) for b in bad[:4]]


def test_near_ties_n2(T, dm):
    coef = W.near_ties_n2()
    want = scaled_ref.blocks(coef, np.ones((8, 8)), 4, False)
    got = scaled_row(T, dm.Plan(100, 0), coef, 4, 0)
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert np.array_equal(got, want), [(coef[b, [0, 1, 8, 9]].tolist(), got[b].tolist(), want[b].tolist()) for b in bad[:4]]
