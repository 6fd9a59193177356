"""dct_amd -- MI355X-native 8x8 DCT + quantization hot path of erkinov-wtf/dct.

Python host over the C-ABI of ``libdct_amd.so`` (include/dct_amd.h, and the
reference's per-block API include/dct.h / include/quantization.h).  PyTorch is
used only as the owner of device memory and streams: tensors are handed to the
library as raw pointers on torch's current HIP stream, so torch.cuda.Event
timing sees the kernels.

The library is REQUIRED: importing a compute entry point without a built
``libdct_amd.so`` raises -- there is no CPU fallback in this package.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdct_amd.so")

# synthetic frame kinds (include/dct_amd.h, dctq_synth)
KINDS = {"uniform": 0, "smooth": 1, "const": 2, "extreme": 3}


class DctqError(RuntimeError):
    pass


class _Plane(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("stride", C.c_longlong), ("frame_stride", C.c_longlong),
                ("width", C.c_int), ("height", C.c_int), ("nframes", C.c_int)]


class _Window(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("nframes", C.c_int),
                ("x0", C.c_int), ("y0", C.c_int), ("frame0", C.c_int)]


class _Extent(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("nframes", C.c_int)]


class _Rgb(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("stride", C.c_longlong), ("frame_stride", C.c_longlong),
                ("channel_stride", C.c_longlong), ("pixel_step", C.c_int),
                ("width", C.c_int), ("height", C.c_int), ("nframes", C.c_int)]


class QuantContext(C.Structure):
    """QuantContext of include/quantization.h (the reference's public layout)."""
    _fields_ = [("block_size", C.c_int), ("quality", C.c_int), ("quant_matrix", C.POINTER(C.POINTER(C.c_double))),
                ("dequant_matrix", C.POINTER(C.POINTER(C.c_double))), ("adaptive", C.c_int)]


def _row_pointers(a):
    """double ** over the rows of a C-contiguous float64 array [n, n] (no copy; the result keeps a alive)."""
    rows = (C.POINTER(C.c_double) * a.shape[0])(*[C.cast(a[r].ctypes.data, C.POINTER(C.c_double))
                                                  for r in range(a.shape[0])])
    rows._array = a
    return rows


def quant_context(table, adaptive: bool = False, quality: int = 50, dequant=None, block_size: int = None) -> QuantContext:
    """A QuantContext over the caller's memory: quant_matrix points at the rows of table (a
    C-contiguous float64 numpy array [n, n], not copied, so later writes to it are writes to the
    context), dequant_matrix at those of dequant, or NULL.  block_size defaults to n."""
    import numpy as np
    for a in (table, dequant):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.ndim == 2
                                  and a.shape[0] == a.shape[1] and a.flags.c_contiguous):
            raise ValueError("table and dequant must be C-contiguous float64 arrays [n, n]")
    ctx = QuantContext(int(table.shape[0] if block_size is None else block_size), int(quality), None, None,
                       int(bool(adaptive)))
    ctx._rows = [_row_pointers(table), _row_pointers(dequant) if dequant is not None else None]
    ctx.quant_matrix = C.cast(ctx._rows[0], C.POINTER(C.POINTER(C.c_double)))
    if dequant is not None:
        ctx.dequant_matrix = C.cast(ctx._rows[1], C.POINTER(C.POINTER(C.c_double)))
    return ctx


_lib = None
_diag = None
DIAG_PATH = os.path.join(HERE, "libdct_amd_diag.so")


def _bind(L: C.CDLL, diagnostic: bool) -> C.CDLL:
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    sig = {
        "dctq_plan_create": ([i, i, C.POINTER(vp)], i),
        "dctq_plan_from_context": ([C.POINTER(QuantContext), C.POINTER(vp)], i),
        "dctq_plan_destroy": ([vp], None),
        "dctq_plan_set_fallback_counter": ([vp, vp], i),
        "dctq_forward_quant": ([vp, C.POINTER(_Plane), vp, vp, vp], i),
        "dctq_forward_quant_planes": ([vp, C.POINTER(_Plane), i, vp, vp, vp], i),
        "dctq_round_trip_planes": ([vp, C.POINTER(_Plane), i, vp, vp, vp, vp], i),
        "dctq_encode_workspace_bytes": ([ll], C.c_size_t),
        "dctq_encode_planes": ([vp, C.POINTER(_Plane), i, vp, vp, vp, ll, vp, vp], i),
        "dctq_encode_planes16": ([vp, C.POINTER(_Plane), i, vp, vp, vp, ll, vp, vp], i),
        "dctq_abi_version": ([], i),
        "dctq_forward_float": ([vp, C.POINTER(_Plane), vp, vp], i),
        "dctq_inverse": ([vp, vp, vp, ll, vp, vp], i),
        "dctq_decode_planes": ([vp, vp, vp, C.POINTER(_Plane), i, vp], i),
        "dctq_decode_symbols_planes": ([vp, vp, i, vp, vp, C.POINTER(_Plane), i, vp], i),
        "dctq_synth": ([C.c_uint64, i, C.POINTER(_Plane), vp], i),
        "dctq_error_string": ([i], C.c_char_p),
        "dctq_synchronize": ([vp], i),
        "dctq_rle_workspace_bytes": ([ll], C.c_size_t),
        "dctq_rle_count": ([vp, ll, vp, vp, vp], i),
        "dctq_rle_emit": ([vp, ll, vp, vp, vp], i),
        "dctq_rle_decode": ([vp, vp, ll, vp, vp], i),
        "dctq_rle_decode16": ([vp, vp, ll, vp, vp], i),
        "dctq_bits_workspace_bytes": ([ll], C.c_size_t),
        "dctq_bits_pack": ([vp, i, vp, ll, vp, vp, ll, vp, vp], i),
        "dctq_bits_decode": ([vp, vp, ll, vp, vp], i),
        "dctq_decode_bits_planes": ([vp, vp, vp, vp, C.POINTER(_Plane), i, vp], i),
        "dctq_decode_bits_window_planes": ([vp, vp, vp, vp, C.POINTER(_Window), C.POINTER(_Plane), i, vp], i),
        "dctq_decode_bits_window_scaled_planes": ([vp, vp, vp, vp, C.POINTER(_Window), C.POINTER(_Plane), i, i, vp], i),
        "dctq_bits_window_workspace_bytes": ([ll], C.c_size_t),
        "dctq_bits_window_offsets": ([vp, vp, C.POINTER(_Window), C.POINTER(_Extent), i, vp, vp, vp, vp], i),
        "dctq_bits_window_gather": ([vp, vp, C.POINTER(_Window), C.POINTER(_Extent), i, vp, vp, C.c_size_t, vp], i),
        "dctq_bits_paste_workspace_bytes": ([ll], C.c_size_t),
        "dctq_bits_paste_offsets": ([vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(_Window), C.POINTER(_Extent), i,
                                     vp, vp, vp, vp], i),
        "dctq_bits_paste_copy": ([vp, vp, vp, vp, C.POINTER(_Window), C.POINTER(_Extent), i, vp, vp, C.c_size_t, vp], i),
        "dctq_block_lengths": ([vp, ll, i, vp, vp, vp], i),
        "dctq_block_offsets_workspace_bytes": ([ll], C.c_size_t),
        "dctq_block_offsets": ([vp, i, ll, vp, vp, vp], i),
        "dctq_plan_symbol_bytes": ([vp], i),
        "dctq_huffman_bits": ([vp, ll, vp, vp], i),
        "dctq_huffman_bits_planes": ([vp, C.POINTER(_Plane), i, vp, vp], i),
        "dctq_distortion_planes": ([vp, C.POINTER(_Plane), i, vp, vp], i),
        "dctq_rgb_to_ycbcr_planes": ([C.POINTER(_Rgb), C.POINTER(_Plane), C.POINTER(_Plane), C.POINTER(_Plane), vp], i),
        "dctq_ycbcr_to_rgb_planes": ([C.POINTER(_Plane), C.POINTER(_Plane), C.POINTER(_Plane), C.POINTER(_Rgb), vp], i),
        "dctq_rgb_to_ycbcr_pad_planes": ([C.POINTER(_Rgb), C.POINTER(_Plane), C.POINTER(_Plane), C.POINTER(_Plane), vp], i),
        "dctq_ycbcr_to_rgb_crop_planes": ([C.POINTER(_Plane), C.POINTER(_Plane), C.POINTER(_Plane), C.POINTER(_Rgb), vp], i),
        "dctq_pad_planes": ([C.POINTER(_Plane), C.POINTER(_Plane), i, vp], i),
        "dctq_stream_release": ([vp], i),
    }
    if diagnostic:
        sig.update({
            "dctq_diag_plan_set_variant": ([vp, i], i),
            "dctq_diag_forward_quant_planes": ([vp, C.POINTER(_Plane), i, vp, vp, vp], i),
            "dctq_diag_forward_float": ([vp, C.POINTER(_Plane), vp, vp], i),
            "dctq_diag_inverse": ([vp, vp, vp, ll, vp, vp], i),
            "dctq_diag_plan_set_num_cus": ([vp, i], i),
            "dctq_diag_plan_set_inverse": ([vp, i], i),
            "dctq_diag_set_grid_limit": ([i], i),
            "dctq_diag_last_grid": ([C.POINTER(C.c_uint)], i),
            "dctq_debug_inverse_bound": ([i, i, C.POINTER(i)], C.c_double),
            "dctq_debug_symbol_bytes": ([i, i], i),
            "dctq_diag_legacy_lanes": ([C.POINTER(i), C.POINTER(i)], i),
            "dctq_diag_movement_planes": ([vp, C.POINTER(_Plane), i, vp, vp], i),
            "dctq_diag_movement_v2_planes": ([vp, C.POINTER(_Plane), i, vp, vp], i),
            "dctq_diag_movement_grid_planes": ([vp, C.POINTER(_Plane), i, vp, i, vp], i),
            "dctq_diag_rt_movement_planes": ([vp, C.POINTER(_Plane), i, vp, vp, vp], i),
            "dctq_diag_stream": ([i, vp, vp, ll, vp], i),
            "dctq_diag_stream_release": ([vp], i),
            "dctq_debug_tables": ([i, i, vp, vp, vp, vp], i),
            "dctq_debug_fastdiv": ([C.c_uint32, C.c_uint32], i),
            "dctq_debug_dc_table": ([i, vp], i),
            "dctq_debug_forward_kernel": ([i, i, ll, i], i),
            "dctq_diag_stream_stash_bytes": ([vp], ll),
        })
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    return L


def lib() -> C.CDLL:
    """Load libdct_amd.so, the product library (fails loudly if it has not been built).
    Inside grid_limit (tests only) it is the diagnostic library instead: the limit lives there."""
    global _lib
    if _grid_limited:
        return diag()
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DctqError(f"{LIB_PATH} is missing: run `python -m dct_amd.build` (hipcc, gfx950)")
        _lib = _bind(C.CDLL(LIB_PATH), False)
    return _lib


def diag() -> C.CDLL:
    """Load libdct_amd_diag.so: the same kernels plus the diagnostic entry points of
    csrc/dctq_diag.h (test-only kernel selection, movement / hardware ceilings, host
    table introspection).  Never used by the product path."""
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_PATH):
            raise DctqError(f"{DIAG_PATH} is missing: run `python -m dct_amd.build` (hipcc, gfx950)")
        _diag = _bind(C.CDLL(DIAG_PATH), True)
    return _diag


_grid_limited = False


@contextlib.contextmanager
def grid_limit(workgroups: int):
    """TESTS ONLY: cap the grid of every persistent grid-stride launch at `workgroups` (1..65535;
    dctq_diag_set_grid_limit), so a test-sized input gives each wave several tiles -- on the full
    grid (256 CUs, multipliers of 32-64) a wave sees one tile up to about 16 M blocks.  The limit
    lives in the diagnostic library, whose globals the product library does not share, so while
    the context is active lib() is that library: every module-level wrapper (rle_*, bits_*,
    block_*, huffman_bits, the colour conversions, frame_*, compress, decompress) and every Plan
    created inside goes through it.  A Plan created outside keeps its own library and is not
    limited.  On exit (also on an exception) the limit is 0 again; does not nest."""
    global _grid_limited
    if _grid_limited:
        raise DctqError("grid_limit does not nest")
    L = diag()
    _check(L.dctq_diag_set_grid_limit(int(workgroups)), L)
    _grid_limited = True
    try:
        yield
    finally:
        _grid_limited = False
        L.dctq_diag_set_grid_limit(0)


def last_grid() -> int:
    """TESTS ONLY: the workgroups of this thread's most recent persistent launch through the
    diagnostic library (dctq_diag_last_grid)."""
    n = C.c_uint(0)
    _check(diag().dctq_diag_last_grid(C.byref(n)), diag())
    return int(n.value)


def _check(rc: int, L: C.CDLL = None) -> None:
    if rc != 0:
        raise DctqError(f"dctq error {rc}: {(L or lib()).dctq_error_string(rc).decode()}")


def _need(t, numel: int, dtype, what: str, device=None):
    """A caller-supplied buffer must be a contiguous device tensor of the right
    dtype holding at least `numel` elements (on `device` when given): the kernels
    write through the raw pointer, so a short or host tensor is refused here."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DctqError(f"{what} must be a tensor on a HIP device")
    if t.dtype != dtype:
        raise DctqError(f"{what} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise DctqError(f"{what} must be contiguous")
    if t.numel() < numel:
        raise DctqError(f"{what} holds {t.numel()} elements, {numel} needed")
    if device is not None and t.device != device:
        raise DctqError(f"{what} is on {t.device}, the input is on {device}")
    return t


def _stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _on_stream(stream):
    """torch's own copies and fills go to `stream` too (None: the current one)."""
    import torch
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _read_back(t, stream):
    """A small int32 device tensor of uint32 bit patterns (offsets, totals) as a list of ints:
    copied on `stream` (None: the current one), so after the launches sent there (one sync)."""
    with _on_stream(stream):
        return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


def plane_desc(px, width: int = None, height: int = None):
    """Describe a uint8 CUDA tensor [H, W] or [F, H, W] (rows may be padded: stride = px.stride(-2))."""
    import torch
    if px.dtype != torch.uint8 or not px.is_cuda:
        raise DctqError("pixels must be a uint8 tensor on a HIP device")
    if px.dim() == 2:
        px = px.unsqueeze(0)
    if px.dim() != 3 or px.stride(-1) != 1:
        raise DctqError("pixels must be [H, W] or [F, H, W] with unit column stride")
    f, h, w = px.shape
    return _Plane(px.data_ptr(), px.stride(1), px.stride(0) if f > 1 else px.stride(1) * h,
                  width if width is not None else w, height if height is not None else h, f)


def _nblocks(d) -> int:
    """The 8 x 8 blocks of a _Plane, or of an (F, H, W) shape."""
    if isinstance(d, _Plane):
        return d.nframes * (d.width // 8) * (d.height // 8)
    f, h, w = d
    return f * (h // 8) * (w // 8)


def _whole_blocks(f, h, w) -> bool:
    """A stored plane is whole blocks and has at least one frame."""
    return f >= 1 and h >= 8 and w >= 8 and not (h % 8 or w % 8)


def _plane_set(planes):
    """(n, descs, nbs) of a list of source planes: the _Plane array a `const dctq_plane *`
    parameter takes and each plane's block count."""
    n = len(planes)
    descs = (_Plane * n)(*[plane_desc(px) for px in planes])
    return n, descs, [_nblocks(d) for d in descs]


def _ptr(t):
    """A tensor (or None) as a `void *` argument (or NULL)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptrs(ts):
    """A list of tensors (or None) as a `void *const *` argument (or NULL): the ctypes array
    itself, which owns the pointers and lives as long as the argument list it stands in."""
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) if ts is not None else None


def _per_plane(outs, nbs, per, dtype, planes, device=None):
    """The per-plane outputs of a multi-plane call: outs as given, or [nb_k, per] tensors of
    dtype beside each plane (or all on device).  _need_planes checks either."""
    import torch
    if outs is None:
        outs = [torch.empty((nb, per), dtype=dtype, device=device or px.device) for nb, px in zip(nbs, planes)]
    return outs


def _out(out, shape, dtype, device):
    """The one result of a call: out as given, or a new tensor of shape beside the input; checked
    either way (_need), which is what refuses an input that is not on a device."""
    import math
    import torch
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    return _need(out, math.prod(shape), dtype, "out", device)


def _workspace(bytes_fn, n, device):
    """The scratch of an n-block call whose size dctq_*_workspace_bytes (bytes_fn) states."""
    import torch
    return torch.empty(int(bytes_fn(n)) // 4 + 1, dtype=torch.int32, device=device)


def _shapes3(shapes):
    """shapes entries (F, H, W) or (H, W) -> [(F, H, W)] of ints."""
    shapes = [(1, *map(int, s)) if len(s) == 2 else tuple(map(int, s)) for s in shapes]
    if any(len(s) != 3 for s in shapes):
        raise DctqError("shapes entries must be (F, H, W) or (H, W)")
    return shapes


def _clamp_quality(q) -> int:
    """A quality as the plan clamps it (1..100)."""
    return min(max(int(q), 1), 100)


def _need_planes(outs, var_nums, recons, nbs, planes):
    """Per-plane output lists of the multi-plane calls: one entry per plane, each
    sized for that plane's blocks (_need)."""
    import torch
    for name, ts, per, dt in (("outs", outs, 64, torch.int16), ("var_nums", var_nums, 1, torch.int32),
                              ("recons", recons, 64, torch.float32)):
        if ts is None:
            continue
        if len(ts) != len(nbs):
            raise DctqError(f"{name} needs one tensor per plane ({len(nbs)}), got {len(ts)}")
        for k, (t, nb, px) in enumerate(zip(ts, nbs, planes)):
            _need(t, nb * per, dt, f"{name}[{k}]", px.device)


def _decode_outs(what, n, shapes, outs, var_nums, devices, var_nbs=None, unit=8):
    """The destination planes of decode_planes and the fused decoders: (outs, descs, nbs).
    shapes[k] is (F, H, W) or (H, W); outs[k], if given, a u8 tensor [F, H, W] or [H, W], possibly
    a strided view; one of the two is needed, and both must agree.  var_nums[k], if given, is
    sized for var_nbs[k] blocks (None: plane k's own).  devices[k]: where outs[k] is allocated.
    unit: the pixels a block gives a destination's side (8; 4, 2 or 1 for a reduced picture,
    where var_nbs is needed: nbs counts 8 x 8 blocks)."""
    import torch
    if shapes is None and outs is None:
        raise DctqError(f"{what} needs shapes or outs")
    for name, ts in (("shapes", shapes), ("outs", outs), ("var_nums", var_nums)):
        if ts is not None and len(ts) != n:
            raise DctqError(f"{name} needs one entry per plane ({n}), got {len(ts)}")
    if shapes is not None:
        shapes = _shapes3(shapes)
    if outs is None:
        outs = [torch.empty(s, dtype=torch.uint8, device=d) for s, d in zip(shapes, devices)]
    _, descs, nbs = _plane_set(outs)
    for k, (d, o) in enumerate(zip(descs, outs)):
        if shapes is not None and (d.nframes, d.height, d.width) != shapes[k]:
            raise DctqError(f"outs[{k}] is {tuple(o.shape)}, shapes[{k}] says {shapes[k]}")
        if d.width % unit or d.height % unit:
            raise DctqError(f"outs[{k}]: width and height must be multiples of {unit}")
        if var_nums is not None:
            _need(var_nums[k], (var_nbs or nbs)[k], torch.int32, f"var_nums[{k}]", o.device)
    return outs, descs, nbs


def _stored_windows(shapes, windows):
    """The windows of the window decoders, checked: shapes[k] the STORED (F, H, W) or (H, W) of
    plane k, windows[k] = ((f0, f1), (y0, y1), (x0, x1)), half-open, y and x in pixels and
    multiples of 8 -> (wins, wshapes, nbs): the _Window array a `const dctq_window *` parameter
    takes, each window's own (F, H, W), and the stored planes' block counts."""
    n = len(shapes)
    if len(windows) != n:
        raise DctqError(f"windows needs one entry per plane ({n}), got {len(windows)}")
    shapes = _shapes3(shapes)
    wins, wshapes = [], []
    for k, ((f, h, w), win) in enumerate(zip(shapes, windows)):
        try:
            (f0, f1), (y0, y1), (x0, x1) = [tuple(map(int, r)) for r in win]
        except (TypeError, ValueError):
            raise DctqError(f"windows[{k}] must be ((f0, f1), (y0, y1), (x0, x1))") from None
        if not _whole_blocks(f, h, w):
            raise DctqError(f"shapes[{k}] {(f, h, w)}: height and width must be multiples of 8, nframes >= 1")
        if not (0 <= f0 < f1 <= f and 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w):
            raise DctqError(f"windows[{k}] {win} is empty or leaves the stored plane {(f, h, w)}")
        if y0 % 8 or y1 % 8 or x0 % 8 or x1 % 8:
            raise DctqError(f"windows[{k}] {win}: rows and columns must be multiples of 8")
        wins.append(_Window(w, h, f, x0, y0, f0))
        wshapes.append((f1 - f0, y1 - y0, x1 - x0))
    nbs = [_nblocks(s) for s in shapes]
    if sum(nbs) >= 1 << 26:
        raise DctqError("more than 2^26 - 1 blocks in one decode")
    return (_Window * n)(*wins), wshapes, nbs


SCALES = {2: 1, 4: 2, 8: 3}   # scale -> log2_scale of dctq_decode_bits_window_scaled_planes


def _log2_scale(scale) -> int:
    """log2 of a reduction's scale, or DctqError: 2, 4 and 8 are all there is."""
    if isinstance(scale, bool) or scale not in SCALES:
        raise DctqError(f"scale must be 2, 4 or 8, got {scale!r}")
    return SCALES[scale]


class Plan:
    """Tables for one (quality, adaptive) configuration on the current device
    (quant_init(8, quality, adaptive) semantics, src/quantization.c:19-41)."""

    def __init__(self, quality: int = 50, adaptive: bool = False, variant: int = None, diagnostic: bool = False,
                 num_cus: int = None, inverse: str = None):
        """variant (tests / A/B only): force the forward kernel through the diagnostic
        library (dctq_diag_plan_set_variant: 1 = v1, 3 = v3 in-place ties, 4 = v2 tie
        queue, at any size); num_cus (tests only): launch as if the device had that many
        CUs (dctq_diag_plan_set_num_cus: smaller grids, more batches per wave);
        diagnostic: create the plan in the diagnostic library (needed for
        diag_movement_planes); inverse="fp64" (tests only): the fused round trip uses
        the paired-lane fp64 inverse even when the plan is admitted to the fp32 one
        (dctq_diag_plan_set_inverse)."""
        self.quality, self.adaptive = quality, bool(adaptive)
        diagnostic = diagnostic or variant is not None or num_cus is not None or inverse is not None
        self._L = diag() if diagnostic else lib()
        # a forced variant is honoured by the diagnostic entry points only (csrc/dctq_diag.h)
        self._diag = variant is not None
        h = C.c_void_p()
        self._chk(self._L.dctq_plan_create(int(quality), int(bool(adaptive)), C.byref(h)))
        self._h = h
        if variant is not None:
            self._chk(self._L.dctq_diag_plan_set_variant(h, int(variant)))
        if num_cus is not None:
            self._chk(self._L.dctq_diag_plan_set_num_cus(h, int(num_cus)))
        if inverse is not None:
            if inverse not in ("fp64", "auto"):
                raise DctqError('inverse must be "fp64" or "auto"')
            self._chk(self._L.dctq_diag_plan_set_inverse(h, 0 if inverse == "fp64" else 1))

    @classmethod
    def from_context(cls, ctx, diagnostic: bool = False):
        """A plan bound to a reference-style context (dctq_plan_from_context): ctx is a
        QuantContext (this module's ctypes structure of include/quantization.h) whose
        quant_matrix rows the caller set.  Only block_size, quality, adaptive and the VALUES of
        quant_matrix are read, and the values are copied before the call returns: plan.table is
        the plan's read-only copy.  Anything the library refuses raises DctqError."""
        import numpy as np
        self = cls.__new__(cls)
        self._L = diag() if diagnostic else lib()
        self._diag = False
        self._h = None
        h = C.c_void_p()
        self._chk(self._L.dctq_plan_from_context(C.byref(ctx) if ctx is not None else None, C.byref(h)))
        self._h = h
        self.quality, self.adaptive = int(ctx.quality), bool(ctx.adaptive)
        self.table = np.array([[ctx.quant_matrix[r][c] for c in range(8)] for r in range(8)], dtype=np.float64)
        self.table.setflags(write=False)
        return self

    @classmethod
    def from_table(cls, table, adaptive: bool = False, quality: int = 50, diagnostic: bool = False):
        """A plan of the caller's own quantization table: table holds the 8 x 8 doubles of a
        QuantContext's quant_matrix, each in [1, 65535] (the library refuses anything else with
        its invalid-argument error, DctqError).  The context handed to dctq_plan_from_context
        has block_size 8, row pointers to the doubles, the given quality and adaptive, and a NULL
        dequant_matrix: the library dequantizes with 1 / table, as the reference's
        generate_dequant_matrix would.  quality is a label only (plan.quality); plan.table keeps
        the values, and every method works as on a standard plan.  compress / decompress stay on
        standard plans: the frame v1 header stores a quality, not a table."""
        import numpy as np
        t = np.ascontiguousarray(table, dtype=np.float64)
        if t.size != 64:
            raise ValueError("table must hold 8 x 8 entries")
        return cls.from_context(quant_context(t.reshape(8, 8), adaptive, quality), diagnostic)

    def _chk(self, rc: int) -> None:
        _check(rc, self._L)

    def _fn(self, name: str):
        """The entry point dctq_<name> of the plan's library, or its dctq_diag_<name> twin when a
        variant is forced (only the twins honour it, csrc/dctq_diag.h)."""
        return getattr(self._L, ("dctq_diag_" if self._diag else "dctq_") + name)

    def close(self):
        if getattr(self, "_h", None):
            self._L.dctq_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_fallback_counter(self, counter):
        """counter: int64 CUDA tensor of one element (or None)."""
        self._chk(self._L.dctq_plan_set_fallback_counter(self._h, _ptr(counter)))

    # --- hot path -------------------------------------------------------
    def forward_quant(self, px, out=None, var_num=None, stream=None):
        """u8 [H,W] / [F,H,W] -> int16 [F*H/8*W/8, 64] quantized coefficients (bit-exact)."""
        import torch
        d = plane_desc(px)
        nblk = _nblocks(d)
        out = _out(out, (nblk, 64), torch.int16, px.device)
        if var_num is not None:
            _need(var_num, nblk, torch.int32, "var_num", px.device)
        if self._diag:   # a forced variant: the planes call has the twin, dctq_forward_quant has none
            self.forward_quant_planes([px], [out], None if var_num is None else [var_num], stream)
        else:
            self._chk(self._L.dctq_forward_quant(self._h, C.byref(d), _ptr(out), _ptr(var_num), _stream_ptr(stream)))
        return out

    def forward_quant_planes(self, planes, outs=None, var_nums=None, stream=None):
        """Up to 4 u8 planes of any geometry (e.g. Y, Cb, Cr) in ONE launch; returns the list
        of int16 [nblk_k, 64] outputs, each equal to forward_quant(planes[k])."""
        import torch
        n, descs, nbs = _plane_set(planes)
        outs = _per_plane(outs, nbs, 64, torch.int16, planes)
        _need_planes(outs, var_nums, None, nbs, planes)
        self._chk(self._fn("forward_quant_planes")(self._h, descs, n, _ptrs(outs), _ptrs(var_nums), _stream_ptr(stream)))
        return outs

    def diag_movement_planes(self, planes, outs, stream=None, shape: int = 3, grid_mult: int = 0):
        """DIAGNOSTIC: the bytes forward_quant_planes moves, with no arithmetic (outs receive
        pixel bytes, not coefficients) -- the memory ceiling of that access pattern."""
        n, descs, nbs = _plane_set(planes)
        _need_planes(outs, None, None, nbs, planes)
        if self._L is not _diag:
            raise DctqError("diag_movement_planes needs a plan of the diagnostic library (Plan(..., diagnostic=True))")
        if grid_mult:
            self._chk(self._L.dctq_diag_movement_grid_planes(self._h, descs, n, _ptrs(outs), grid_mult,
                                                             _stream_ptr(stream)))
            return outs
        fn = self._L.dctq_diag_movement_planes if shape == 3 else self._L.dctq_diag_movement_v2_planes
        self._chk(fn(self._h, descs, n, _ptrs(outs), _stream_ptr(stream)))
        return outs

    def diag_rt_movement_planes(self, planes, outs, recons, stream=None):
        """DIAGNOSTIC: the bytes round_trip_planes moves (its grid, stage and stores), with no
        arithmetic (outs/recons receive pixel bytes) -- the memory ceiling of that pattern."""
        n, descs, nbs = _plane_set(planes)
        _need_planes(outs, None, recons, nbs, planes)
        if self._L is not _diag:
            raise DctqError("diag_rt_movement_planes needs a plan of the diagnostic library (Plan(..., diagnostic=True))")
        self._chk(self._L.dctq_diag_rt_movement_planes(self._h, descs, n, _ptrs(outs), _ptrs(recons),
                                                      _stream_ptr(stream)))
        return outs, recons

    def round_trip_planes(self, planes, outs=None, recons=None, var_nums=None, stream=None):
        """Fused forward + inverse of up to 4 planes in ONE launch.  Returns (coefs, recons):
        int16 [nblk_k, 64] (== forward_quant) and float32 [nblk_k, 64]
        (== inverse(coef, var_num) within 1e-4)."""
        import torch
        n, descs, nbs = _plane_set(planes)
        outs = _per_plane(outs, nbs, 64, torch.int16, planes)
        recons = _per_plane(recons, nbs, 64, torch.float32, planes)
        _need_planes(outs, var_nums, recons, nbs, planes)
        self._chk(self._L.dctq_round_trip_planes(self._h, descs, n, _ptrs(outs), _ptrs(var_nums), _ptrs(recons),
                                                 _stream_ptr(stream)))
        return outs, recons

    @property
    def symbol_bytes(self) -> int:
        """The most compact symbol format this plan admits (dctq_plan_symbol_bytes): 2 when the
        plan bounds every |quantized coefficient| by 511 (dctq_encode_planes16), else 4."""
        return int(self._L.dctq_plan_symbol_bytes(self._h))

    def encode_planes(self, planes, outs=None, capacity=None, stream=None, symbol_bytes=None):
        """Forward + zigzag/RLE of up to 4 planes (the count fused into the forward launch).
        Returns (coefs [int16 [nblk_k, 64]], offsets int32 [N+1], symbols [total]) -- offsets
        hold uint32 bit patterns, blocks numbered plane by plane.  symbol_bytes 4
        (dctq_encode_planes): int32 holding (uint16)value | run << 16; 2
        (dctq_encode_planes16, only where the plan admits it): int16 holding
        run << 10 | (value & 0x3FF); None: the most compact format the plan admits
        (self.symbol_bytes).  capacity (symbols) defaults to the worst case (64 per block).
        Reads the total back (one sync)."""
        import torch
        sb = self.symbol_bytes if symbol_bytes is None else int(symbol_bytes)
        if sb not in (2, 4):
            raise ValueError("symbol_bytes must be 2 or 4")
        n, descs, nbs = _plane_set(planes)
        nb = sum(nbs)
        dev = planes[0].device
        outs = _per_plane(outs, nbs, 64, torch.int16, planes, device=dev)
        _need_planes(outs, None, None, nbs, planes)
        cap = 64 * nb if capacity is None else int(capacity)
        off = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        sym = torch.empty(max(cap, 1), dtype=torch.int16 if sb == 2 else torch.int32, device=dev)
        ws = _workspace(self._L.dctq_encode_workspace_bytes, nb, dev)
        fn = self._L.dctq_encode_planes16 if sb == 2 else self._L.dctq_encode_planes
        self._chk(fn(self._h, descs, n, _ptrs(outs), _ptr(off), _ptr(sym), cap, _ptr(ws), _stream_ptr(stream)))
        total = _read_back(off[nb:], stream)[0]
        return outs, off, sym[:min(total, cap)]

    def _per_block_planes(self, fn, planes, out, stream):
        """The body of huffman_bits_planes and distortion_planes: one int32 per block of up to 4
        planes, blocks numbered plane by plane."""
        import torch
        n, descs, nbs = _plane_set(planes)
        out = _out(out, (sum(nbs),), torch.int32, planes[0].device)
        self._chk(fn(self._h, descs, n, _ptr(out), _stream_ptr(stream)))
        return out

    def huffman_bits_planes(self, planes, out=None, stream=None):
        """Per-block Huffman size straight from up to 4 u8 planes (the whole per-block loop of
        tests/test_entropy.c:300-341 on the GPU, coefficients kept on chip): int32 [N], blocks
        numbered plane by plane, equal to huffman_bits(cat(forward_quant_planes(planes)))."""
        return self._per_block_planes(self._L.dctq_huffman_bits_planes, planes, out, stream)

    def distortion_planes(self, planes, out=None, stream=None):
        """Per-block squared error of the decoded picture straight from up to 4 u8 planes in ONE
        launch (dctq_distortion_planes; no coefficient, recon or picture buffer): int32 [N],
        blocks numbered as huffman_bits_planes numbers them, entry b the sum over block b of
        (px - dec)^2 with dec bit for bit the pixels of
        decode_planes(forward_quant_planes(planes, var_nums), var_nums)."""
        if len(planes) == 0:
            raise DctqError("distortion_planes needs at least one plane")
        return self._per_block_planes(self._L.dctq_distortion_planes, planes, out, stream)

    def rate_distortion_planes(self, planes, stream=None):
        """(bits, sse) = (huffman_bits_planes(planes), distortion_planes(planes)): both columns
        of the reference's per-block report (tests/test_entropy.c:300-393), two launches on one
        stream, pixels in and 4 + 4 B per block out."""
        return self.huffman_bits_planes(planes, stream=stream), self.distortion_planes(planes, stream=stream)

    def forward_float(self, px, out=None, stream=None):
        import torch
        d = plane_desc(px)
        nblk = _nblocks(d)
        out = _out(out, (nblk, 64), torch.float32, px.device)
        self._chk(self._fn("forward_float")(self._h, C.byref(d), _ptr(out), _stream_ptr(stream)))
        return out

    def inverse(self, coef, var_num=None, out=None, stream=None):
        """int16 [N, 64] -> float32 [N, 64] = dct_inverse(dequantize(coef)) + 128: fp64, rounded
        once to fp32 (|err| <= 2^-24 |recon|: below 1e-4 for |recon| < 2048, i.e. for every
        forward-produced block of a non-adaptive plan, not for arbitrary coefficients)."""
        import torch
        _need(coef, 0, torch.int16, "coef")
        n = coef.numel() // 64
        out = _out(out, (n, 64), torch.float32, coef.device)
        if var_num is not None:
            _need(var_num, n, torch.int32, "var_num", coef.device)
        self._chk(self._fn("inverse")(self._h, _ptr(coef), _ptr(var_num), n, _ptr(out), _stream_ptr(stream)))
        return out

    def decode_planes(self, coefs, shapes=None, outs=None, var_nums=None, stream=None):
        """Quantized coefficients -> u8 pixels of up to 4 planes in ONE launch
        (dctq_decode_planes): coefs[k] int16 [nblk_k, 64] in forward_quant's block order,
        var_nums[k] int32 [nblk_k] (required for adaptive plans, ignored otherwise).
        shapes[k] is (F, H, W) or (H, W); outs[k], if given, is a u8 tensor [F, H, W] or
        [H, W] and may be a strided view (e.g. a padded buffer sliced to width): bytes
        outside width x height of each frame are not touched.  One of shapes / outs is
        needed.  Returns the list of u8 tensors [F, H, W] (outs as given), each pixel
        rne(clamp(r, 0, 255)) of the fp32 recon r that round_trip_planes reports.
        Within 0.5 + 1e-4 of the clamped reference for coefficients inside the plan's
        forward range (what forward_quant produces from u8 pixels); any other int16 is
        decoded too, within 0.5 + a bound linear in the block's coefficient magnitudes
        (include/dct_amd.h, tools/inv_bound.py block_error)."""
        import torch
        outs, descs, nbs = _decode_outs("decode_planes", len(coefs), shapes, outs, var_nums,
                                        [c.device for c in coefs])
        for k, (o, c) in enumerate(zip(outs, coefs)):
            _need(c, nbs[k] * 64, torch.int16, f"coefs[{k}]", o.device)
        self._chk(self._L.dctq_decode_planes(self._h, _ptrs(coefs), _ptrs(var_nums), descs, len(coefs),
                                             _stream_ptr(stream)))
        return outs

    def _decode_stream(self, what, need, src, offsets, shapes, outs, var_nums, stream, launch, stored=None, unit=8):
        """The body of the fused decoders decode_symbols, decode_bits and decode_bits_window (what):
        the source checked by its validator (need: _need_symbols or _need_bytes), the destinations
        made or checked (_decode_outs), the offsets checked, all on one device, then the wrapper's
        own C call, launch(var_nums, descs, n, stream).  stored: the block counts the stream is
        numbered over and var_nums are sized by, where they are not the destinations' own (a window);
        unit: as _decode_outs."""
        need(src)
        n = len(shapes if shapes is not None else outs if outs is not None else ())
        outs, descs, nbs = _decode_outs(what, n, shapes, outs, var_nums, [src.device] * n, stored, unit)
        _need_byte_offsets(offsets, sum(stored or nbs), src)
        if any(o.device != src.device for o in outs):
            raise DctqError(f"{'symbols' if need is _need_symbols else 'bytes'}, offsets and outs must be on one device")
        self._chk(launch(_ptrs(var_nums), descs, n, _stream_ptr(stream)))
        return outs

    def decode_symbols(self, symbols, offsets, shapes=None, outs=None, var_nums=None, stream=None):
        """Run-length symbols -> u8 pixels of up to 4 planes in ONE launch, with no
        coefficient buffer (dctq_decode_symbols_planes): bit for bit
        decode_planes(split(rle_decode(symbols, offsets)), ...).  symbols / offsets as
        encode_planes returns them (blocks numbered plane by plane; offsets int32
        [sum(nblk_k) + 1]); symbols.dtype picks the format (int16: 2-byte, int32: 4-byte),
        whatever the plan's own symbol_bytes.  shapes / outs / var_nums as decode_planes,
        and its error bound for the domain the symbols' values fall in (a 4-byte symbol
        carries any int16, a 2-byte symbol [-512, 511])."""
        return self._decode_stream(
            "decode_symbols", _need_symbols, symbols, offsets, shapes, outs, var_nums, stream,
            lambda vn, descs, n, s: self._L.dctq_decode_symbols_planes(
                self._h, _ptr(symbols), symbols.element_size(), _ptr(offsets), vn, descs, n, s))

    def decode_bits(self, bytes, offsets, shapes=None, outs=None, var_nums=None, stream=None):
        """The bit-packed stream "bits v1" -> u8 pixels of up to 4 planes in ONE launch, with no
        coefficient buffer (dctq_decode_bits_planes): bit for bit
        decode_planes(split(bits_decode(bytes, offsets)), ...).  bytes (uint8) / offsets (int32
        [sum(nblk_k) + 1], byte offsets) as bits_pack returns them, blocks numbered plane by
        plane; any bytes decode.  shapes / outs / var_nums as decode_planes, and its error bound
        for the domain the decoded values fall in (a packed symbol carries any int16)."""
        return self._decode_stream(
            "decode_bits", _need_bytes, bytes, offsets, shapes, outs, var_nums, stream,
            lambda vn, descs, n, s: self._L.dctq_decode_bits_planes(self._h, _ptr(bytes), _ptr(offsets), vn, descs, n, s))

    def decode_bits_window(self, bytes, offsets, shapes, windows, outs=None, var_nums=None, stream=None):
        """A window of every plane of a "bits v1" stream -> u8 pixels in ONE launch that reads
        only the blocks inside the windows (dctq_decode_bits_window_planes).  shapes[k] is the
        STORED (F, H, W) or (H, W) of plane k, what bytes / offsets (the whole stream's, as for
        decode_bits) are numbered over; windows[k] = ((f0, f1), (y0, y1), (x0, x1)), half-open,
        y and x in pixels and multiples of 8.  Returns the list of u8 tensors [f1 - f0, y1 - y0,
        x1 - x0], each bit for bit decode_bits(bytes, offsets, shapes=shapes, ...)[k][f0:f1,
        y0:y1, x0:x1].  outs, if given, are the windows' own tensors and may be strided views
        (bytes outside them are not touched); var_nums[k] (adaptive plans) is the whole stored
        plane's.  The work unit is a run of up to 64 blocks of one window row
        (tools/window_ref.py): a window narrower than 512 pixels leaves part of each wave idle."""
        wins, wshapes, nbs = _stored_windows(shapes, windows)
        if self.adaptive and var_nums is None:
            raise DctqError("adaptive decode needs var_nums")
        return self._decode_stream(
            "decode_bits_window", _need_bytes, bytes, offsets, wshapes, outs, var_nums, stream,
            lambda vn, descs, n, s: self._L.dctq_decode_bits_window_planes(
                self._h, _ptr(bytes), _ptr(offsets), vn, wins, descs, n, s),
            stored=nbs)

    def decode_bits_scaled(self, bytes, offsets, shapes, scale, windows=None, outs=None, var_nums=None, stream=None):
        """A "bits v1" stream -> u8 pixels at 1 / scale size (scale 2, 4 or 8) in ONE launch, with
        no full-size picture in between (dctq_decode_bits_window_scaled_planes): every stored
        8 x 8 block gives n x n pixels, n = 8 / scale, from its n x n lowest coefficients, exactly
        as include/dct_amd.h defines them (tools/scaled_ref.py applied to bits_decode(bytes,
        offsets), byte for byte; for scale 8 the block's mean).  shapes, windows and var_nums as
        decode_bits_window; windows None: the whole planes.  Returns the list of u8 tensors
        [f1 - f0, (y1 - y0) / scale, (x1 - x0) / scale].  outs, if given, are those tensors and may
        be strided views whose address and strides are multiples of n bytes (bytes outside them
        are not touched).  The bit walk of a block stops after its corner, which is where the
        time goes at full size."""
        log2s = _log2_scale(scale)
        shapes = _shapes3(shapes)
        if windows is None:
            windows = [((0, f), (0, h), (0, w)) for f, h, w in shapes]
        wins, wshapes, nbs = _stored_windows(shapes, windows)
        if self.adaptive and var_nums is None:
            raise DctqError("adaptive decode needs var_nums")
        return self._decode_stream(
            "decode_bits_scaled", _need_bytes, bytes, offsets, [(f, h // scale, w // scale) for f, h, w in wshapes],
            outs, var_nums, stream,
            lambda vn, descs, n, s: self._L.dctq_decode_bits_window_scaled_planes(
                self._h, _ptr(bytes), _ptr(offsets), vn, wins, descs, n, log2s, s),
            stored=nbs, unit=8 >> log2s)

    def encode_bits_planes(self, planes, outs=None, capacity=None, stream=None, symbol_bytes=None):
        """encode_planes + bits_pack: forward, zigzag/RLE and the bit-packed stream of up to 4
        planes.  Returns (coefs [int16 [nblk_k, 64]], byte_offsets int32 [N+1], bytes uint8
        [total]); capacity (bytes) defaults to the stream's own size.  The symbols are an
        intermediate of the plan's most compact format (or symbol_bytes)."""
        coefs, off, sym = self.encode_planes(planes, outs=outs, stream=stream, symbol_bytes=symbol_bytes)
        packed, boff = bits_pack(sym, off, capacity=capacity, stream=stream)
        return coefs, boff, packed

    def decode(self, coef, shape=None, out=None, var_num=None, stream=None):
        """One plane of decode_planes: int16 [nblk, 64] -> u8 [F, H, W] (same bound, per input domain)."""
        return self.decode_planes([coef], None if shape is None else [shape], None if out is None else [out],
                                  None if var_num is None else [var_num], stream)[0]


def stream_release(stream=None, diagnostic: bool = False) -> None:
    """The calling thread forgets `stream` (torch's current one by default) in the
    library's launch-isolation list (dctq_stream_release; call it before destroying the
    stream).  The product keeps no per-stream memory.  diagnostic=True:
    dctq_diag_stream_release -- wait for the stream and free the tie-path stashes
    this thread's v2 (variant 4) launches on it hold."""
    L = diag() if diagnostic else lib()
    fn = L.dctq_diag_stream_release if diagnostic else L.dctq_stream_release
    _check(fn(_stream_ptr(stream)), L)


def rle_encode(coef, stream=None):
    """Zigzag + run-length symbols of int16 blocks [N, 64] (src/entropy.c run_length_encode per
    block, concatenated).  Returns (offsets [N+1], symbols [total]) as int32 tensors holding the
    uint32 bit patterns: symbol = (uint16)value | run << 16.  Reads the total back (one sync)."""
    import torch
    _need(coef, 0, torch.int16, "coef")
    n = coef.numel() // 64
    ws = _workspace(lib().dctq_rle_workspace_bytes, n, coef.device)
    off = torch.empty(n + 1, dtype=torch.int32, device=coef.device)
    s = _stream_ptr(stream)
    _check(lib().dctq_rle_count(_ptr(coef), n, _ptr(off), _ptr(ws), s))
    total = _read_back(off[n:], stream)[0]
    sym = torch.empty(max(total, 1), dtype=torch.int32, device=coef.device)
    _check(lib().dctq_rle_emit(_ptr(coef), n, _ptr(off), _ptr(sym), s))
    return off, sym[:total]


def huffman_bits(coef, out=None, stream=None):
    """int16 [N, 64] quantized blocks -> int32 [N]: per block, the bits the reference's
    get_encoded_size reports after build_huffman_codes on that block's RLE symbols
    (tests/test_entropy.c:329-341)."""
    import torch
    _need(coef, 0, torch.int16, "coef")
    n = coef.numel() // 64
    out = _out(out, (n,), torch.int32, coef.device)
    _check(lib().dctq_huffman_bits(_ptr(coef), n, _ptr(out), _stream_ptr(stream)))
    return out


def psnr_u8(sse_sum, npixels) -> float:
    """PSNR in dB of a u8 picture from its summed squared error over npixels pixels:
    10 log10(255^2 npixels / sse_sum), inf for an exact picture.  Plain host arithmetic: reduce
    Plan.distortion_planes per plane, per frame or over a whole stack, then call this."""
    import math
    sse_sum, npixels = float(sse_sum), float(npixels)
    if sse_sum <= 0.0:
        return math.inf
    return 10.0 * math.log10(255.0 * 255.0 * npixels / sse_sum)


def rle_decode(symbols, offsets, out=None, stream=None):
    """Inverse of rle_encode / encode_planes: int16 [N, 64] blocks (run_length_decode +
    zigzag_to_block).  int16 symbols are the 2-byte format (dctq_rle_decode16)."""
    import torch
    n = offsets.numel() - 1
    out = _out(out, (n, 64), torch.int16, offsets.device)
    fn = lib().dctq_rle_decode16 if symbols.dtype == torch.int16 else lib().dctq_rle_decode
    _check(fn(_ptr(symbols), _ptr(offsets), n, _ptr(out), _stream_ptr(stream)))
    return out


def _need_symbols(symbols) -> int:
    """The symbols of a run-length stream: a contiguous int16 or int32 device tensor.  Returns
    the symbol format its dtype picks (2 or 4 bytes)."""
    import torch
    if not isinstance(symbols, torch.Tensor) or not symbols.is_cuda or symbols.dtype not in (torch.int16, torch.int32):
        raise DctqError("symbols must be an int16 or int32 tensor on a HIP device")
    if not symbols.is_contiguous():
        raise DctqError("symbols must be contiguous")
    return 2 if symbols.dtype == torch.int16 else 4


def _need_bytes(bytes) -> None:
    """The bytes of a packed stream: a contiguous uint8 device tensor."""
    import torch
    if not isinstance(bytes, torch.Tensor) or not bytes.is_cuda or bytes.dtype != torch.uint8:
        raise DctqError("bytes must be a uint8 tensor on a HIP device")
    if not bytes.is_contiguous():
        raise DctqError("bytes must be contiguous")


def _need_byte_offsets(offsets, nblk, bytes):
    """The offsets of a symbol or packed stream: a contiguous int32 device tensor of nblk + 1
    elements (nblk None: of any number of blocks), on the device of `bytes`."""
    import torch
    if (not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.dtype != torch.int32
            or not offsets.is_contiguous() or offsets.numel() < 2
            or (nblk is not None and offsets.numel() != nblk + 1)):
        want = "at least 2" if nblk is None else str(nblk + 1)
        raise DctqError(f"offsets must be a contiguous int32 device tensor of {want} elements "
                        "(one per block, plus one)")
    if offsets.device != bytes.device:
        raise DctqError("bytes and offsets must be on one device")


def bits_pack(symbols, offsets, symbol_bytes=None, capacity=None, stream=None):
    """Run-length symbols -> the bit-packed stream "bits v1" (dctq_bits_pack; the format:
    include/dct_amd.h, tools/bits_ref.py).  symbols / offsets as encode_planes or rle_encode
    return them (or anybody's: any int16 value, any run); symbols.dtype picks the format
    (int16: 2-byte, int32: 4-byte), and symbol_bytes, if given, must agree.  Returns
    (bytes uint8 [min(total, capacity)], byte_offsets int32 [N+1], uint32 bit patterns,
    always complete).  capacity None: two passes, the second sized by the first's total;
    0: the offsets only.  Reads the total back (one sync a pass)."""
    import torch
    sb = _need_symbols(symbols)
    if symbol_bytes is not None and int(symbol_bytes) != sb:
        raise DctqError(f"symbol_bytes {symbol_bytes} does not match symbols of {symbols.dtype}")
    _need_byte_offsets(offsets, None, symbols)
    if capacity is not None and int(capacity) < 0:
        raise DctqError("capacity must be >= 0")
    n = offsets.numel() - 1
    dev = symbols.device
    L = lib()
    ws = _workspace(L.dctq_bits_workspace_bytes, n, dev)
    boff = torch.empty(n + 1, dtype=torch.int32, device=dev)
    s = _stream_ptr(stream)

    def run(buf, cap):
        _check(L.dctq_bits_pack(_ptr(symbols), sb, _ptr(offsets), n, _ptr(boff), _ptr(buf), cap, _ptr(ws), s))
        return _read_back(boff[n:], stream)[0]

    cap = run(None, 0) if capacity is None else int(capacity)  # offsets only: the total
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=dev)
    total = run(out if cap else None, cap)
    return out[:min(total, cap)], boff


def bits_decode(bytes, offsets, out=None, stream=None):
    """Inverse of bits_pack, counterpart of rle_decode: int16 [N, 64] blocks from the packed
    stream (dctq_bits_decode).  Any bytes decode."""
    import torch
    _need_bytes(bytes)
    _need_byte_offsets(offsets, None, bytes)
    n = offsets.numel() - 1
    out = _out(out, (n, 64), torch.int16, bytes.device)
    _check(lib().dctq_bits_decode(_ptr(bytes), _ptr(offsets), n, _ptr(out), _stream_ptr(stream)))
    return out


def bits_window(bytes, offsets, shapes, windows, var_nums=None, stream=None):
    """A window of every plane of a "bits v1" stream as a stream of its own, without decoding
    (dctq_bits_window_offsets, dctq_bits_window_gather; tools/extract_ref.py window_stream gives
    the same bytes): the stored stream's blocks inside the windows, numbered as the window's own
    picture numbers them, so Plan.decode_bits(bytes', offsets', window shapes) is bit for bit
    Plan.decode_bits_window(bytes, offsets, shapes, windows).  bytes, offsets, shapes, windows and
    var_nums are as Plan.decode_bits_window takes them (var_nums[k] the whole stored plane's; any
    bytes, any non-decreasing offsets).  Returns (bytes' uint8 [total], offsets' int32 [N' + 1]
    holding uint32 bit patterns, var_nums': per-plane int32 views of one array, or None).  Reads
    the window's payload size back (one sync) and allocates exactly that."""
    import torch
    wins, wshapes, nbs = _stored_windows(shapes, windows)
    _need_bytes(bytes)
    _need_byte_offsets(offsets, sum(nbs), bytes)
    n, dev = len(wshapes), bytes.device
    if var_nums is not None:
        if len(var_nums) != n:
            raise DctqError(f"var_nums needs one entry per plane ({n}), got {len(var_nums)}")
        for k, v in enumerate(var_nums):
            _need(v, nbs[k], torch.int32, f"var_nums[{k}]", dev)
    exts = (_Extent * n)(*[_Extent(w, h, f) for f, h, w in wshapes])
    wnbs = [_nblocks(s) for s in wshapes]
    total_blocks = sum(wnbs)
    L, s = lib(), _stream_ptr(stream)
    ws = _workspace(L.dctq_bits_window_workspace_bytes, total_blocks, dev)
    woff = torch.empty(total_blocks + 1, dtype=torch.int32, device=dev)
    wvar = torch.empty(total_blocks, dtype=torch.int32, device=dev) if var_nums is not None else None
    _check(L.dctq_bits_window_offsets(_ptr(offsets), _ptrs(var_nums), wins, exts, n, _ptr(woff), _ptr(wvar),
                                      _ptr(ws), s), L)
    total = _read_back(woff[total_blocks:], stream)[0]
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    if total:
        _check(L.dctq_bits_window_gather(_ptr(bytes), _ptr(offsets), wins, exts, n, _ptr(woff), _ptr(out), total, s), L)
    return out, woff, (list(torch.split(wvar, wnbs)) if wvar is not None else None)


def bits_paste(bytes, offsets, shapes, windows, patch_bytes, patch_offsets, var_nums=None, patch_var_nums=None,
               stream=None):
    """A "bits v1" stream with a window of every plane replaced by another stream's blocks, without
    decoding: the inverse direction of bits_window (dctq_bits_paste_offsets, dctq_bits_paste_copy;
    tools/paste_ref.py paste_stream gives the same bytes).  bytes, offsets, shapes, windows and
    var_nums are as bits_window takes them; patch_bytes / patch_offsets / patch_var_nums are a stream
    of the windows' own pictures, numbered as bits_window numbers its result, so
    bits_paste(b, o, shapes, windows, *bits_window(b, o, shapes, windows)[:2]) is (b, o).  Block s of
    the result is the patch's block when s lies in its plane's window and the base's block s
    otherwise; lengths are exact differences of offsets.  var_nums and patch_var_nums are both given
    (one int32 tensor per plane each) or both None.  Returns (bytes' uint8 [total], offsets' int32
    [N + 1] holding uint32 bit patterns, var_nums': per-plane int32 views of one array, or None).
    The two payloads together must stay below 2^32 bytes (DctqError before anything is launched:
    the result's offsets are 32-bit).  Reads the result's payload size back (one sync) and allocates
    exactly that."""
    import torch
    wins, wshapes, nbs = _stored_windows(shapes, windows)
    wnbs = [_nblocks(s) for s in wshapes]
    _need_bytes(bytes)
    _need_byte_offsets(offsets, sum(nbs), bytes)
    _need_bytes(patch_bytes)
    _need_byte_offsets(patch_offsets, sum(wnbs), patch_bytes)
    n, dev = len(wshapes), bytes.device
    if patch_bytes.device != dev:
        raise DctqError("bytes and patch_bytes must be on one device")
    if (var_nums is None) != (patch_var_nums is None):
        raise DctqError("var_nums and patch_var_nums are both given or both None")
    if var_nums is not None:
        for name, vs, counts in (("var_nums", var_nums, nbs), ("patch_var_nums", patch_var_nums, wnbs)):
            if len(vs) != n:
                raise DctqError(f"{name} needs one entry per plane ({n}), got {len(vs)}")
            for k, v in enumerate(vs):
                _need(v, counts[k], torch.int32, f"{name}[{k}]", dev)
    if bytes.numel() + patch_bytes.numel() >= 1 << 32:
        raise DctqError("bits_paste: the two payloads together must stay below 2^32 bytes")
    exts = (_Extent * n)(*[_Extent(w, h, f) for f, h, w in wshapes])
    total_blocks = sum(nbs)
    L, s = lib(), _stream_ptr(stream)
    ws = _workspace(L.dctq_bits_paste_workspace_bytes, total_blocks, dev)
    ooff = torch.empty(total_blocks + 1, dtype=torch.int32, device=dev)
    ovar = torch.empty(total_blocks, dtype=torch.int32, device=dev) if var_nums is not None else None
    _check(L.dctq_bits_paste_offsets(_ptr(offsets), _ptrs(var_nums), _ptr(patch_offsets), _ptrs(patch_var_nums),
                                     bytes.numel(), patch_bytes.numel(), wins, exts, n, _ptr(ooff), _ptr(ovar),
                                     _ptr(ws), s), L)
    total = _read_back(ooff[total_blocks:], stream)[0]
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    if total:
        # an empty stream has no address: any non-NULL pointer stands for bytes that are never read
        _check(L.dctq_bits_paste_copy(_ptr(bytes if bytes.numel() else out), _ptr(offsets),
                                      _ptr(patch_bytes if patch_bytes.numel() else out), _ptr(patch_offsets), wins,
                                      exts, n, _ptr(ooff), _ptr(out), total, s), L)
    return out, ooff, (list(torch.split(ovar, nbs)) if ovar is not None else None)


def rgb_desc(t, bgr: bool = False):
    """Describe a uint8 device tensor [F, H, W, C] or [H, W, C] (channel axis last in the shape,
    C 3 or 4) as an RGB picture stack, without a copy.  Unit channel stride and a pixel stride of
    3 or 4 is interleaved RGB / RGBX (a contiguous HWC tensor); unit pixel stride is planar (e.g.
    chw.permute(0, 2, 3, 1) of a contiguous [F, 3, H, W] tensor: channel stride H * W); rows and
    frames may be padded.  bgr=True describes the same memory with R and B exchanged (BGR / BGRX,
    or the channel planes in reverse).  A stride that multiplies nothing is not looked at: a
    one-pixel-wide tensor whose channel stride is 1 is read as interleaved, and the row stride of
    a one-row tensor is taken as at least a row.  Strides the descriptor cannot express raise DctqError;
    alignment is the library's to check (include/dct_amd.h)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise DctqError("rgb must be a uint8 tensor")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[3] not in (3, 4):
        raise DctqError("rgb must be [H, W, C] or [F, H, W, C] with C 3 or 4 (channel axis last)")
    if not t.is_cuda:
        raise DctqError("rgb must be a tensor on a HIP device")
    f, h, w, c = t.shape
    sf, sh, sw, sc = t.stride()
    if w == 1 and sw == 1 and sc == 1:  # one column of adjacent R, G, B: the pixel stride means nothing
        sw = c
    if h == 1:                          # one row: neither does the row stride
        sh = max(sh, w * (1 if sw == 1 else sw))
    if sw == 1 and sc != 1:
        step, cs = 1, sc
    elif sc == 1 and sw in (3, 4) and c <= sw:
        step, cs = sw, 1
    else:
        raise DctqError(f"rgb strides {tuple(t.stride())} are neither interleaved (channel stride 1, pixel stride "
                        "3 or 4) nor planar (pixel stride 1)")
    if sh < w * step or (f > 1 and sf < sh * h):
        raise DctqError(f"rgb strides {tuple(t.stride())}: rows or frames overlap")
    ptr = t.data_ptr() + (2 * cs if bgr else 0)
    return _Rgb(ptr, sh, sf if f > 1 else sh * h, -cs if bgr else cs, step, w, h, f)


def _same_device(ts, what):
    import torch
    if any(not isinstance(t, torch.Tensor) for t in ts):
        raise DctqError(f"{what} must be tensors")
    if any(t.device != ts[0].device for t in ts):
        raise DctqError(f"{what} must be on one device")


def rgb_to_ycbcr(rgb, subsampling: str = "420", outs=None, bgr: bool = False, stream=None, pad: bool = False):
    """An RGB picture stack (rgb_desc(rgb, bgr)) -> (y, cb, cr) u8 planes in ONE launch
    (dctq_rgb_to_ycbcr_planes): y [F, H, W] and cb, cr [F, H/2, W/2] ("420") or [F, H, W]
    ("444"), ready for Plan.forward_quant_planes([y, cb, cr]) and Plan.encode_bits_planes.
    Exact integer BT.601 full range as tools/color_ref.py states it.  outs, if given, are the
    three u8 tensors and may be strided views (bytes outside width x height are not touched).
    pad=True (dctq_rgb_to_ycbcr_pad_planes) takes any size and any strides rgb_desc can express,
    at any alignment: the picture is extended by edge replication to H', W', the next multiples
    of 8 ("444") or 16 ("420"), and the planes are those of the extended picture
    (color_ref.forward_padded)."""
    import torch
    d = rgb_desc(rgb, bgr)
    if subsampling not in ("420", "444"):
        raise DctqError('subsampling must be "420" or "444"')
    sub = 2 if subsampling == "420" else 1
    m = 8 * sub
    if not pad and (d.width % m or d.height % m):
        raise DctqError(f"{subsampling}: width and height must be multiples of {8 * sub}, got {d.width} x {d.height}")
    eh, ew = -(-d.height // m) * m, -(-d.width // m) * m
    shapes = [(d.nframes, eh, ew)] + [(d.nframes, eh // sub, ew // sub)] * 2
    if outs is None:
        outs = [torch.empty(s_, dtype=torch.uint8, device=rgb.device) for s_ in shapes]
    if len(outs) != 3:
        raise DctqError(f"outs needs three planes (y, cb, cr), got {len(outs)}")
    _same_device([rgb, *outs], "rgb and outs")
    descs = [plane_desc(o) for o in outs]
    for name, p, want in zip(("y", "cb", "cr"), descs, shapes):
        if (p.nframes, p.height, p.width) != want:
            raise DctqError(f"outs: {name} is {(p.nframes, p.height, p.width)}, {subsampling} of rgb needs {want}")
    fn = lib().dctq_rgb_to_ycbcr_pad_planes if pad else lib().dctq_rgb_to_ycbcr_planes
    _check(fn(C.byref(d), C.byref(descs[0]), C.byref(descs[1]), C.byref(descs[2]), _stream_ptr(stream)))
    return tuple(outs)


def ycbcr_to_rgb(y, cb, cr, out=None, channels: int = 3, planar: bool = False, bgr: bool = False, stream=None,
                 size=None):
    """(y, cb, cr) u8 planes (4:2:0 or 4:4:4, read from their shapes) -> an RGB picture stack in
    ONE launch (dctq_ycbcr_to_rgb_planes), the exact integer inverse of tools/color_ref.py.
    out None: allocates u8 [F, H, W, channels] (channels 3 or 4; the fourth byte is 255), or with
    planar=True [F, 3, H, W], returned as its [F, H, W, 3] view.  Otherwise writes into out as
    rgb_desc(out, bgr) describes it (strided views are fine: padding is not touched).  bgr=True
    stores B where R would go and R where B would.  size=(H, W) crops
    (dctq_ycbcr_to_rgb_crop_planes; color_ref.inverse_cropped): the planes are those of a picture
    extended to whole blocks, only its H x W pixels are written, and out, if given, is H x W at
    any alignment."""
    import torch
    _same_device([y, cb, cr], "y, cb and cr")
    descs = [plane_desc(p) for p in (y, cb, cr)]
    f, h, w = descs[0].nframes, descs[0].height, descs[0].width
    if any(p.nframes != f for p in descs):
        raise DctqError("y, cb and cr differ in the number of frames")
    if size is not None:
        m = 8 if (descs[1].height, descs[1].width) == (h, w) else 16
        ch, cw = int(size[0]), int(size[1])
        if ch < 1 or cw < 1 or -(-ch // m) * m != h or -(-cw // m) * m != w:
            raise DctqError(f"size {(ch, cw)} rounded up to multiples of {m} is not y's {(h, w)}")
        h, w = ch, cw
    if out is None:
        if planar:
            out = torch.empty((f, 3, h, w), dtype=torch.uint8, device=y.device).permute(0, 2, 3, 1)
        elif channels in (3, 4):
            out = torch.empty((f, h, w, channels), dtype=torch.uint8, device=y.device)
        else:
            raise DctqError("channels must be 3 or 4")
    d = rgb_desc(out, bgr)
    _same_device([y, out], "the planes and out")
    if (d.nframes, d.height, d.width) != (f, h, w):
        raise DctqError(f"out is {(d.nframes, d.height, d.width)} (F, H, W), y is {(f, h, w)}")
    fn = lib().dctq_ycbcr_to_rgb_planes if size is None else lib().dctq_ycbcr_to_rgb_crop_planes
    _check(fn(C.byref(descs[0]), C.byref(descs[1]), C.byref(descs[2]), C.byref(d), _stream_ptr(stream)))
    return out


def pad_planes(planes, outs=None, stream=None):
    """1..4 u8 planes [F, H, W] / [H, W] of any size, strides and alignment -> their edge-padded
    copies of ceil(H / 8) 8 x ceil(W / 8) 8 in ONE launch (dctq_pad_planes): out(x, y) =
    plane(min(x, W - 1), min(y, H - 1)); a plane that is whole blocks already is copied.  outs, if
    given, are u8 tensors of the padded sizes (strided views are fine: bytes outside them are
    not touched).  Returns the list of padded planes, [F, H', W'] each."""
    import torch
    planes = list(planes)
    if not 1 <= len(planes) <= 4:
        raise DctqError("pad_planes needs 1..4 planes")
    _same_device(planes, "planes")
    src = [plane_desc(p) for p in planes]
    shapes = [(d.nframes, -(-d.height // 8) * 8, -(-d.width // 8) * 8) for d in src]
    if outs is None:
        outs = [torch.empty(s_, dtype=torch.uint8, device=planes[0].device) for s_ in shapes]
    if len(outs) != len(planes):
        raise DctqError(f"outs needs one tensor per plane ({len(planes)}), got {len(outs)}")
    _same_device([*planes, *outs], "planes and outs")
    dst = [plane_desc(o) for o in outs]
    for k, (d, want) in enumerate(zip(dst, shapes)):
        if (d.nframes, d.height, d.width) != want:
            raise DctqError(f"outs[{k}] is {(d.nframes, d.height, d.width)}, the padded plane is {want}")
    n = len(planes)
    _check(lib().dctq_pad_planes((_Plane * n)(*src), (_Plane * n)(*dst), n, _stream_ptr(stream)))
    return [o if o.dim() == 3 else o.unsqueeze(0) for o in outs]


# ---- the container "frame v1" (include/dct_amd.h, tools/frame_ref.py) -------------------------------
FRAME_MAGIC = b"DCTQFRM1"
FRAME_MAGIC_CROP = b"DCTQFRC1"   # the same with (pad_right | pad_bottom << 16) in each plane record's fourth word
_FRAME_MAX_BLOCKS = 11_671_106   # 368 * nblocks < 2^32, as dctq_bits_pack
_FRAME_HEAD = 48 + 16 * 4        # the longest header


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


def block_lengths(offsets, length_bytes=None, stream=None):
    """Byte offsets int32 [N+1] (uint32 bit patterns, as bits_pack returns them) -> (lengths,
    length_bytes): lengths[b] = offsets[b+1] - offsets[b] as uint8 [N] (length_bytes 1) or int16
    [N] holding uint16 bit patterns (2) (dctq_block_lengths).  length_bytes None tries 1, reads
    the largest length back (one sync) and reruns with 2 only when a block exceeds 255 B.  A
    length that does not fit length_bytes (above 65535 for None: no offsets of a packed stream)
    raises DctqError."""
    import torch
    _need_byte_offsets(offsets, None, offsets)
    if length_bytes is not None and int(length_bytes) not in (1, 2):
        raise DctqError("length_bytes must be 1, 2 or None")
    n = offsets.numel() - 1
    mx = torch.empty(1, dtype=torch.int32, device=offsets.device)
    for lb in ((1, 2) if length_bytes is None else (int(length_bytes),)):
        out = torch.empty(n, dtype=torch.uint8 if lb == 1 else torch.int16, device=offsets.device)
        _check(lib().dctq_block_lengths(_ptr(offsets), n, lb, _ptr(out), _ptr(mx), _stream_ptr(stream)))
        longest = _read_back(mx, stream)[0]
        if longest < 1 << (8 * lb):
            return out, lb
    raise DctqError(f"a block of {longest} bytes does not fit length_bytes {lb}")


def block_offsets(lengths, out=None, stream=None):
    """The inverse of block_lengths (dctq_block_offsets): int32 [N+1] exclusive prefix sums of
    min(length, 368), the last entry the total.  lengths.dtype picks the width: uint8 is 1,
    int16 or uint16 is 2."""
    import torch
    two = {torch.int16} | ({torch.uint16} if hasattr(torch, "uint16") else set())
    if not isinstance(lengths, torch.Tensor) or not lengths.is_cuda or lengths.dtype not in {torch.uint8} | two:
        raise DctqError("lengths must be a uint8, int16 or uint16 tensor on a HIP device")
    if not lengths.is_contiguous() or lengths.numel() < 1:
        raise DctqError("lengths must be contiguous and hold at least one block")
    n = lengths.numel()
    out = _out(out, (n + 1,), torch.int32, lengths.device)
    L = lib()
    ws = _workspace(L.dctq_block_offsets_workspace_bytes, n, lengths.device)
    _check(L.dctq_block_offsets(_ptr(lengths), 1 if lengths.dtype == torch.uint8 else 2, n, _ptr(out), _ptr(ws),
                                _stream_ptr(stream)))
    return out


def _frame_geometry(shapes, colour) -> int:
    """The plane records' rules of frame v1 for shapes [(F, H, W)]; returns nblocks."""
    if not 1 <= len(shapes) <= 4:
        raise DctqError("frame: nplanes must be 1..4")
    n = 0
    for f, h, w in shapes:
        if not _whole_blocks(f, h, w):
            raise DctqError(f"frame: plane {w} x {h} x {f}: width and height must be multiples of 8, nframes >= 1")
        n += _nblocks((f, h, w))
    if not 1 <= n <= _FRAME_MAX_BLOCKS:
        raise DctqError(f"frame: nblocks {n} outside 1..{_FRAME_MAX_BLOCKS}")
    if colour:
        if len(shapes) != 3:
            raise DctqError("frame: colour needs three planes")
        (f, h, w), cb, cr = shapes
        if cb != cr or cb[0] != f or ((cb[1], cb[2]) != (h, w) and (2 * cb[1], 2 * cb[2]) != (h, w)):
            raise DctqError("frame: colour needs chroma planes of 4:4:4 or 4:2:0 of plane 0")
    return n


def _frame_crops(crops, shapes, colour):
    """The rules of frame c1's fourth words for crops [(pad_bottom, pad_right)] per plane."""
    if len(crops) != len(shapes):
        raise DctqError("frame: crops needs one (pad_bottom, pad_right) per plane")
    for k, ((pb, pr), (_, h, w)) in enumerate(zip(crops, shapes)):
        most = 7
        if colour:
            most = 0 if k else (15 if shapes[1][1:] != shapes[0][1:] else 7)
        if not (0 <= pb <= most and 0 <= pr <= most) or pr >= w or pb >= h:
            raise DctqError(f"frame: plane {k}: pads {(pb, pr)} outside 0..{most} or not smaller than the plane")
    if not any(pb or pr for pb, pr in crops):
        raise DctqError("frame: the crop magic with no crop (that picture is frame v1)")


def _frame_sections(header_bytes, nblocks, length_bytes, adaptive, payload_bytes):
    """(starts, total): where the lengths, (var_num) and payload sections start, and the payload's end."""
    at, starts = header_bytes, []
    for size in [nblocks * length_bytes] + ([4 * nblocks] if adaptive else []) + [payload_bytes]:
        at = _align16(at)
        starts.append(at)
        at += size
    return starts, at


def _frame_header(head: bytes, buflen: int) -> dict:
    """The header of a frame v1 container of buflen bytes from its first min(buflen, 112) bytes,
    with everything that can be refused without the lengths refused (DctqError)."""
    import struct
    if buflen < 48 or len(head) < 48:
        raise DctqError("frame: shorter than the 48-byte fixed header")
    if head[:8] not in (FRAME_MAGIC, FRAME_MAGIC_CROP):
        raise DctqError("frame: bad magic")
    cropped = head[:8] == FRAME_MAGIC_CROP
    header_bytes, quality, adaptive, nplanes, length_bytes, colour = struct.unpack_from("<IBBBBB", head, 8)
    nblocks, payload_bytes, total = struct.unpack_from("<QQQ", head, 24)
    if not 1 <= quality <= 100 or adaptive > 1 or not 1 <= nplanes <= 4 or length_bytes not in (1, 2) or colour > 1:
        raise DctqError("frame: a header field is out of range")
    if any(head[17:24]):
        raise DctqError("frame: reserved bytes are not 0")
    if header_bytes != 48 + 16 * nplanes:
        raise DctqError("frame: header_bytes does not match nplanes")
    if buflen < header_bytes or len(head) < header_bytes:
        raise DctqError("frame: shorter than header_bytes")
    shapes, words = [], []
    for k in range(nplanes):
        w, h, f, word = struct.unpack_from("<IIII", head, 48 + 16 * k)
        if word and not cropped:
            raise DctqError("frame: a plane record's fourth word is not 0")
        shapes.append((f, h, w))
        words.append(word)
    if _frame_geometry(shapes, colour) != nblocks:
        raise DctqError("frame: nblocks does not match the plane records")
    crops = None
    if cropped:
        crops = [(word >> 16, word & 0xFFFF) for word in words]
        _frame_crops(crops, shapes, colour)
    if payload_bytes >= 1 << 32:
        raise DctqError("frame: payload_bytes must stay below 2^32")
    if buflen < total:
        raise DctqError("frame: shorter than total_bytes")
    starts, end = _frame_sections(header_bytes, nblocks, length_bytes, adaptive, payload_bytes)
    if end > total:
        raise DctqError("frame: a section ends past total_bytes")
    if end != total:
        raise DctqError("frame: total_bytes is not the end of the payload")
    return {"quality": quality, "adaptive": bool(adaptive), "colour": bool(colour), "length_bytes": length_bytes,
            "shapes": shapes, "nblocks": nblocks, "payload_bytes": payload_bytes, "starts": starts, "crops": crops}


def frame_pack(bytes, offsets, shapes, quality, adaptive=False, var_nums=None, colour=False, stream=None, crops=None,
               length_bytes=None):
    """A packed stream and what its decoder must know -> one uint8 device tensor, the container
    "frame v1" (include/dct_amd.h; tools/frame_ref.py pack gives the same bytes).  bytes / offsets
    as bits_pack or Plan.encode_bits_planes return them; shapes[k] is (F, H, W) or (H, W) of plane
    k; quality and adaptive the plan's (quality is clamped to 1..100 as the plan clamps it);
    var_nums (adaptive only) one int32 tensor per plane or one [N]; colour=True says the three
    planes are rgb_to_ycbcr's.  The header is built on the host, the sections are device copies
    into one allocation.  Reads the largest length and the total back (two syncs).  crops: per
    plane (pad_bottom, pad_right), the rows and columns of the stored plane to drop after decoding;
    with any of them non-zero the container is "frame c1" (magic DCTQFRC1), with None or all zero
    it is frame v1, byte for byte.  length_bytes None: 1 when every block is at most 255 B, else
    2 (as block_lengths chooses); 1 or 2 asks for that width (frame_concat keeps its sources' 2)."""
    import struct
    import torch
    _need_bytes(bytes)
    shapes = _shapes3(shapes)
    nblocks = _frame_geometry(shapes, colour)
    if crops is not None:
        crops = [(int(pb), int(pr)) for pb, pr in crops]
        if len(crops) != len(shapes) or any(pb or pr for pb, pr in crops):
            _frame_crops(crops, shapes, colour)   # which refuses a wrong count first
        else:
            crops = None
    _need_byte_offsets(offsets, nblocks, bytes)
    dev = bytes.device
    sections = []
    lengths, lb = block_lengths(offsets, length_bytes, stream=stream)
    sections.append(lengths.view(torch.uint8))
    first, total = _read_back(offsets[[0, nblocks]], stream)
    if first != 0 or total != bytes.numel():
        raise DctqError(f"offsets run from {first} to {total}, bytes holds {bytes.numel()}")
    if adaptive:
        if var_nums is None:
            raise DctqError("an adaptive container needs var_nums")
        vn = torch.cat([v.reshape(-1) for v in var_nums]) if isinstance(var_nums, (list, tuple)) else var_nums
        sections.append(_need(vn, nblocks, torch.int32, "var_nums", dev)[:nblocks].view(torch.uint8))
    sections.append(bytes)
    header_bytes = 48 + 16 * len(shapes)
    starts, end = _frame_sections(header_bytes, nblocks, lb, bool(adaptive), bytes.numel())
    head = bytearray(FRAME_MAGIC if crops is None else FRAME_MAGIC_CROP)
    head += struct.pack("<IBBBBB7xQQQ", header_bytes, _clamp_quality(quality), int(bool(adaptive)), len(shapes),
                        lb, int(bool(colour)), nblocks, bytes.numel(), end)
    for (f, h, w), (pb, pr) in zip(shapes, crops or [(0, 0)] * len(shapes)):
        head += struct.pack("<IIII", w, h, f, pr | pb << 16)
    out = torch.empty(end, dtype=torch.uint8, device=dev)
    with _on_stream(stream):
        out[:header_bytes].copy_(torch.frombuffer(head, dtype=torch.uint8))
        for at, sec in zip(starts, sections):
            out[at:at + sec.numel()].copy_(sec)
            out[at + sec.numel():min(_align16(at + sec.numel()), end)].zero_()
    return out


def frame_unpack(buf, stream=None) -> dict:
    """A frame v1 container -> its parts, everything checked on the host before anything is
    decoded (DctqError for every rule of the format's refusal list).  buf: a uint8 device tensor,
    or anything host-side with the buffer protocol (bytes, bytearray, a numpy array), which is
    uploaded; a device tensor that does not start on a 16-byte boundary is copied first.  The
    header is read back from the first 112 bytes at most; the offsets are rebuilt on the device
    (block_offsets) and their total compared with payload_bytes (two syncs in all).  Returns a
    dict: quality, adaptive, colour, shapes [(F, H, W)], offsets int32 [N+1], bytes (the whole
    payload, a view into buf: what Plan.decode_bits takes with offsets) and var_nums (adaptive:
    a list of int32 views into buf, one per plane; else None), and crops: None for frame v1, for
    frame c1 the list of (pad_bottom, pad_right) per plane."""
    return _frame_parts(*_frame_open(buf, stream), stream)


def _frame_open(buf, stream):
    """frame_unpack's first half: buf on the device, and its header checked on the host
    (_frame_header) -> (buf, h).  Nothing is launched but the copies."""
    import torch
    if isinstance(buf, torch.Tensor):
        if not buf.is_cuda or buf.dtype != torch.uint8 or buf.dim() != 1:
            raise DctqError("buf must be a one-dimensional uint8 tensor on a HIP device, or a host buffer")
        with _on_stream(stream):
            if not buf.is_contiguous() or buf.data_ptr() % 16:
                buf = buf.clone(memory_format=torch.contiguous_format)
    else:
        host = bytearray(memoryview(buf).cast("B"))
        if len(host) < 48:
            raise DctqError("frame: shorter than the 48-byte fixed header")
        with _on_stream(stream):
            buf = torch.frombuffer(host, dtype=torch.uint8).to("cuda")
    if buf.numel() < 48:
        raise DctqError("frame: shorter than the 48-byte fixed header")
    with _on_stream(stream):
        head = buf[:_FRAME_HEAD].cpu().numpy().tobytes()
    return buf, _frame_header(head, buf.numel())


def _frame_parts(buf, h, stream):
    """frame_unpack's second half: the offsets rebuilt on the device and the sections as views."""
    import torch
    n, lb, starts = h["nblocks"], h["length_bytes"], h["starts"]
    lengths = buf[starts[0]:starts[0] + n * lb]
    offsets = block_offsets(lengths if lb == 1 else lengths.view(torch.int16), stream=stream)
    total = _read_back(offsets[n:], stream)[0]
    if total != h["payload_bytes"]:
        raise DctqError(f"frame: the lengths sum to {total}, payload_bytes says {h['payload_bytes']}")
    var_nums = None
    if h["adaptive"]:
        vn = buf[starts[1]:starts[1] + 4 * n].view(torch.int32)
        var_nums = list(torch.split(vn, [_nblocks(s) for s in h["shapes"]]))
    return {"quality": h["quality"], "adaptive": h["adaptive"], "colour": h["colour"], "shapes": h["shapes"],
            "length_bytes": lb, "offsets": offsets, "bytes": buf[starts[-1]:starts[-1] + h["payload_bytes"]],
            "var_nums": var_nums, "crops": h["crops"]}


_frame_plans = {}


def _frame_plan(quality: int, adaptive: bool, device) -> "Plan":
    """compress / decompress keep one Plan per (quality, adaptive, device) and library (grid_limit)."""
    import torch
    key = (_clamp_quality(quality), bool(adaptive), torch.device(device).index or 0, _grid_limited)
    if key not in _frame_plans:
        with torch.cuda.device(key[2]):
            _frame_plans[key] = Plan(key[0], key[1])
    return _frame_plans[key]


def compress(src, quality: int = 50, adaptive: bool = False, subsampling: str = "420", bgr: bool = False, stream=None):
    """Pixels -> one self-contained uint8 device tensor (frame v1) that decompress turns back
    into pixels with nothing else to remember.  src: an RGB stack as rgb_desc takes it (through
    rgb_to_ycbcr with `subsampling` and `bgr`; the container says colour), or a list of 1..4 u8
    planes [F, H, W] / [H, W] (plain planes).  Non-adaptive plans run Plan.encode_bits_planes;
    adaptive ones forward_quant_planes into one coefficient and one var_num buffer, rle_encode and
    bits_pack, because the decoder needs the var_num of every block.
    A source whose sides are not whole blocks (multiples of 8; of 16 for a 4:2:0 picture) is
    edge-padded on the way in (rgb_to_ycbcr(pad=True), pad_planes) and the container is "frame
    c1", which records what decompress crops; every other source takes the unpadded path and
    gives frame v1."""
    import torch
    colour = isinstance(src, torch.Tensor)
    if colour:
        d = rgb_desc(src, bgr)
        m = 16 if subsampling == "420" else 8
        crops = [(-d.height % m, -d.width % m), (0, 0), (0, 0)]
        planes = list(rgb_to_ycbcr(src, subsampling, bgr=bgr, stream=stream, pad=any(crops[0])))
    else:
        planes = list(src)
        if not 1 <= len(planes) <= 4:
            raise DctqError("compress needs an RGB stack or a list of 1..4 planes")
        _same_device(planes, "planes")
        crops = [(-d.height % 8, -d.width % 8) for d in map(plane_desc, planes)]
        if any(pb or pr for pb, pr in crops):
            planes = pad_planes(planes, stream=stream)
    descs = [plane_desc(p) for p in planes]
    shapes = [(d.nframes, d.height, d.width) for d in descs]
    plan = _frame_plan(quality, adaptive, planes[0].device)
    var_nums = None
    if adaptive:
        nbs = [_nblocks(s) for s in shapes]
        coef = torch.empty((sum(nbs), 64), dtype=torch.int16, device=planes[0].device)
        var_nums = torch.empty(sum(nbs), dtype=torch.int32, device=planes[0].device)
        plan.forward_quant_planes(planes, outs=list(torch.split(coef, nbs)), var_nums=list(torch.split(var_nums, nbs)),
                                  stream=stream)
        off, sym = rle_encode(coef, stream=stream)
        packed, boff = bits_pack(sym, off, stream=stream)
    else:
        _, boff, packed = plan.encode_bits_planes(planes, stream=stream)
    return frame_pack(packed, boff, shapes, plan.quality, adaptive, var_nums, colour, stream=stream, crops=crops)


def _pair(r, what):
    """(a, b) as two ints, or DctqError."""
    try:
        a, b = r
        return int(a), int(b)
    except (TypeError, ValueError):
        raise DctqError(f"{what} must be a pair of integers, got {r!r}") from None


def _region_windows(shapes, crops, colour, region, frames):
    """decompress's region arithmetic, on the host: the stored shapes [(F, H, W)] and crops
    [(pad_bottom, pad_right)] or None of a container, a region in pixels of the TRUE picture
    (or None: all of it; plain planes: one region, or a list of one per plane) and frames
    (f0, f1) or None -> (windows, cuts): windows[k] = ((f0, f1), (Y0, Y1), (X0, X1)) of stored
    plane k for Plan.decode_bits_window, the region grown to multiples of m (8; 16 in the luma
    of a 4:2:0 picture, whose chroma windows are half of it), and cuts[k] = (dy, dx, h, w):
    where the region sits inside the window's picture (colour: one cut, the picture's).
    DctqError for a region or frame range that is empty or leaves the true picture, and for
    anything else that is not what the container's kind takes."""
    crops = crops or [(0, 0)] * len(shapes)
    true = [(h - pb, w - pr) for (_, h, w), (pb, pr) in zip(shapes, crops)]
    nf = min(f for f, _, _ in shapes)
    f0, f1 = (0, nf) if frames is None else _pair(frames, "frames")
    if not 0 <= f0 < f1 <= nf:
        raise DctqError(f"frames {(f0, f1)} is empty or outside the {nf} frames")
    npic = 1 if colour else len(shapes)
    if region is None:
        regions = [((0, h), (0, w)) for h, w in true[:npic]]
    else:
        try:
            single = not hasattr(region[0][0], "__len__")
        except (TypeError, IndexError):
            raise DctqError("region must be ((y0, y1), (x0, x1))" + ("" if colour else ", or a list of one per plane")) from None
        if single:
            if len(set(true[:npic])) != 1:
                raise DctqError("the planes differ in size: region must be a list of one region per plane")
            regions = [region] * npic
        elif colour or len(region) != npic:
            raise DctqError(f"region must be ((y0, y1), (x0, x1))" + ("" if colour else f", or a list of {npic} of them"))
        else:
            regions = list(region)
    sub = 2 if colour and shapes[1][1:] != shapes[0][1:] else 1
    m = 8 * sub
    windows, cuts = [], []
    for k, (r, (th, tw)) in enumerate(zip(regions, true)):
        if not hasattr(r, "__len__") or len(r) != 2:
            raise DctqError(f"region {r!r} must be ((y0, y1), (x0, x1))")
        (y0, y1), (x0, x1) = _pair(r[0], "a region's rows"), _pair(r[1], "a region's columns")
        if not (0 <= y0 < y1 <= th and 0 <= x0 < x1 <= tw):
            raise DctqError(f"region {((y0, y1), (x0, x1))} is empty or outside the picture of {th} x {tw}")
        ya, xa = y0 // m * m, x0 // m * m
        yb, xb = -(-y1 // m) * m, -(-x1 // m) * m   # inside the stored plane: it is whole multiples of m
        windows.append(((f0, f1), (ya, yb), (xa, xb)))
        cuts.append((y0 - ya, x0 - xa, y1 - y0, x1 - x0))
    if colour:
        (_, (ya, yb), (xa, xb)) = windows[0]
        windows += [((f0, f1), (ya // sub, yb // sub), (xa // sub, xb // sub))] * 2
    return windows, cuts


def _decompress_scaled(d, plan, scale, frames, channels, planar, bgr, stream):
    """decompress(scale=): the parts d of a container at 1 / scale size."""
    import torch
    windows, cuts = _region_windows(d["shapes"], d["crops"], d["colour"], None, frames)
    small = [(-(-h // scale), -(-w // scale)) for _, _, h, w in cuts]   # of the TRUE sizes
    kw = dict(var_nums=d["var_nums"], stream=stream)
    if not d["colour"]:
        outs = plan.decode_bits_scaled(d["bytes"], d["offsets"], d["shapes"], scale, windows, **kw)
        return [o[:, :h, :w] for o, (h, w) in zip(outs, small)]
    # Y, Cb, Cr into the top-left of planes of whole blocks, which is what ycbcr_to_rgb(size=) takes:
    # the reduced chroma is exactly half the reduced luma, and a pixel inside `small` reads only
    # bytes that were decoded (ceil(H / scale) <= stored H / scale)
    sub = 2 if d["shapes"][1][1:] != d["shapes"][0][1:] else 1
    m = 8 * sub
    bh, bw = -(-small[0][0] // m) * m, -(-small[0][1] // m) * m
    (f0, f1) = windows[0][0]
    with _on_stream(stream):
        bufs = [torch.empty((f1 - f0, bh // c, bw // c), dtype=torch.uint8, device=d["bytes"].device)
                for c in (1, sub, sub)]
    outs = [b[:, :(y1 - y0) // scale, :(x1 - x0) // scale] for b, (_, (y0, y1), (x0, x1)) in zip(bufs, windows)]
    plan.decode_bits_scaled(d["bytes"], d["offsets"], d["shapes"], scale, windows, outs=outs, **kw)
    return ycbcr_to_rgb(*bufs, channels=channels, planar=planar, bgr=bgr, stream=stream, size=small[0])


def decompress(buf, channels: int = 3, planar: bool = False, bgr: bool = False, stream=None, region=None, frames=None,
               scale=None):
    """The inverse of compress: frame_unpack, the container's plan, Plan.decode_bits and, for a
    colour container, ycbcr_to_rgb (channels / planar / bgr as there).  Returns the RGB stack
    [F, H, W, channels] for a colour container, the list of u8 planes [F, H, W] otherwise.
    Nothing is decoded from a container that frame_unpack refuses.  A frame c1 container comes
    back at its true size: the picture through ycbcr_to_rgb(size=(H, W)); plain planes as the
    [:, :H, :W] VIEWS of the decoded (padded) planes, which are therefore not contiguous.
    region=((y0, y1), (x0, x1)), in pixels of the TRUE picture at any alignment, and / or
    frames=(f0, f1), both half-open: only that part, byte for byte decompress(buf, ...)[f0:f1,
    y0:y1, x0:x1], for frame v1 and frame c1 alike, decoded from the blocks it needs and no
    others (Plan.decode_bits_window over the enclosing window of whole blocks -- of 16 x 16
    luma pixels for a 4:2:0 picture; chroma upsampling is nearest neighbour, so the window
    converts exactly as the whole picture does).  The result may be a VIEW into the window's
    picture (a region that does not start on a block), so it need not be contiguous.  Plain
    planes take one region when all planes have one true size, else a list of one region per
    plane; frames must lie inside every plane's.  A region or frame range that is empty or
    leaves the true picture raises DctqError before anything is decoded.  With neither given
    the path and the result are those described first.
    scale=2, 4 or 8 (optionally with frames): the pictures at 1 / scale size, decoded at that
    size from the stream (Plan.decode_bits_scaled; include/dct_amd.h defines the pixels), for
    frame v1 and frame c1 alike: plain planes as [F, ceil(H / scale), ceil(W / scale)] views, H
    and W the TRUE size; a colour container as the RGB stack of that size, converted from the
    reduced Y, Cb and Cr as every picture is.  scale together with region raises DctqError
    (Plan.decode_bits_scaled takes windows), and so does any other scale."""
    if scale is not None:
        _log2_scale(scale)
        if region is not None:
            raise DctqError("decompress: scale together with region is not supported "
                            "(Plan.decode_bits_scaled takes windows)")
    d = frame_unpack(buf, stream=stream)
    if d["offsets"] is not None and not d["bytes"].numel():
        # a container of empty blocks (frame_blank): an empty tensor has no address and the decoders
        # take no NULL, so four bytes of the offsets stand for a payload of which none is read
        import torch
        d = dict(d, bytes=d["offsets"].view(torch.uint8)[:4])
    plan = _frame_plan(d["quality"], d["adaptive"], d["bytes"].device)
    crops = d["crops"]
    if scale is not None:
        return _decompress_scaled(d, plan, scale, frames, channels, planar, bgr, stream)
    if region is not None or frames is not None:
        windows, cuts = _region_windows(d["shapes"], crops, d["colour"], region, frames)
        outs = plan.decode_bits_window(d["bytes"], d["offsets"], d["shapes"], windows, var_nums=d["var_nums"],
                                       stream=stream)
        if not d["colour"]:
            return [o[:, dy:dy + h, dx:dx + w] for o, (dy, dx, h, w) in zip(outs, cuts)]
        dy, dx, h, w = cuts[0]
        whole = (dy + h, dx + w) == tuple(outs[0].shape[1:])
        rgb = ycbcr_to_rgb(*outs, channels=channels, planar=planar, bgr=bgr, stream=stream,
                           size=None if whole else (dy + h, dx + w))
        return rgb[:, dy:, dx:] if dy or dx else rgb
    outs = plan.decode_bits(d["bytes"], d["offsets"], shapes=d["shapes"], var_nums=d["var_nums"], stream=stream)
    if not d["colour"]:
        if crops is None:
            return outs
        return [o[:, :o.shape[1] - pb, :o.shape[2] - pr] for o, (pb, pr) in zip(outs, crops)]
    size = None if crops is None else (outs[0].shape[1] - crops[0][0], outs[0].shape[2] - crops[0][1])
    return ycbcr_to_rgb(*outs, channels=channels, planar=planar, bgr=bgr, stream=stream, size=size)


def _window_crops(shapes, crops, colour, region, frames):
    """frame_window's region arithmetic, on the host: decompress's (_region_windows), with the one
    rule a stream adds -- a region starts on a multiple of m (8; 16 for a 4:2:0 picture), since a
    stream cannot begin inside a block -> (windows, wshapes, crops'): the stored windows, their own
    (F, H, W), and what the new container records, (window height - region height, window width -
    region width) on plane 0 of a picture or per plane for plain planes, (0, 0) elsewhere."""
    windows, cuts = _region_windows(shapes, crops, colour, region, frames)
    m = 16 if colour and shapes[1][1:] != shapes[0][1:] else 8
    if any(dy or dx for dy, dx, _, _ in cuts):
        raise DctqError(f"frame_window: a region must start on multiples of {m} (a stream cannot begin inside a "
                        f"block), got rows and columns from {[(w[1][0] + c[0], w[2][0] + c[1]) for w, c in zip(windows, cuts)]}")
    wshapes = [(f1 - f0, y1 - y0, x1 - x0) for (f0, f1), (y0, y1), (x0, x1) in windows]
    new = [(wh - h, ww - w) for (_, wh, ww), (_, _, h, w) in zip(wshapes, cuts)]
    return windows, wshapes, new + [(0, 0)] * (len(shapes) - len(new))


def frame_window(buf, region=None, frames=None, stream=None):
    """A region and / or a frame range of a container (frame v1 or frame c1) as a container of its
    own, without decoding: frame_unpack, decompress's region arithmetic, bits_window, frame_pack
    (tools/extract_ref.py frame_window gives the same bytes).  Quality, adaptive and colour are
    carried over; length_bytes is chosen from the window's own blocks.  region=((y0, y1), (x0,
    x1)) in pixels of the TRUE picture (plain planes: one region, or a list of one per plane),
    frames=(f0, f1), both half-open, as for decompress -- but a region must START on multiples of
    m (8; 16 for a 4:2:0 picture), or DctqError is raised before anything is launched.  It may end
    anywhere inside the true picture: the window is grown to multiples of m, and the new container
    records the difference as its crop (frame c1; frame v1 when there is none).  Lossless:
    decompress(frame_window(buf, region, frames), ...) is byte for byte decompress(buf,
    region=region, frames=frames, ...), and where the region ends on multiples of m or on the true
    picture's edge, frame_window(compress(x, ...), region, frames) is byte for byte
    compress(x[f0:f1, y0:y1, x0:x1], ...)."""
    buf, h = _frame_open(buf, stream)
    windows, wshapes, crops = _window_crops(h["shapes"], h["crops"], h["colour"], region, frames)
    d = _frame_parts(buf, h, stream)
    packed, off, var = bits_window(d["bytes"], d["offsets"], d["shapes"], windows, d["var_nums"], stream=stream)
    return frame_pack(packed, off, wshapes, d["quality"], d["adaptive"], var, d["colour"], stream=stream, crops=crops)


def frame_concat(bufs, stream=None):
    """Two or more containers joined along the frame axis, without decoding: the inverse of
    frame_window(frames=) (tools/extract_ref.py frame_concat gives the same bytes).  The sources
    must agree in quality, adaptive, colour, the number of planes, every plane's stored (H, W) and
    crops, else DctqError; so do more than 11 671 106 blocks or a payload of 2^32 bytes or more.
    Blocks are numbered plane by plane, so plane k of the result is plane k of each source in turn,
    in the lengths, var_num and payload sections alike: device slices and copies, with the plane
    boundaries' offsets read back (one sync a source).  length_bytes is 2 if any source's is 2.
    frame_concat([frame_window(b, frames=(0, a)), frame_window(b, frames=(a, F))]) is b byte for
    byte for any b that compress wrote, and frame_concat([compress(x[:a]), compress(x[a:])]) is
    compress(x)."""
    import torch
    bufs = list(bufs)
    if len(bufs) < 2:
        raise DctqError("frame_concat needs two or more containers")
    ds = [frame_unpack(b, stream=stream) for b in bufs]
    a = ds[0]
    for i, d in enumerate(ds[1:], 1):
        for key in ("quality", "adaptive", "colour", "crops"):
            if d[key] != a[key]:
                raise DctqError(f"frame_concat: container {i} differs from container 0 in {key}: {d[key]} != {a[key]}")
        if len(d["shapes"]) != len(a["shapes"]) or [s[1:] for s in d["shapes"]] != [s[1:] for s in a["shapes"]]:
            raise DctqError(f"frame_concat: container {i} differs from container 0 in its planes' stored sizes")
        if d["bytes"].device != a["bytes"].device:
            raise DctqError("frame_concat: the containers must be on one device")
    nplanes = len(a["shapes"])
    shapes = [(sum(d["shapes"][k][0] for d in ds), *a["shapes"][k][1:]) for k in range(nplanes)]
    nblocks = sum(_nblocks(s) for s in shapes)
    if nblocks > _FRAME_MAX_BLOCKS:
        raise DctqError(f"frame_concat: {nblocks} blocks, a container holds at most {_FRAME_MAX_BLOCKS}")
    if sum(d["bytes"].numel() for d in ds) >= 1 << 32:
        raise DctqError("frame_concat: the payload must stay below 2^32 bytes")
    # each source's plane boundaries: block numbers, and their byte offsets read back
    firsts, cuts = [], []
    for d in ds:
        first = [0]
        for s in d["shapes"]:
            first.append(first[-1] + _nblocks(s))
        firsts.append(first)
        cuts.append(_read_back(d["offsets"][first], stream))
    offs, pays, base = [], [], 0
    with _on_stream(stream):
        for k in range(nplanes):
            for d, first, cut in zip(ds, firsts, cuts):
                shift = (base - cut[k]) & 0xFFFFFFFF    # uint32 arithmetic in int32 bit patterns
                offs.append(d["offsets"][first[k]:first[k + 1]] + (shift - (1 << 32) if shift >> 31 else shift))
                pays.append(d["bytes"][cut[k]:cut[k + 1]])
                base += cut[k + 1] - cut[k]
        offs.append(torch.tensor([base - (1 << 32) if base >> 31 else base], dtype=torch.int32, device=offs[0].device))
        off, packed = torch.cat(offs), torch.cat(pays)
        var = None
        if a["adaptive"]:
            var = torch.cat([d["var_nums"][k] for k in range(nplanes) for d in ds])
    return frame_pack(packed, off, shapes, a["quality"], a["adaptive"], var, a["colour"], stream=stream, crops=a["crops"],
                      length_bytes=max(d["length_bytes"] for d in ds))


def _paste_windows(b, p, at, frame):
    """frame_paste's host rules (tools/paste_ref.py paste_windows): the headers b of the base and p
    of the patch, `at` and `frame` -> the stored windows of the base, one per plane; DctqError for
    anything frame_paste refuses."""
    for key in ("quality", "adaptive", "colour"):
        if b[key] != p[key]:
            raise DctqError(f"frame_paste: the patch differs from the container in {key}: {p[key]} != {b[key]}")
    shapes, pshapes, colour = b["shapes"], p["shapes"], b["colour"]
    sub = 2 if colour and shapes[1][1:] != shapes[0][1:] else 1
    if len(pshapes) != len(shapes) or (colour and (2 if pshapes[1][1:] != pshapes[0][1:] else 1) != sub):
        raise DctqError("frame_paste: the patch differs from the container in its planes or subsampling")
    crops = b["crops"] or [(0, 0)] * len(shapes)
    pcrops = p["crops"] or [(0, 0)] * len(shapes)
    npic = 1 if colour else len(shapes)
    m = 8 * sub
    true = [(h - pb, w - pr) for (_, h, w), (pb, pr) in zip(shapes, crops)][:npic]
    try:
        single = not hasattr(at[0], "__len__")
    except (TypeError, IndexError):
        raise DctqError("at must be (y, x)" + ("" if colour else ", or a list of one per plane")) from None
    if single:
        if len(set(true)) != 1:
            raise DctqError("the planes differ in size: at must be a list of one (y, x) per plane")
        ats = [_pair(at, "at")] * npic
    elif colour or len(at) != npic:
        raise DctqError("at must be (y, x)" + ("" if colour else f", or a list of {npic} of them"))
    else:
        ats = [_pair(a, "at") for a in at]
    frame = int(frame)
    windows = []
    for k, ((y, x), (th, tw)) in enumerate(zip(ats, true)):
        if y < 0 or x < 0 or y % m or x % m:
            raise DctqError(f"frame_paste: at must be non-negative multiples of {m} (a stream cannot begin inside a "
                            f"block), got {(y, x)}")
        pf, ph, pw = pshapes[k]
        if frame < 0 or frame + pf > shapes[k][0]:
            raise DctqError(f"frame_paste: frames {(frame, frame + pf)} leave the {shapes[k][0]} frames")
        for axis, a0, stored, pad, t in (("rows", y, ph, pcrops[k][0], th), ("columns", x, pw, pcrops[k][1], tw)):
            if not ((pad == 0 and a0 + stored <= t) or a0 + stored - pad == t):
                raise DctqError(f"frame_paste: plane {k}: the patch's {axis} {(a0, a0 + stored - pad)} must end inside "
                                f"the true picture of {t} without a crop, or exactly on its edge: anything else would "
                                "write replicated edge pixels over real ones")
        windows.append(((frame, frame + pf), (y, y + ph), (x, x + pw)))
    if colour:
        (fr, (ya, yb), (xa, xb)) = windows[0]
        windows += [(fr, (ya // sub, yb // sub), (xa // sub, xb // sub))] * 2
    return windows


def frame_paste(buf, patch, at=(0, 0), frame: int = 0, stream=None):
    """The container buf with the container patch written in, without decoding either: the inverse
    of frame_window (frame_unpack of both, bits_paste, frame_pack; tools/paste_ref.py frame_paste
    gives the same bytes).  at=(y, x): where the patch's first pixel goes, in pixels of buf's TRUE
    picture (plain planes: one pair when every plane has one true size, or a list of one per
    plane); frame: the first frame it replaces.  The result has buf's geometry and crops;
    length_bytes is chosen from the result's own blocks.  Refused with DctqError before anything
    is launched: a patch that differs in quality, adaptive, colour, the number of planes or the
    subsampling; at that is not multiples of m (8; 16 for a 4:2:0 picture); frame + the patch's
    frames beyond buf's; and, on each axis, a patch that neither has no crop and ends inside the
    true picture, nor has its TRUE extent end exactly on the true picture's edge (then its padded
    rows and columns are exactly what compress of the edited picture writes there) -- anything
    else would write replicated edge pixels over real ones.
    frame_paste(b, frame_window(b, region, frames), at=the region's start, frame=frames[0]) is b
    byte for byte, frame_paste(compress(x), compress(p), at, f) is compress(x with p written in),
    and decompress of the result is decompress(buf) with decompress(patch) written in: the blocks
    that are not replaced keep their bytes, so nothing goes through a second generation."""
    buf, hb = _frame_open(buf, stream)
    patch, hp = _frame_open(patch, stream)
    if patch.device != buf.device:
        raise DctqError("frame_paste: the containers must be on one device")
    windows = _paste_windows(hb, hp, at, frame)
    d, p = _frame_parts(buf, hb, stream), _frame_parts(patch, hp, stream)
    packed, off, var = bits_paste(d["bytes"], d["offsets"], d["shapes"], windows, p["bytes"], p["offsets"],
                                  d["var_nums"], p["var_nums"], stream=stream)
    return frame_pack(packed, off, d["shapes"], d["quality"], d["adaptive"], var, d["colour"], stream=stream,
                      crops=d["crops"])


def frame_blank(shapes, quality, adaptive=False, colour=False, crops=None, device="cuda", stream=None):
    """A container of the stored shapes [(F, H, W)] whose every block has length 0 and, for an
    adaptive plan, var_num 0 (tools/paste_ref.py frame_blank gives the same bytes).  An empty block
    is valid bits v1 and decodes as zero coefficients, so the container decompresses to flat
    mid-grey; it is what frame_tile pastes into.  quality, adaptive, colour and crops as frame_pack."""
    import torch
    shapes = _shapes3(shapes)
    n = _frame_geometry(shapes, colour)
    with _on_stream(stream):
        off = torch.zeros(n + 1, dtype=torch.int32, device=device)
        var = torch.zeros(n, dtype=torch.int32, device=device) if adaptive else None
        packed = torch.empty(0, dtype=torch.uint8, device=device)
    return frame_pack(packed, off, shapes, quality, adaptive, var, colour, stream=stream, crops=crops)


def _tile_layout(hs):
    """frame_tile's host rules (tools/paste_ref.py tile_layout): the grid of headers -> (shapes,
    crops, ats): the joined container's stored shapes and crops, and each tile's `at`."""
    rows, cols = len(hs), len(hs[0]) if hs else 0
    if rows < 1 or cols < 1 or any(len(row) != cols for row in hs):
        raise DctqError("frame_tile: a grid of one or more rows of equal length")
    a = hs[0][0]
    colour, n = a["colour"], len(a["shapes"])
    sub = 2 if colour and a["shapes"][1][1:] != a["shapes"][0][1:] else 1
    for row in hs:
        for h in row:
            for key in ("quality", "adaptive", "colour"):
                if h[key] != a[key]:
                    raise DctqError(f"frame_tile: the containers differ in {key}: {h[key]} != {a[key]}")
            if (len(h["shapes"]) != n or (colour and (2 if h["shapes"][1][1:] != h["shapes"][0][1:] else 1) != sub)
                    or [s[0] for s in h["shapes"]] != [s[0] for s in a["shapes"]]):
                raise DctqError("frame_tile: the containers differ in their planes, subsampling or frames")
    npic = 1 if colour else n

    def true(h, k):
        (_, hh, ww), (pb, pr) = h["shapes"][k], (h["crops"] or [(0, 0)] * n)[k]
        return hh - pb, ww - pr, pb, pr

    shapes, crops, ys, xs = [], [], [], []
    for k in range(npic):
        for r, row in enumerate(hs):
            if len({true(h, k)[0] for h in row}) != 1:
                raise DctqError(f"frame_tile: plane {k}: true heights differ along row {r}")
            if r < rows - 1 and any(true(h, k)[2] for h in row):
                raise DctqError("frame_tile: only the last row may carry a bottom crop")
        for c in range(cols):
            col = [row[c] for row in hs]
            if len({true(h, k)[1] for h in col}) != 1:
                raise DctqError(f"frame_tile: plane {k}: true widths differ along column {c}")
            if c < cols - 1 and any(true(h, k)[3] for h in col):
                raise DctqError("frame_tile: only the last column may carry a right crop")
        y, x = [0], [0]
        for row in hs:
            y.append(y[-1] + true(row[0], k)[0])
        for h in hs[0]:
            x.append(x[-1] + true(h, k)[1])
        pb, pr = true(hs[-1][0], k)[2], true(hs[0][-1], k)[3]
        ys.append(y)
        xs.append(x)
        shapes.append((a["shapes"][k][0], y[-1] + pb, x[-1] + pr))
        crops.append((pb, pr))
    if colour:
        f, hh, ww = shapes[0]
        shapes += [(f, hh // sub, ww // sub)] * 2
        crops += [(0, 0), (0, 0)]
    ats = [[(ys[0][r], xs[0][c]) if colour else [(ys[k][r], xs[k][c]) for k in range(n)] for c in range(cols)]
           for r in range(rows)]
    return shapes, crops, ats


def frame_tile(grid, stream=None):
    """A list of rows of containers joined spatially into one container, without decoding: the
    spatial counterpart of frame_concat (tools/paste_ref.py frame_tile gives the same bytes).  All
    containers must agree in quality, adaptive, colour, the number of planes, the subsampling and
    the frames; true heights must be equal along a row and true widths along a column; only the
    last row and the last column may carry a crop (every other tile is whole blocks of m: 8; 16
    for a 4:2:0 picture); else DctqError before anything is launched.  frame_tile of the tiles'
    compress is byte for byte compress of the joined picture, so band shards (dct_amd/shard.py)
    that each compress their band become one container with no coefficients or pixels moved.
    Built as frame_blank plus one frame_paste per tile: K tiles are K passes over the payload built
    so far (each a copy of what the earlier ones wrote), which is simple and not the fastest way
    to join many tiles."""
    opened = [[_frame_open(b, stream) for b in row] for row in grid]
    shapes, crops, ats = _tile_layout([[h for _, h in row] for row in opened])
    a = opened[0][0][1]
    if any(b.device != opened[0][0][0].device for row in opened for b, _ in row):
        raise DctqError("frame_tile: the containers must be on one device")
    out = frame_blank(shapes, a["quality"], a["adaptive"], a["colour"], crops, device=opened[0][0][0].device,
                      stream=stream)
    for row, at_row in zip(opened, ats):
        for (b, _), at in zip(row, at_row):
            out = frame_paste(out, b, at=at, frame=0, stream=stream)
    return out


def symbol_bytes(quality: int, adaptive: bool = False) -> int:
    """Host-only: the encoder's symbol format of a standard-table plan (2 or 4 bytes)."""
    return int(diag().dctq_debug_symbol_bytes(int(quality), int(bool(adaptive))))


def synth(seed: int, kind, width: int, height: int, nframes: int = 1, device="cuda", stream=None, out=None):
    """Synthetic u8 frames [F, H, W] generated on the device (oracle-identical)."""
    import torch
    k = KINDS[kind] if isinstance(kind, str) else int(kind)
    if out is None:
        out = torch.empty((nframes, height, width), dtype=torch.uint8, device=device)
    d = plane_desc(out)
    _check(lib().dctq_synth(C.c_uint64(seed), k, C.byref(d), _stream_ptr(stream)))
    return out


def forward_kernel(quality: int, adaptive: bool, batches: int, num_cus: int) -> str:
    """Name of the forward kernel dctq_forward_quant_planes launches for this plan over
    `batches` 64-block batches on num_cus CUs (host-only, dctq_debug_forward_kernel)."""
    v = diag().dctq_debug_forward_kernel(int(quality), int(bool(adaptive)), int(batches), int(num_cus))
    return f"fdct8_quant_v{v}<{str(bool(adaptive)).lower()}, false, false>"


def inverse_bound(quality: int, adaptive: bool = False):
    """Host-only: (bound, admitted) -- the rigorous bound of |recon - reference| of the
    fused round trip's fp32 inverse for this standard-table plan, and whether
    round_trip_planes runs that inverse for it (tools/inv_bound.py, plan_tables.hip)."""
    a = C.c_int(0)
    b = diag().dctq_debug_inverse_bound(int(quality), int(bool(adaptive)), C.byref(a))
    return float(b), bool(a.value)


def debug_tables(quality: int, adaptive: bool = False):
    """Host-only: the (w, thr, D, Q) tables a plan would upload (no GPU needed)."""
    import numpy as np
    w = np.zeros(64, np.float32)
    thr = np.zeros(64, np.float32)
    d = np.zeros(64, np.float64)
    q = np.zeros(64, np.float64)
    _check(diag().dctq_debug_tables(quality, int(adaptive), w.ctypes.data, thr.ctypes.data, d.ctypes.data,
                                    q.ctypes.data))
    return w, thr, d, q
