"""CPU: every refusal of the Python host (dct_amd/__init__.py) that host tensors, or no tensors at
all, can reach, pinned by its exact message.  The expected strings are literals, copied from what
the host raised before its wrappers were folded onto shared helpers; they are never computed from
the code under test.  A Plan method is reached through a Plan without a handle (no device, no
dctq_plan_create): every case here raises before the library is called.

Refusals that need a device tensor to get past the first check are in
tests/test_host_refusals_gpu.py.  Left out of both files:
  lib(), diag()         -- "... is missing": needs an install without its libraries;
  _need, _need_planes, _need_byte_offsets, _same_device, Plan.decode_symbols, Plan.decode_bits,
  Plan.decode_bits_window -- their "... is on cuda:1 ..." / "... must be on one device" refusals
                           need a second device;
  _frame_header         -- its rules are tests/test_frame_cpu.py's.

Three messages were reworded by that fold, on purpose, and are quoted as they are now: frame_pack
gives the two `bytes` messages of every other `bytes` consumer (before: "bytes must be a contiguous
uint8 tensor on a HIP device"), its crop count comes from _frame_crops in the same words, and
decode_symbols' offsets message is _need_byte_offsets' (tests/test_host_refusals_gpu.py)."""
import numpy as np
import pytest
import torch

import dct_amd as dm

E = dm.DctqError
PIXELS = "pixels must be a uint8 tensor on a HIP device"
BYTES = "bytes must be a uint8 tensor on a HIP device"
SYMBOLS = "symbols must be an int16 or int32 tensor on a HIP device"
SHAPES = "shapes entries must be (F, H, W) or (H, W)"
TABLE = "table and dequant must be C-contiguous float64 arrays [n, n]"
SHORT = "frame: shorter than the 48-byte fixed header"

u8 = torch.zeros((8, 8), dtype=torch.uint8)
i16 = torch.zeros((1, 64), dtype=torch.int16)
i32 = torch.zeros(2, dtype=torch.int32)
f32 = torch.zeros((1, 64), dtype=torch.float32)
WIN = [((0, 1), (0, 8), (0, 8))]


@pytest.fixture(scope="module")
def plan():
    from dct_amd.build import build
    build()
    p = dm.Plan.__new__(dm.Plan)
    p._L, p._diag, p._h, p.quality, p.adaptive = dm.lib(), False, None, 50, False
    return p


def raised(call, exc):
    with pytest.raises(exc) as info:
        call()
    assert type(info.value) is exc
    return str(info.value)


PLAN_CASES = [
    ("forward_quant", lambda p: p.forward_quant(u8), E, PIXELS),
    ("forward_quant float", lambda p: p.forward_quant(u8.float()), E, PIXELS),
    ("forward_quant_planes", lambda p: p.forward_quant_planes([u8]), E, PIXELS),
    ("diag_movement_planes", lambda p: p.diag_movement_planes([u8], [i16]), E, PIXELS),
    ("diag_rt_movement_planes", lambda p: p.diag_rt_movement_planes([u8], [i16], [f32]), E, PIXELS),
    ("round_trip_planes", lambda p: p.round_trip_planes([u8]), E, PIXELS),
    ("encode_planes", lambda p: p.encode_planes([u8], symbol_bytes=4), E, PIXELS),
    ("encode_planes symbol_bytes", lambda p: p.encode_planes([u8], symbol_bytes=3), ValueError,
     "symbol_bytes must be 2 or 4"),
    ("encode_bits_planes", lambda p: p.encode_bits_planes([u8], symbol_bytes=2), E, PIXELS),
    ("huffman_bits_planes", lambda p: p.huffman_bits_planes([u8]), E, PIXELS),
    ("distortion_planes", lambda p: p.distortion_planes([u8]), E, PIXELS),
    ("distortion_planes none", lambda p: p.distortion_planes([]), E, "distortion_planes needs at least one plane"),
    ("rate_distortion_planes", lambda p: p.rate_distortion_planes([u8]), E, PIXELS),
    ("forward_float", lambda p: p.forward_float(u8), E, PIXELS),
    ("inverse", lambda p: p.inverse(i16), E, "coef must be a tensor on a HIP device"),
    ("inverse no tensor", lambda p: p.inverse([0] * 64), E, "coef must be a tensor on a HIP device"),
    ("decode_planes", lambda p: p.decode_planes([i16], shapes=[(8, 8)]), E, PIXELS),
    ("decode_planes outs", lambda p: p.decode_planes([i16], outs=[u8]), E, PIXELS),
    ("decode_planes neither", lambda p: p.decode_planes([i16]), E, "decode_planes needs shapes or outs"),
    ("decode_planes shapes count", lambda p: p.decode_planes([i16], shapes=[(8, 8), (8, 8)]), E,
     "shapes needs one entry per plane (1), got 2"),
    ("decode_planes outs count", lambda p: p.decode_planes([i16], outs=[]), E,
     "outs needs one entry per plane (1), got 0"),
    ("decode_planes var_nums count", lambda p: p.decode_planes([i16], shapes=[(8, 8)], var_nums=[i32, i32]), E,
     "var_nums needs one entry per plane (1), got 2"),
    ("decode_planes shape of one", lambda p: p.decode_planes([i16], shapes=[(8,)]), E, SHAPES),
    ("decode_planes shape of four", lambda p: p.decode_planes([i16], shapes=[(1, 1, 8, 8)]), E, SHAPES),
    ("decode", lambda p: p.decode(i16, (8, 8)), E, PIXELS),
    ("decode neither", lambda p: p.decode(i16), E, "decode_planes needs shapes or outs"),
    ("decode_symbols", lambda p: p.decode_symbols(i32, i32, shapes=[(8, 8)]), E, SYMBOLS),
    ("decode_symbols no tensor", lambda p: p.decode_symbols(None, i32, shapes=[(8, 8)]), E, SYMBOLS),
    ("decode_bits", lambda p: p.decode_bits(u8.reshape(-1), i32, shapes=[(8, 8)]), E, BYTES),
    ("decode_bits no tensor", lambda p: p.decode_bits(b"\0" * 4, i32, shapes=[(8, 8)]), E, BYTES),
    ("decode_bits_window", lambda p: p.decode_bits_window(u8.reshape(-1), i32, [(8, 8)], WIN), E, BYTES),
]

MODULE_CASES = [
    ("rle_encode", lambda: dm.rle_encode(i16), E, "coef must be a tensor on a HIP device"),
    ("huffman_bits", lambda: dm.huffman_bits(i16), E, "coef must be a tensor on a HIP device"),
    ("rle_decode", lambda: dm.rle_decode(i32, i32), E, "out must be a tensor on a HIP device"),
    ("bits_pack", lambda: dm.bits_pack(i32, i32), E, SYMBOLS),
    ("bits_pack no tensor", lambda: dm.bits_pack([1, 2], i32), E, SYMBOLS),
    ("bits_decode", lambda: dm.bits_decode(u8.reshape(-1), i32), E, BYTES),
    ("block_lengths", lambda: dm.block_lengths(i32), E,
     "offsets must be a contiguous int32 device tensor of at least 2 elements (one per block, plus one)"),
    ("block_offsets", lambda: dm.block_offsets(u8.reshape(-1)), E,
     "lengths must be a uint8, int16 or uint16 tensor on a HIP device"),
    ("block_offsets no tensor", lambda: dm.block_offsets([1, 2]), E,
     "lengths must be a uint8, int16 or uint16 tensor on a HIP device"),
    ("plane_desc", lambda: dm.plane_desc(u8), E, PIXELS),
    ("rgb_desc dtype", lambda: dm.rgb_desc(torch.zeros((8, 8, 3))), E, "rgb must be a uint8 tensor"),
    ("rgb_desc no tensor", lambda: dm.rgb_desc(np.zeros((8, 8, 3), np.uint8)), E, "rgb must be a uint8 tensor"),
    ("rgb_desc two axes", lambda: dm.rgb_desc(u8), E,
     "rgb must be [H, W, C] or [F, H, W, C] with C 3 or 4 (channel axis last)"),
    ("rgb_desc two channels", lambda: dm.rgb_desc(torch.zeros((8, 8, 2), dtype=torch.uint8)), E,
     "rgb must be [H, W, C] or [F, H, W, C] with C 3 or 4 (channel axis last)"),
    ("rgb_desc host", lambda: dm.rgb_desc(torch.zeros((8, 8, 3), dtype=torch.uint8)), E,
     "rgb must be a tensor on a HIP device"),
    ("rgb_to_ycbcr", lambda: dm.rgb_to_ycbcr(torch.zeros((16, 16, 3), dtype=torch.uint8)), E,
     "rgb must be a tensor on a HIP device"),
    ("ycbcr_to_rgb no tensors", lambda: dm.ycbcr_to_rgb(1, 2, 3), E, "y, cb and cr must be tensors"),
    ("ycbcr_to_rgb", lambda: dm.ycbcr_to_rgb(u8, u8, u8), E, PIXELS),
    ("pad_planes none", lambda: dm.pad_planes([]), E, "pad_planes needs 1..4 planes"),
    ("pad_planes five", lambda: dm.pad_planes([u8] * 5), E, "pad_planes needs 1..4 planes"),
    ("pad_planes no tensors", lambda: dm.pad_planes([1]), E, "planes must be tensors"),
    ("pad_planes", lambda: dm.pad_planes([u8]), E, PIXELS),
    ("frame_pack", lambda: dm.frame_pack(u8.reshape(-1), i32, [(8, 8)], 50), E, BYTES),
    ("frame_pack no tensor", lambda: dm.frame_pack(b"\0" * 4, i32, [(8, 8)], 50), E, BYTES),
    ("frame_unpack host tensor", lambda: dm.frame_unpack(torch.zeros(64, dtype=torch.uint8)), E,
     "buf must be a one-dimensional uint8 tensor on a HIP device, or a host buffer"),
    ("frame_unpack short", lambda: dm.frame_unpack(b"\0" * 47), E, SHORT),
    ("frame_unpack short array", lambda: dm.frame_unpack(np.zeros(10, np.uint8)), E, SHORT),
    ("decompress short", lambda: dm.decompress(bytearray(12)), E, SHORT),
    ("compress no planes", lambda: dm.compress([]), E, "compress needs an RGB stack or a list of 1..4 planes"),
    ("compress five planes", lambda: dm.compress([u8] * 5), E, "compress needs an RGB stack or a list of 1..4 planes"),
    ("compress no tensors", lambda: dm.compress([1, 2]), E, "planes must be tensors"),
    ("compress planes", lambda: dm.compress([u8]), E, PIXELS),
    ("compress rgb", lambda: dm.compress(torch.zeros((16, 16, 3), dtype=torch.uint8)), E,
     "rgb must be a tensor on a HIP device"),
    ("compress rgb dtype", lambda: dm.compress(torch.zeros((16, 16, 3))), E, "rgb must be a uint8 tensor"),
    # quant_context and Plan.from_table: ValueError, before any library call
    ("quant_context float32", lambda: dm.quant_context(np.ones((8, 8), np.float32)), ValueError, TABLE),
    ("quant_context list", lambda: dm.quant_context([[1.0] * 8] * 8), ValueError, TABLE),
    ("quant_context flat", lambda: dm.quant_context(np.ones(64)), ValueError, TABLE),
    ("quant_context oblong", lambda: dm.quant_context(np.ones((8, 4))), ValueError, TABLE),
    ("quant_context strided", lambda: dm.quant_context(np.ones((8, 16))[:, ::2]), ValueError, TABLE),
    ("quant_context dequant", lambda: dm.quant_context(np.ones((8, 8)), dequant=np.ones((8, 8), np.float32)),
     ValueError, TABLE),
    ("from_table 63", lambda: dm.Plan.from_table(np.ones(63)), ValueError, "table must hold 8 x 8 entries"),
    ("from_table 9 x 9", lambda: dm.Plan.from_table(np.ones((9, 9))), ValueError, "table must hold 8 x 8 entries"),
]

P3 = [(2, 32, 32), (2, 16, 16), (2, 16, 16)]       # a 4:2:0 picture, two frames
P1 = [(1, 16, 16)]
GEOMETRY_CASES = [
    # _frame_geometry(shapes, colour)
    ("no planes", lambda: dm._frame_geometry([], False), "frame: nplanes must be 1..4"),
    ("five planes", lambda: dm._frame_geometry(P1 * 5, False), "frame: nplanes must be 1..4"),
    ("width 12", lambda: dm._frame_geometry([(1, 16, 12)], False),
     "frame: plane 12 x 16 x 1: width and height must be multiples of 8, nframes >= 1"),
    ("height 0", lambda: dm._frame_geometry([(1, 0, 16)], False),
     "frame: plane 16 x 0 x 1: width and height must be multiples of 8, nframes >= 1"),
    ("no frames", lambda: dm._frame_geometry([(0, 8, 8)], False),
     "frame: plane 8 x 8 x 0: width and height must be multiples of 8, nframes >= 1"),
    ("too many blocks", lambda: dm._frame_geometry([(1, 8 * 4096, 8 * 4096)], False),
     "frame: nblocks 16777216 outside 1..11671106"),
    ("colour of two", lambda: dm._frame_geometry(P1 * 2, True), "frame: colour needs three planes"),
    ("colour 4:2:2", lambda: dm._frame_geometry([(1, 16, 16), (1, 16, 8), (1, 16, 8)], True),
     "frame: colour needs chroma planes of 4:4:4 or 4:2:0 of plane 0"),
    ("colour cb is not cr", lambda: dm._frame_geometry([(1, 16, 16), (1, 8, 8), (1, 16, 16)], True),
     "frame: colour needs chroma planes of 4:4:4 or 4:2:0 of plane 0"),
    ("colour frames", lambda: dm._frame_geometry([(2, 16, 16), (1, 8, 8), (1, 8, 8)], True),
     "frame: colour needs chroma planes of 4:4:4 or 4:2:0 of plane 0"),
    # _frame_crops(crops, shapes, colour)
    ("crops count", lambda: dm._frame_crops([(1, 0)], P1 * 2, False),
     "frame: crops needs one (pad_bottom, pad_right) per plane"),
    ("pad of 8", lambda: dm._frame_crops([(8, 0)], P1, False),
     "frame: plane 0: pads (8, 0) outside 0..7 or not smaller than the plane"),
    ("negative pad", lambda: dm._frame_crops([(0, -1)], P1, False),
     "frame: plane 0: pads (0, -1) outside 0..7 or not smaller than the plane"),
    ("4:2:0 luma pad of 16", lambda: dm._frame_crops([(16, 0), (0, 0), (0, 0)], P3, True),
     "frame: plane 0: pads (16, 0) outside 0..15 or not smaller than the plane"),
    ("4:4:4 luma pad of 8", lambda: dm._frame_crops([(0, 8), (0, 0), (0, 0)], P1 * 3, True),
     "frame: plane 0: pads (0, 8) outside 0..7 or not smaller than the plane"),
    ("chroma pad", lambda: dm._frame_crops([(1, 0), (0, 1), (0, 0)], P3, True),
     "frame: plane 1: pads (0, 1) outside 0..0 or not smaller than the plane"),
    ("the whole plane", lambda: dm._frame_crops([(8, 0), (0, 0), (0, 0)], [(1, 8, 16), (1, 4, 8), (1, 4, 8)], True),
     "frame: plane 0: pads (8, 0) outside 0..15 or not smaller than the plane"),
    ("no crop", lambda: dm._frame_crops([(0, 0)], P1, False),
     "frame: the crop magic with no crop (that picture is frame v1)"),
    # _region_windows(shapes, crops, colour, region, frames) and _pair
    ("frames is no pair", lambda: dm._region_windows(P1, None, False, None, 3),
     "frames must be a pair of integers, got 3"),
    ("frames of three", lambda: dm._region_windows(P1, None, False, None, (0, 1, 2)),
     "frames must be a pair of integers, got (0, 1, 2)"),
    ("frames of words", lambda: dm._region_windows(P1, None, False, None, ("a", "b")),
     "frames must be a pair of integers, got ('a', 'b')"),
    ("frames empty", lambda: dm._region_windows(P3, None, True, None, (1, 1)),
     "frames (1, 1) is empty or outside the 2 frames"),
    ("frames past the end", lambda: dm._region_windows(P3, None, True, None, (0, 3)),
     "frames (0, 3) is empty or outside the 2 frames"),
    ("region is a number, colour", lambda: dm._region_windows(P3, None, True, 5, None),
     "region must be ((y0, y1), (x0, x1))"),
    ("region is a number, planes", lambda: dm._region_windows(P1, None, False, 5, None),
     "region must be ((y0, y1), (x0, x1)), or a list of one per plane"),
    ("region is empty, planes", lambda: dm._region_windows(P1, None, False, (), None),
     "region must be ((y0, y1), (x0, x1)), or a list of one per plane"),
    ("one region, two sizes", lambda: dm._region_windows([(1, 16, 16), (1, 8, 8)], None, False, ((0, 8), (0, 8)), None),
     "the planes differ in size: region must be a list of one region per plane"),
    ("one region, two true sizes", lambda: dm._region_windows(P1 * 2, [(1, 0), (0, 0)], False, ((0, 8), (0, 8)), None),
     "the planes differ in size: region must be a list of one region per plane"),
    ("a list for a picture", lambda: dm._region_windows(P3, None, True, [((0, 8), (0, 8))], None),
     "region must be ((y0, y1), (x0, x1))"),
    ("a list of the wrong length", lambda: dm._region_windows(P1 * 2, None, False, [((0, 8), (0, 8))], None),
     "region must be ((y0, y1), (x0, x1)), or a list of 2 of them"),
    ("a region of three ranges", lambda: dm._region_windows(P1, None, False, [((0, 8), (0, 8), (0, 8))], None),
     "region ((0, 8), (0, 8), (0, 8)) must be ((y0, y1), (x0, x1))"),
    ("rows of three", lambda: dm._region_windows(P1, None, False, ((0, 4, 8), (0, 8)), None),
     "a region's rows must be a pair of integers, got (0, 4, 8)"),
    ("columns of words", lambda: dm._region_windows(P1, None, False, ((0, 8), ("a", 8)), None),
     "a region's columns must be a pair of integers, got ('a', 8)"),
    ("region empty", lambda: dm._region_windows(P1, None, False, ((4, 4), (0, 8)), None),
     "region ((4, 4), (0, 8)) is empty or outside the picture of 16 x 16"),
    ("region leaves the true picture", lambda: dm._region_windows(P1, [(3, 5)], False, ((0, 14), (0, 11)), None),
     "region ((0, 14), (0, 11)) is empty or outside the picture of 13 x 11"),
]


def check(call, exc, want):
    assert raised(call, exc) == want


@pytest.mark.parametrize("call,exc,want", [c[1:] for c in PLAN_CASES], ids=[c[0] for c in PLAN_CASES])
def test_plan_method_refuses(plan, call, exc, want):
    check(lambda: call(plan), exc, want)


@pytest.mark.parametrize("call,exc,want", [c[1:] for c in MODULE_CASES], ids=[c[0] for c in MODULE_CASES])
def test_module_function_refuses(call, exc, want):
    check(call, exc, want)


@pytest.mark.parametrize("call,want", [c[1:] for c in GEOMETRY_CASES], ids=[c[0] for c in GEOMETRY_CASES])
def test_geometry_rule_refuses(call, want):
    check(call, E, want)


def test_grid_limit_does_not_nest_and_resets(plan):
    """The limit is host state of the diagnostic library: no device is needed to set it."""
    with dm.grid_limit(2):
        assert dm.lib() is dm.diag()
        assert raised(lambda: dm.grid_limit(3).__enter__(), E) == "grid_limit does not nest"
        assert dm.lib() is dm.diag()            # the refused one did not end the outer one
    assert dm.lib() is not dm.diag()
    with dm.grid_limit(1):                      # and the outer one ended clean
        pass
    assert dm.lib() is not dm.diag()
