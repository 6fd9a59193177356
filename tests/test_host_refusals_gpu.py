"""GPU: the refusals of the Python host (dct_amd/__init__.py) that need a device tensor to get past
the first check, pinned by their exact messages; tests/test_host_refusals_cpu.py has the rest and
the list of what neither file can reach.  The expected strings are literals, copied from what the
host raised before its wrappers were folded onto shared helpers.  Two were reworded by that fold, on
purpose, and are quoted as they are now: decode_symbols' offsets message is _need_byte_offsets'
(before: "... (one per block of every plane, plus one)"), and frame_pack gives the two `bytes`
messages of every other `bytes` consumer (before: one merged "bytes must be a contiguous uint8
tensor on a HIP device").

Tensors are a few bytes to a few KB and nearly every case raises before any launch (block_lengths
and frame_pack launch on one to four blocks).  Two tests at the end are about what the fold must
keep sound rather than about messages: totals read back on the caller's stream, and pointer arrays
that outlive the call they are built for."""
import gc
import types

import pytest
import torch

import dct_amd as dm

pytestmark = pytest.mark.gpu

E = dm.DctqError
PIXELS = "pixels must be a uint8 tensor on a HIP device"
PLANE = "pixels must be [H, W] or [F, H, W] with unit column stride"
BYTES = "bytes must be a uint8 tensor on a HIP device"
SYMBOLS = "symbols must be an int16 or int32 tensor on a HIP device"
SHAPES = "shapes entries must be (F, H, W) or (H, W)"
OFFSETS5 = "offsets must be a contiguous int32 device tensor of 5 elements (one per block, plus one)"
OFFSETS_ANY = "offsets must be a contiguous int32 device tensor of at least 2 elements (one per block, plus one)"
LENGTHS = "lengths must be a uint8, int16 or uint16 tensor on a HIP device"
W1 = [((0, 1), (0, 8), (0, 8))]               # the first block of a (1, 16, 16) plane


def z(shape, dtype, device="cuda"):
    return torch.zeros(shape, dtype=dtype, device=device)


@pytest.fixture(scope="module")
def t():
    """The tensors the cases share: p a (1, 16, 16) plane (4 blocks), its outputs of the right and
    of wrong kinds, a 4-block symbol stream and a 4-block byte stream."""
    i16, i32, f32, u8 = torch.int16, torch.int32, torch.float32, torch.uint8
    n = types.SimpleNamespace(i16=i16, i32=i32, f32=f32, u8=u8)
    n.plan, n.aplan = dm.Plan(50, False), dm.Plan(50, True)
    n.p, n.p8 = z((1, 16, 16), u8), z((1, 8, 8), u8)
    n.c, n.c3, n.r, n.v, n.v3 = z((4, 64), i16), z((3, 64), i16), z((4, 64), f32), z(4, i32), z(3, i32)
    n.strided = z((4, 128), i16)[:, ::2]
    n.off = torch.arange(5, dtype=i32, device="cuda")      # four blocks of one symbol / one byte each
    n.sym, n.byt = z(4, i32), z(4, u8)
    n.rgb = z((1, 16, 16, 3), u8)
    n.y, n.cb = z((1, 16, 16), u8), z((1, 8, 8), u8)
    return n


CASES = [
    # _need through forward_quant: host, dtype, contiguity, size
    ("out host", lambda t: t.plan.forward_quant(t.p, out=z((4, 64), t.i16, "cpu")), "out must be a tensor on a HIP device"),
    ("out dtype", lambda t: t.plan.forward_quant(t.p, out=z((4, 64), t.i32)), "out must be torch.int16, got torch.int32"),
    ("out strided", lambda t: t.plan.forward_quant(t.p, out=t.strided), "out must be contiguous"),
    ("out short", lambda t: t.plan.forward_quant(t.p, out=t.c3), "out holds 192 elements, 256 needed"),
    ("var_num dtype", lambda t: t.plan.forward_quant(t.p, var_num=z(4, t.i16)), "var_num must be torch.int32, got torch.int16"),
    ("var_num short", lambda t: t.plan.forward_quant(t.p, var_num=t.v3), "var_num holds 3 elements, 4 needed"),
    ("var_num host", lambda t: t.plan.forward_quant(t.p, var_num=[0] * 4), "var_num must be a tensor on a HIP device"),
    # plane_desc
    ("pixels of four axes", lambda t: t.plan.forward_quant(z((1, 1, 8, 8), t.u8)), PLANE),
    ("pixels of one axis", lambda t: t.plan.forward_quant_planes([z(64, t.u8)]), PLANE),
    ("pixels with a column stride", lambda t: t.plan.forward_quant(z((1, 8, 16), t.u8)[:, :, ::2]), PLANE),
    ("pixels dtype", lambda t: t.plan.forward_quant(z((1, 8, 8), torch.int8)), PIXELS),
    # the per-plane lists (_need_planes)
    ("outs count", lambda t: t.plan.forward_quant_planes([t.p], outs=[]), "outs needs one tensor per plane (1), got 0"),
    ("outs dtype", lambda t: t.plan.forward_quant_planes([t.p], outs=[t.r]), "outs[0] must be torch.int16, got torch.float32"),
    ("var_nums count", lambda t: t.plan.forward_quant_planes([t.p, t.p], var_nums=[t.v]),
     "var_nums needs one tensor per plane (2), got 1"),
    ("var_nums short", lambda t: t.plan.forward_quant_planes([t.p, t.p], var_nums=[t.v, t.v3]),
     "var_nums[1] holds 3 elements, 4 needed"),
    ("var_nums dtype", lambda t: t.plan.forward_quant_planes([t.p], var_nums=[t.c]),
     "var_nums[0] must be torch.int32, got torch.int16"),
    ("outs host", lambda t: t.plan.forward_quant_planes([t.p], outs=[t.c.cpu()]), "outs[0] must be a tensor on a HIP device"),
    ("outs strided", lambda t: t.plan.forward_quant_planes([t.p], outs=[t.strided]), "outs[0] must be contiguous"),
    ("outs short", lambda t: t.plan.forward_quant_planes([t.p, t.p], outs=[t.c, t.c3]), "outs[1] holds 192 elements, 256 needed"),
    ("var_nums host", lambda t: t.plan.forward_quant_planes([t.p], var_nums=[t.v.cpu()]),
     "var_nums[0] must be a tensor on a HIP device"),
    ("var_nums strided", lambda t: t.plan.forward_quant_planes([t.p], var_nums=[z(8, t.i32)[::2]]), "var_nums[0] must be contiguous"),
    ("round trip recons count", lambda t: t.plan.round_trip_planes([t.p], recons=[t.r, t.r]),
     "recons needs one tensor per plane (1), got 2"),
    ("round trip recons dtype", lambda t: t.plan.round_trip_planes([t.p], recons=[t.c]),
     "recons[0] must be torch.float32, got torch.int16"),
    ("round trip recons short", lambda t: t.plan.round_trip_planes([t.p], recons=[z((3, 64), t.f32)]),
     "recons[0] holds 192 elements, 256 needed"),
    ("round trip recons host", lambda t: t.plan.round_trip_planes([t.p], recons=[t.r.cpu()]),
     "recons[0] must be a tensor on a HIP device"),
    ("round trip recons strided", lambda t: t.plan.round_trip_planes([t.p], recons=[z((4, 128), t.f32)[:, ::2]]),
     "recons[0] must be contiguous"),
    ("round trip outs dtype", lambda t: t.plan.round_trip_planes([t.p], outs=[t.r]), "outs[0] must be torch.int16, got torch.float32"),
    ("round trip outs short", lambda t: t.plan.round_trip_planes([t.p], outs=[t.c3]), "outs[0] holds 192 elements, 256 needed"),
    ("round trip var_nums host", lambda t: t.plan.round_trip_planes([t.p], var_nums=[t.v.cpu()]),
     "var_nums[0] must be a tensor on a HIP device"),
    ("round trip var_nums strided", lambda t: t.plan.round_trip_planes([t.p], var_nums=[z(8, t.i32)[::2]]),
     "var_nums[0] must be contiguous"),
    ("round trip var_nums dtype", lambda t: t.plan.round_trip_planes([t.p], var_nums=[z(4, t.i16)]),
     "var_nums[0] must be torch.int32, got torch.int16"),
    ("round trip outs strided", lambda t: t.plan.round_trip_planes([t.p], outs=[t.strided]), "outs[0] must be contiguous"),
    ("round trip outs host", lambda t: t.plan.round_trip_planes([t.p], outs=[t.c.cpu()]),
     "outs[0] must be a tensor on a HIP device"),
    ("round trip var_nums short", lambda t: t.plan.round_trip_planes([t.p], var_nums=[t.v3]),
     "var_nums[0] holds 3 elements, 4 needed"),
    ("encode outs count", lambda t: t.plan.encode_planes([t.p], outs=[t.c, t.c]), "outs needs one tensor per plane (1), got 2"),
    ("encode outs short", lambda t: t.plan.encode_planes([t.p], outs=[t.c3]), "outs[0] holds 192 elements, 256 needed"),
    ("encode symbol_bytes", lambda t: t.plan.encode_planes([t.p], symbol_bytes=8), "symbol_bytes must be 2 or 4"),
    ("movement outs count", lambda t: t.plan.diag_movement_planes([t.p], []), "outs needs one tensor per plane (1), got 0"),
    ("movement of a product plan", lambda t: t.plan.diag_movement_planes([t.p], [t.c]),
     "diag_movement_planes needs a plan of the diagnostic library (Plan(..., diagnostic=True))"),
    ("rt movement recons short", lambda t: t.plan.diag_rt_movement_planes([t.p], [t.c], [z((3, 64), t.f32)]),
     "recons[0] holds 192 elements, 256 needed"),
    ("rt movement of a product plan", lambda t: t.plan.diag_rt_movement_planes([t.p], [t.c], [t.r]),
     "diag_rt_movement_planes needs a plan of the diagnostic library (Plan(..., diagnostic=True))"),
    # one result per block
    ("huffman planes out dtype", lambda t: t.plan.huffman_bits_planes([t.p], out=z(4, t.i16)),
     "out must be torch.int32, got torch.int16"),
    ("huffman planes out short", lambda t: t.plan.huffman_bits_planes([t.p, t.p8], out=t.v), "out holds 4 elements, 5 needed"),
    ("distortion out short", lambda t: t.plan.distortion_planes([t.p, t.p8], out=t.v), "out holds 4 elements, 5 needed"),
    ("distortion out host", lambda t: t.plan.distortion_planes([t.p], out=t.v.cpu()), "out must be a tensor on a HIP device"),
    ("distortion of nothing", lambda t: t.plan.distortion_planes([]), "distortion_planes needs at least one plane"),
    ("huffman planes out strided", lambda t: t.plan.huffman_bits_planes([t.p], out=z(8, t.i32)[::2]), "out must be contiguous"),
    ("huffman planes out host", lambda t: t.plan.huffman_bits_planes([t.p], out=t.v.cpu()), "out must be a tensor on a HIP device"),
    ("distortion out dtype", lambda t: t.plan.distortion_planes([t.p], out=z(4, t.i16)), "out must be torch.int32, got torch.int16"),
    ("huffman out short", lambda t: dm.huffman_bits(t.c, out=t.v3), "out holds 3 elements, 4 needed"),
    ("huffman coef dtype", lambda t: dm.huffman_bits(t.r), "coef must be torch.int16, got torch.float32"),
    ("forward_float out dtype", lambda t: t.plan.forward_float(t.p, out=t.c), "out must be torch.float32, got torch.int16"),
    ("forward_float out short", lambda t: t.plan.forward_float(t.p, out=z((3, 64), t.f32)), "out holds 192 elements, 256 needed"),
    ("inverse coef dtype", lambda t: t.plan.inverse(z((4, 64), t.i32)), "coef must be torch.int16, got torch.int32"),
    ("inverse coef strided", lambda t: t.plan.inverse(t.strided), "coef must be contiguous"),
    ("inverse out short", lambda t: t.plan.inverse(t.c, out=z((3, 64), t.f32)), "out holds 192 elements, 256 needed"),
    ("inverse out dtype", lambda t: t.plan.inverse(t.c, out=z((4, 64), t.i16)), "out must be torch.float32, got torch.int16"),
    ("inverse out strided", lambda t: t.plan.inverse(t.c, out=z((4, 128), t.f32)[:, ::2]), "out must be contiguous"),
    ("inverse out host", lambda t: t.plan.inverse(t.c, out=t.r.cpu()), "out must be a tensor on a HIP device"),
    ("inverse var_num dtype", lambda t: t.plan.inverse(t.c, var_num=z(4, t.i16)), "var_num must be torch.int32, got torch.int16"),
    ("inverse var_num strided", lambda t: t.plan.inverse(t.c, var_num=z(8, t.i32)[::2]), "var_num must be contiguous"),
    ("inverse var_num short", lambda t: t.plan.inverse(t.c, var_num=t.v3), "var_num holds 3 elements, 4 needed"),
    ("plan inverse", lambda t: dm.Plan(50, False, inverse="fp32"), 'inverse must be "fp64" or "auto"'),
    # decode_planes and its destinations (_decode_outs)
    ("decode coefs short", lambda t: t.plan.decode_planes([t.c3], shapes=[(16, 16)]), "coefs[0] holds 192 elements, 256 needed"),
    ("decode coefs dtype", lambda t: t.plan.decode_planes([t.r], shapes=[(16, 16)]), "coefs[0] must be torch.int16, got torch.float32"),
    ("decode coefs host", lambda t: t.plan.decode_planes([t.c.cpu()], outs=[t.p]), "coefs[0] must be a tensor on a HIP device"),
    ("decode coefs strided", lambda t: t.plan.decode_planes([t.strided], outs=[t.p]), "coefs[0] must be contiguous"),
    ("decode var_nums host", lambda t: t.plan.decode_planes([t.c], outs=[t.p], var_nums=[t.v.cpu()]),
     "var_nums[0] must be a tensor on a HIP device"),
    ("decode var_nums strided", lambda t: t.plan.decode_planes([t.c], outs=[t.p], var_nums=[z(8, t.i32)[::2]]),
     "var_nums[0] must be contiguous"),
    ("decode neither", lambda t: t.plan.decode_planes([t.c]), "decode_planes needs shapes or outs"),
    ("decode shapes count", lambda t: t.plan.decode_planes([t.c], shapes=[]), "shapes needs one entry per plane (1), got 0"),
    ("decode outs count", lambda t: t.plan.decode_planes([t.c], outs=[t.p, t.p]), "outs needs one entry per plane (1), got 2"),
    ("decode var_nums count", lambda t: t.plan.decode_planes([t.c], outs=[t.p], var_nums=[]),
     "var_nums needs one entry per plane (1), got 0"),
    ("decode shape of one", lambda t: t.plan.decode_planes([t.c], shapes=[(16,)]), SHAPES),
    ("decode outs against shapes", lambda t: t.plan.decode_planes([t.c], shapes=[(16, 16)], outs=[t.p8]),
     "outs[0] is (1, 8, 8), shapes[0] says (1, 16, 16)"),
    ("decode outs of two axes against shapes", lambda t: t.plan.decode_planes([t.c], shapes=[(2, 8, 8)], outs=[t.p8[0]]),
     "outs[0] is (8, 8), shapes[0] says (2, 8, 8)"),
    ("decode outs of 12 rows", lambda t: t.plan.decode_planes([t.c], outs=[z((1, 12, 16), t.u8)]),
     "outs[0]: width and height must be multiples of 8"),
    ("decode shapes of 12 columns", lambda t: t.plan.decode_planes([t.c], shapes=[(16, 12)]),
     "outs[0]: width and height must be multiples of 8"),
    ("decode outs dtype", lambda t: t.plan.decode_planes([t.c], outs=[t.c]), PIXELS),
    ("decode var_nums short", lambda t: t.plan.decode_planes([t.c], outs=[t.p], var_nums=[t.v3]),
     "var_nums[0] holds 3 elements, 4 needed"),
    ("decode one var_num dtype", lambda t: t.plan.decode(t.c, (16, 16), var_num=t.c),
     "var_nums[0] must be torch.int32, got torch.int16"),
    # decode_symbols
    ("symbols dtype", lambda t: t.plan.decode_symbols(t.byt, t.off, shapes=[(16, 16)]), SYMBOLS),
    ("symbols strided", lambda t: t.plan.decode_symbols(z(8, t.i32)[::2], t.off, shapes=[(16, 16)]), "symbols must be contiguous"),
    ("symbols neither", lambda t: t.plan.decode_symbols(t.sym, t.off), "decode_symbols needs shapes or outs"),
    ("symbols outs against shapes", lambda t: t.plan.decode_symbols(t.sym, t.off, shapes=[(16, 16)], outs=[t.p8]),
     "outs[0] is (1, 8, 8), shapes[0] says (1, 16, 16)"),
    ("symbols outs count", lambda t: t.plan.decode_symbols(t.sym, t.off, shapes=[(16, 16)], outs=[t.p, t.p]),
     "outs needs one entry per plane (1), got 2"),
    ("symbols var_nums short", lambda t: t.plan.decode_symbols(t.sym, t.off, shapes=[(16, 16)], var_nums=[t.v3]),
     "var_nums[0] holds 3 elements, 4 needed"),
    ("symbols offsets short", lambda t: t.plan.decode_symbols(t.sym, t.off[:4], shapes=[(16, 16)]), OFFSETS5),
    ("symbols offsets host", lambda t: t.plan.decode_symbols(t.sym, t.off.cpu(), outs=[t.p]), OFFSETS5),
    ("symbols offsets dtype", lambda t: t.plan.decode_symbols(t.sym, t.off.long(), outs=[t.p]), OFFSETS5),
    ("symbols offsets strided", lambda t: t.plan.decode_symbols(t.sym, z(10, t.i32)[::2], outs=[t.p]), OFFSETS5),
    # decode_bits
    ("bytes dtype", lambda t: t.plan.decode_bits(z(4, torch.int8), t.off, shapes=[(16, 16)]), BYTES),
    ("bytes strided", lambda t: t.plan.decode_bits(z(8, t.u8)[::2], t.off, shapes=[(16, 16)]), "bytes must be contiguous"),
    ("bits neither", lambda t: t.plan.decode_bits(t.byt, t.off), "decode_bits needs shapes or outs"),
    ("bits var_nums count", lambda t: t.plan.decode_bits(t.byt, t.off, shapes=[(16, 16)], var_nums=[t.v, t.v]),
     "var_nums needs one entry per plane (1), got 2"),
    ("bits outs of 12 rows", lambda t: t.plan.decode_bits(t.byt, t.off, outs=[z((1, 12, 16), t.u8)]),
     "outs[0]: width and height must be multiples of 8"),
    ("bits offsets long", lambda t: t.plan.decode_bits(t.byt, z(6, t.i32), shapes=[(16, 16)]), OFFSETS5),
    ("bits offsets host", lambda t: t.plan.decode_bits(t.byt, t.off.cpu(), shapes=[(16, 16)]), OFFSETS5),
    # decode_bits_window
    ("window bytes strided", lambda t: t.plan.decode_bits_window(z(8, t.u8)[::2], t.off, [(16, 16)], W1), "bytes must be contiguous"),
    ("window count", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], W1 * 2),
     "windows needs one entry per plane (1), got 2"),
    ("window shape of four", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(1, 1, 16, 16)], W1), SHAPES),
    ("window of two ranges", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], [((0, 1), (0, 8))]),
     "windows[0] must be ((f0, f1), (y0, y1), (x0, x1))"),
    ("window of a number", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], [7]),
     "windows[0] must be ((f0, f1), (y0, y1), (x0, x1))"),
    ("window stored plane of 12 rows", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(12, 16)], W1),
     "shapes[0] (1, 12, 16): height and width must be multiples of 8, nframes >= 1"),
    ("window stored plane of no frames", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(0, 16, 16)], W1),
     "shapes[0] (0, 16, 16): height and width must be multiples of 8, nframes >= 1"),
    ("window past the frames", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], [((0, 2), (0, 8), (0, 8))]),
     "windows[0] ((0, 2), (0, 8), (0, 8)) is empty or leaves the stored plane (1, 16, 16)"),
    ("window empty", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], [((0, 1), (8, 8), (0, 8))]),
     "windows[0] ((0, 1), (8, 8), (0, 8)) is empty or leaves the stored plane (1, 16, 16)"),
    ("window off the blocks", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], [((0, 1), (4, 8), (0, 8))]),
     "windows[0] ((0, 1), (4, 8), (0, 8)): rows and columns must be multiples of 8"),
    ("window of 2^26 stored blocks", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(65536, 65536)], W1),
     "more than 2^26 - 1 blocks in one decode"),
    ("window outs against the window", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], W1, outs=[t.p]),
     "outs[0] is (1, 16, 16), shapes[0] says (1, 8, 8)"),
    ("window outs count", lambda t: t.plan.decode_bits_window(t.byt, t.off, [(16, 16)], W1, outs=[]),
     "outs needs one entry per plane (1), got 0"),
    ("window offsets of the window", lambda t: t.plan.decode_bits_window(t.byt, t.off[:2], [(16, 16)], W1), OFFSETS5),
    ("window adaptive", lambda t: t.aplan.decode_bits_window(t.byt, t.off, [(16, 16)], W1), "adaptive decode needs var_nums"),
    ("window var_nums count", lambda t: t.aplan.decode_bits_window(t.byt, t.off, [(16, 16)], W1, var_nums=[t.v, t.v]),
     "var_nums needs one entry per plane (1), got 2"),
    ("window var_nums of the window", lambda t: t.aplan.decode_bits_window(t.byt, t.off, [(16, 16)], W1, var_nums=[z(1, t.i32)]),
     "var_nums[0] holds 1 elements, 4 needed"),
    ("window var_nums dtype", lambda t: t.aplan.decode_bits_window(t.byt, t.off, [(16, 16)], W1, var_nums=[z(4, t.i16)]),
     "var_nums[0] must be torch.int32, got torch.int16"),
    # the stream functions
    ("rle_encode coef dtype", lambda t: dm.rle_encode(z((4, 64), t.i32)), "coef must be torch.int16, got torch.int32"),
    ("rle_decode out dtype", lambda t: dm.rle_decode(t.sym, t.off, out=t.r), "out must be torch.int16, got torch.float32"),
    ("rle_decode out short", lambda t: dm.rle_decode(t.sym, t.off, out=t.c3), "out holds 192 elements, 256 needed"),
    ("pack symbols dtype", lambda t: dm.bits_pack(t.byt, t.off), SYMBOLS),
    ("pack symbols strided", lambda t: dm.bits_pack(z(8, t.i16)[::2], t.off), "symbols must be contiguous"),
    ("pack symbol_bytes", lambda t: dm.bits_pack(t.sym, t.off, symbol_bytes=2), "symbol_bytes 2 does not match symbols of torch.int32"),
    ("pack symbol_bytes of int16", lambda t: dm.bits_pack(z(4, t.i16), t.off, symbol_bytes=4),
     "symbol_bytes 4 does not match symbols of torch.int16"),
    ("pack offsets of one", lambda t: dm.bits_pack(t.sym, t.off[:1]), OFFSETS_ANY),
    ("pack offsets dtype", lambda t: dm.bits_pack(t.sym, t.off.long()), OFFSETS_ANY),
    ("pack offsets host", lambda t: dm.bits_pack(t.sym, t.off.cpu()), OFFSETS_ANY),
    ("pack offsets strided", lambda t: dm.bits_pack(t.sym, z(10, t.i32)[::2]), OFFSETS_ANY),
    ("pack capacity", lambda t: dm.bits_pack(t.sym, t.off, capacity=-1), "capacity must be >= 0"),
    ("unpack bytes dtype", lambda t: dm.bits_decode(t.sym, t.off), BYTES),
    ("unpack bytes strided", lambda t: dm.bits_decode(z(8, t.u8)[::2], t.off), "bytes must be contiguous"),
    ("unpack offsets host", lambda t: dm.bits_decode(t.byt, t.off.cpu()), OFFSETS_ANY),
    ("unpack out short", lambda t: dm.bits_decode(t.byt, t.off, out=t.c3), "out holds 192 elements, 256 needed"),
    ("lengths of offsets dtype", lambda t: dm.block_lengths(t.off.long()), OFFSETS_ANY),
    ("length_bytes", lambda t: dm.block_lengths(t.off, length_bytes=3), "length_bytes must be 1, 2 or None"),
    ("a length of 300 in one byte", lambda t: dm.block_lengths(torch.tensor([0, 300, 301], dtype=t.i32, device="cuda"), length_bytes=1),
     "a block of 300 bytes does not fit length_bytes 1"),
    ("a length of 70000", lambda t: dm.block_lengths(torch.tensor([0, 70000], dtype=t.i32, device="cuda")),
     "a block of 70000 bytes does not fit length_bytes 2"),
    ("offsets of lengths dtype", lambda t: dm.block_offsets(t.sym), LENGTHS),
    ("offsets of no lengths", lambda t: dm.block_offsets(z(0, t.u8)), "lengths must be contiguous and hold at least one block"),
    ("offsets of strided lengths", lambda t: dm.block_offsets(z(8, t.u8)[::2]), "lengths must be contiguous and hold at least one block"),
    ("offsets out short", lambda t: dm.block_offsets(t.byt, out=t.v), "out holds 4 elements, 5 needed"),
    ("offsets out dtype", lambda t: dm.block_offsets(t.byt, out=z(5, t.i16)), "out must be torch.int32, got torch.int16"),
    # colour and padding
    ("subsampling", lambda t: dm.rgb_to_ycbcr(t.rgb, "422"), 'subsampling must be "420" or "444"'),
    ("420 of 24 columns", lambda t: dm.rgb_to_ycbcr(z((1, 16, 24, 3), t.u8)), "420: width and height must be multiples of 16, got 24 x 16"),
    ("444 of 12 rows", lambda t: dm.rgb_to_ycbcr(z((12, 16, 3), t.u8), "444"), "444: width and height must be multiples of 8, got 16 x 12"),
    ("colour outs count", lambda t: dm.rgb_to_ycbcr(t.rgb, outs=[t.y, t.cb]), "outs needs three planes (y, cb, cr), got 2"),
    ("colour outs no tensors", lambda t: dm.rgb_to_ycbcr(t.rgb, outs=[t.y, t.cb, None]), "rgb and outs must be tensors"),
    ("colour cb of luma size", lambda t: dm.rgb_to_ycbcr(t.rgb, outs=[t.y, t.y, t.cb]), "outs: cb is (1, 16, 16), 420 of rgb needs (1, 8, 8)"),
    ("colour cr of chroma size", lambda t: dm.rgb_to_ycbcr(t.rgb, "444", outs=[t.y, t.y, t.cb]),
     "outs: cr is (1, 8, 8), 444 of rgb needs (1, 16, 16)"),
    ("colour padded y", lambda t: dm.rgb_to_ycbcr(z((1, 10, 10, 3), t.u8), outs=[z((1, 10, 10), t.u8), t.cb, t.cb], pad=True),
     "outs: y is (1, 10, 10), 420 of rgb needs (1, 16, 16)"),
    ("colour outs dtype", lambda t: dm.rgb_to_ycbcr(t.rgb, outs=[t.y, t.cb, z((1, 8, 8), t.i16)]), PIXELS),
    ("planes differ in frames", lambda t: dm.ycbcr_to_rgb(z((2, 16, 16), t.u8), t.cb, t.cb), "y, cb and cr differ in the number of frames"),
    ("size of 20 rows", lambda t: dm.ycbcr_to_rgb(t.y, t.cb, t.cb, size=(20, 16)),
     "size (20, 16) rounded up to multiples of 16 is not y's (16, 16)"),
    ("size of no rows", lambda t: dm.ycbcr_to_rgb(t.y, t.y, t.y, size=(0, 16)),
     "size (0, 16) rounded up to multiples of 8 is not y's (16, 16)"),
    ("size of 8 columns in 444", lambda t: dm.ycbcr_to_rgb(t.y, t.y, t.y, size=(16, 8)),
     "size (16, 8) rounded up to multiples of 8 is not y's (16, 16)"),
    ("channels", lambda t: dm.ycbcr_to_rgb(t.y, t.cb, t.cb, channels=5), "channels must be 3 or 4"),
    ("rgb out size", lambda t: dm.ycbcr_to_rgb(t.y, t.cb, t.cb, out=z((1, 8, 8, 3), t.u8)), "out is (1, 8, 8) (F, H, W), y is (1, 16, 16)"),
    ("rgb out against size", lambda t: dm.ycbcr_to_rgb(t.y, t.cb, t.cb, out=t.rgb, size=(10, 10)),
     "out is (1, 16, 16) (F, H, W), y is (1, 10, 10)"),
    ("rgb out dtype", lambda t: dm.ycbcr_to_rgb(t.y, t.cb, t.cb, out=z((1, 16, 16, 3), t.i16)), "rgb must be a uint8 tensor"),
    ("rgb out host", lambda t: dm.ycbcr_to_rgb(t.y, t.cb, t.cb, out=t.rgb.cpu()), "rgb must be a tensor on a HIP device"),
    ("pad outs count", lambda t: dm.pad_planes([z((1, 10, 12), t.u8)], outs=[t.y, t.y]), "outs needs one tensor per plane (1), got 2"),
    ("pad outs size", lambda t: dm.pad_planes([z((1, 10, 12), t.u8)], outs=[z((1, 16, 8), t.u8)]),
     "outs[0] is (1, 16, 8), the padded plane is (1, 16, 16)"),
    ("pad outs no tensors", lambda t: dm.pad_planes([t.y], outs=[None]), "planes and outs must be tensors"),
    ("compress five planes", lambda t: dm.compress([t.p8] * 5), "compress needs an RGB stack or a list of 1..4 planes"),
    ("compress no planes", lambda t: dm.compress([]), "compress needs an RGB stack or a list of 1..4 planes"),
    # the container
    ("pack bytes strided", lambda t: dm.frame_pack(z(8, t.u8)[::2], t.off, [(16, 16)], 50), "bytes must be contiguous"),
    ("pack bytes dtype", lambda t: dm.frame_pack(z(4, torch.int8), t.off, [(16, 16)], 50), BYTES),
    ("pack shape of one", lambda t: dm.frame_pack(t.byt, t.off, [(16,)], 50), SHAPES),
    ("pack plane of 12 rows", lambda t: dm.frame_pack(t.byt, t.off, [(12, 16)], 50),
     "frame: plane 16 x 12 x 1: width and height must be multiples of 8, nframes >= 1"),
    ("pack colour of one plane", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, colour=True), "frame: colour needs three planes"),
    ("pack crops count", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, crops=[(0, 0), (0, 0)]),
     "frame: crops needs one (pad_bottom, pad_right) per plane"),
    ("pack crops count, one set", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, crops=[(1, 0), (0, 0)]),
     "frame: crops needs one (pad_bottom, pad_right) per plane"),
    ("pack pad of 8", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, crops=[(8, 0)]),
     "frame: plane 0: pads (8, 0) outside 0..7 or not smaller than the plane"),
    ("pack offsets of one block", lambda t: dm.frame_pack(t.byt, t.off[:2], [(16, 16)], 50), OFFSETS5),
    ("pack offsets host", lambda t: dm.frame_pack(t.byt, t.off.cpu(), [(16, 16)], 50), OFFSETS5),
    ("pack total", lambda t: dm.frame_pack(z(8, t.u8), t.off, [(16, 16)], 50), "offsets run from 0 to 4, bytes holds 8"),
    ("pack first offset", lambda t: dm.frame_pack(t.byt, t.off + 1, [(16, 16)], 50), "offsets run from 1 to 5, bytes holds 4"),
    ("pack adaptive", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, adaptive=True), "an adaptive container needs var_nums"),
    ("pack var_nums short", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, adaptive=True, var_nums=t.v3),
     "var_nums holds 3 elements, 4 needed"),
    ("pack var_nums list short", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, adaptive=True, var_nums=[t.v3[:1], t.v3[:2]]),
     "var_nums holds 3 elements, 4 needed"),
    ("pack var_nums dtype", lambda t: dm.frame_pack(t.byt, t.off, [(16, 16)], 50, adaptive=True, var_nums=z(4, t.i16)),
     "var_nums must be torch.int32, got torch.int16"),
    ("unpack of two axes", lambda t: dm.frame_unpack(z((8, 8), t.u8)),
     "buf must be a one-dimensional uint8 tensor on a HIP device, or a host buffer"),
    ("unpack dtype", lambda t: dm.frame_unpack(z(64, t.i16)),
     "buf must be a one-dimensional uint8 tensor on a HIP device, or a host buffer"),
    ("unpack short", lambda t: dm.frame_unpack(z(47, t.u8)), "frame: shorter than the 48-byte fixed header"),
    ("unpack no magic", lambda t: dm.frame_unpack(z(64, t.u8)), "frame: bad magic"),
]


@pytest.mark.parametrize("call,want", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refuses(t, call, want):
    with pytest.raises((E, ValueError)) as info:
        call(t)
    got = str(info.value)
    assert type(info.value) is (ValueError if want == "symbol_bytes must be 2 or 4" else E), got
    assert got == want


def test_unpack_refuses_lengths_that_do_not_sum_to_the_payload(t):
    """The fixture's good four-block container (a 64-byte header, then the lengths 1, 1, 1, 1)
    with its first length made 2 on the host: the total frame_unpack reads back is 5."""
    buf = dm.frame_pack(t.byt, t.off, [(16, 16)], 50).cpu().numpy().copy()
    assert buf[64:68].tolist() == [1, 1, 1, 1]
    buf[64] += 1
    with pytest.raises(E) as info:
        dm.frame_unpack(buf)
    assert str(info.value) == "frame: the lengths sum to 5, payload_bytes says 4"
    with pytest.raises(E) as info:
        dm.frame_unpack(torch.from_numpy(buf).cuda())
    assert str(info.value) == "frame: the lengths sum to 5, payload_bytes says 4"


def test_a_whole_container_still_packs_after_the_refusals(t):
    """The fixture's stream is a good one: what the cases above bend is the only thing wrong."""
    d = dm.frame_unpack(dm.frame_pack(t.byt, t.off, [(16, 16)], 50, crops=[(0, 0)]))
    assert d["shapes"] == [(1, 16, 16)] and d["crops"] is None and d["quality"] == 50
    assert torch.equal(d["offsets"], t.off) and d["bytes"].numel() == 4


# ---- totals are read on the caller's stream -------------------------------------------------------------
def test_totals_on_a_side_stream_equal_those_on_the_default_stream():
    """encode_planes, rle_encode, bits_pack and block_lengths size what they return by a total
    (or a maximum) the kernel wrote.  With torch's current stream left at the default and the
    launch sent to another stream, that value has to be copied back on the launch's stream:
    encode_planes and rle_encode used .item(), a copy on the CURRENT stream that nothing orders
    after the kernel.  A race cannot be made to fail on demand, so this test may well pass on the
    racy code too: it guards the state after the change and is not the evidence of the bug, which
    is the code itself (a copy on one stream, a kernel on another, no event between them).
    130 + 33 + 33 blocks: full tiles of 64 plus a tail, and planes that end in the middle of a tile."""
    plan = dm.Plan(50, False)
    planes = [dm.synth(11, "uniform", 520, 16), dm.synth(12, "uniform", 264, 8), dm.synth(13, "uniform", 264, 8)]
    assert [tuple(p.shape) for p in planes] == [(1, 16, 520), (1, 8, 264), (1, 8, 264)]

    def run(stream):
        coefs, off, sym = plan.encode_planes(planes, stream=stream)
        packed, boff = dm.bits_pack(sym, off, stream=stream)
        lengths, lb = dm.block_lengths(boff, stream=stream)
        return coefs, off, sym, packed, boff, lengths, lb

    want = run(None)
    coef = torch.cat(want[0])
    want_rle = dm.rle_encode(coef)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert torch.cuda.current_stream() != side
    got = run(side)
    got_rle = dm.rle_encode(coef, stream=side)
    assert torch.cuda.current_stream() != side
    side.synchronize()
    assert want[1].numel() == 197 and int(want[1][-1]) == want[2].numel() and int(want[4][-1]) == want[3].numel()
    for a, b in zip(want[0], got[0]):
        assert torch.equal(a, b)
    for a, b in zip(want[1:6] + tuple(want_rle), got[1:6] + tuple(got_rle)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert want[6] == got[6]
    dm.stream_release(side)


# ---- pointer arrays outlive the call --------------------------------------------------------------------
def test_per_plane_pointer_arrays_survive_a_collection():
    """The arrays of per-plane pointers handed to the library are temporaries of the wrapper: they
    must be owned by what is passed, up to the return of the C call.  Three planes with outputs
    the test allocated and poisoned, a collection between building them and the call, and every
    output must be what the one-plane calls give (an adaptive plan, so var_nums are written by the
    round trip and read by the decoder)."""
    plan = dm.Plan(90, True)
    planes = [dm.synth(21, "uniform", 24, 16), dm.synth(22, "smooth", 8, 8), dm.synth(23, "extreme", 16, 8)]
    nbs = [6, 1, 2]
    outs = [torch.full((nb, 64), 0x7F7F, dtype=torch.int16, device="cuda") for nb in nbs]
    recons = [torch.full((nb, 64), float("nan"), dtype=torch.float32, device="cuda") for nb in nbs]
    var_nums = [torch.full((nb,), -1, dtype=torch.int32, device="cuda") for nb in nbs]
    pix = [torch.full(tuple(p.shape), 0xAA, dtype=torch.uint8, device="cuda") for p in planes]
    gc.collect()
    o, r = plan.round_trip_planes(planes, outs=outs, recons=recons, var_nums=var_nums)
    gc.collect()
    d = plan.decode_planes(outs, outs=pix, var_nums=var_nums)
    assert all(a is b for a, b in zip(o + r + d, outs + recons + pix))
    for k, p in enumerate(planes):
        vn = torch.full((nbs[k],), -1, dtype=torch.int32, device="cuda")
        (c1,), (r1,) = plan.round_trip_planes([p], var_nums=[vn])
        assert torch.equal(outs[k], c1) and torch.equal(recons[k], r1) and torch.equal(var_nums[k], vn)
        assert not torch.isnan(recons[k]).any()
        assert torch.equal(pix[k], plan.decode(c1, tuple(p.shape), var_num=vn))
