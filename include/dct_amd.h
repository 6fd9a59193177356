/*
 * dct_amd.h -- batched (plane/frame-level) C-ABI of libdct_amd.so: the MI355X
 * hot path.  New surface added NEXT TO the reference's per-block API
 * (include/dct.h, include/quantization.h), which has no frame-level entry
 * point: the reference's only frame-level caller is the per-block pipeline of
 * tests/test_entropy.c:300-316 (create_block_from_pixels -> dct_forward ->
 * calculate_block_variance -> quantize) and its inverse :350-373
 * (dequantize -> dct_inverse).  Each entry point below replaces that loop over
 * every 8x8 block of a plane with one HIP launch.
 *
 * Conventions: plain pointers and sizes, no HIP/torch types.  Device pointers
 * are HIP device memory of the calling thread's current device; `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Every call is
 * asynchronous on `stream` and returns 0 or a negative DCTQ_E* code
 * (dctq_error_string).  Results are bit-identical to the reference
 * (src/dct.c + src/quantization.c) for the quantized path; see DESIGN.md.
 */
#ifndef DCT_AMD_H
#define DCT_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "quantization.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header.  6: dctq_encode_planes writes 4-byte symbols for
 * every plan again (round 5 had switched plans with |q| <= 511 to 2-byte symbols
 * under the same entry point); the 2-byte format is dctq_encode_planes16, opt-in;
 * dctq_abi_version() returns the library's revision so a host can check both. */
#define DCTQ_ABI_VERSION 6
int dctq_abi_version(void);

#define DCTQ_OK 0
#define DCTQ_EINVAL (-1)   /* bad argument (sizes not multiples of 8, misaligned, ...) */
#define DCTQ_EHIP (-2)     /* a HIP runtime call failed (dctq_error_string has the detail) */
#define DCTQ_ENOMEM (-3)
#define DCTQ_ENODEV (-4)   /* no gfx950 device visible */

/* Opaque per-configuration state: the host-computed tables (D of src/dct.c:17-30,
 * Q of src/quantization.c:51-99, fast-path scale and guard tables) uploaded to
 * the device that was current at creation.  A plan is read-only after
 * creation: one plan may serve several streams and threads at once, and the
 * library keeps no per-stream device state.  Threading: the batched calls do not
 * serialise -- after a thread's first call of an entry point on a stream (which
 * shields the host's rand() stream from the HIP runtime, as every plan and
 * memory call does) they take no lock and touch no global state. */
typedef struct dctq_plan dctq_plan;

/* quality is clamped to 1..100 exactly as quant_init does (src/quantization.c:26-31).
 * A plan holds only its ~4 KB of tables in device memory; it is reusable and
 * cheap to keep (one per quality is fine).  The forward resolves every plan's
 * rounding ties in place and allocates nothing per launch. */
int dctq_plan_create(int quality, int adaptive, dctq_plan **plan);
/* Bind an existing reference-style context (block_size must be 8); its
 * quant_matrix VALUES are used, so a caller-modified table is honoured. */
int dctq_plan_from_context(const QuantContext *qctx, dctq_plan **plan);
/* Frees the plan's device tables (hipFree, which waits for the device as cudaFree
 * does); launches that use the plan must have been issued before. */
void dctq_plan_destroy(dctq_plan *plan);

/* A stack of equally-shaped u8 planes in device memory. */
typedef struct {
    const uint8_t *pixels;   /* frame 0, row 0; 8-byte aligned */
    long long stride;        /* bytes between pixel rows; multiple of 8, >= width */
    long long frame_stride;  /* bytes between consecutive frames */
    int width, height;       /* multiples of 8 */
    int nframes;             /* >= 1 */
} dctq_plane;

/* Forward DCT + quantization of every 8x8 block:
 *   coef[f][by][bx][64] (int16, row-major within the block, blocks in raster
 *   order -- the order the reference emits them) = quantize(dct_forward(px-128)).
 * var_num (optional, may be NULL): per block 64*sum(x^2) - sum(x)^2 with
 * x = px-128; calculate_block_variance() == var_num / 4096.0 exactly.  Needed by
 * the adaptive inverse. */
int dctq_forward_quant(const dctq_plan *plan, const dctq_plane *src, int16_t *coef, int32_t *var_num,
                       void *stream);

/* The same for up to 4 planes of independent geometry (e.g. the Y, Cb, Cr planes
 * of a 4:2:0 frame stack) in ONE launch: plane k writes coef[k] (and var_num[k]
 * when var_num is non-NULL, in which case every var_num[k] must be set), exactly
 * as dctq_forward_quant(plan, &planes[k], coef[k], var_num[k]) would.  Saves a
 * launch gap and a grid tail per extra plane (the reference has no plane
 * notion: a caller coding Y/Cb/Cr runs its per-block loop once per plane). */
int dctq_forward_quant_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                              int32_t *const *var_num, void *stream);

/* Fused round trip (BASELINE configs[4]) of up to 4 planes in ONE launch: for
 * plane k, coef[k] (and var_num[k] if var_num is non-NULL) exactly as
 * dctq_forward_quant_planes, and
 *   recon[k][b][64] = dct_inverse(dequantize(coef[k][b])) + 128
 * exactly as dctq_inverse(plan, coef[k], var_num[k], ...) would produce it
 * (float, unclamped, |err| <= 1e-4: the coefficients here are the forward's own,
 * of u8 pixels, so they lie in the plan's forward range -- see dctq_decode_planes
 * -- and |recon| stays below 2048).  The quantized ints go from the forward to
 * the inverse through LDS: 448 B of HBM traffic per block instead of 584 B for
 * the two calls.  var_num is optional even for adaptive plans.  recon 16-byte
 * aligned. */
int dctq_round_trip_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                           int32_t *const *var_num, float *const *recon, void *stream);

/* Encoder: forward DCT + quantization + zigzag run-length
 * symbols of up to 4 planes.  coef[k] exactly as dctq_forward_quant_planes;
 * blocks numbered plane 0 first, then plane 1, ... (N in total, N < 2^26):
 *   offsets[b]  = first symbol of block b, offsets[N] = total symbols
 *   symbols[..] = the reference's run_length_encode of every block, in order
 *                 (as dctq_rle_count + dctq_rle_emit over the concatenated
 *                 coefficient planes): uint32_t (uint16_t)value | run << 16.
 * The symbol count is fused into the forward launch.  Symbols at index >=
 * symbols_capacity are not written; offsets are always complete (compare
 * offsets[N] with the capacity).  symbols == NULL or capacity 0: coefficients
 * and offsets only.  Worst case 64 symbols per block.  symbols 4-byte aligned.
 * workspace: dctq_encode_workspace_bytes(N) bytes of device memory, 4-byte
 * aligned; scratch (its contents after the call mean nothing). */
size_t dctq_encode_workspace_bytes(long long total_blocks);
int dctq_encode_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                       uint32_t *offsets, uint32_t *symbols, long long symbols_capacity, void *workspace,
                       void *stream);
/* The same stream in 2-byte symbols (opt-in, half the bytes):
 *   uint16_t (run & 63) << 10 | (value & 0x3FF), value in [-511, 511];
 * runs are 0..63 except the one symbol of an all-zero block, (value 0, run 64),
 * which is 0x0000 (no other symbol is: a zero value only ends a block, with
 * run >= 1).  dctq_rle_decode16 reads it.  Only for plans whose quantization
 * table bounds every quantized coefficient by 511 (dctq_plan_symbol_bytes == 2;
 * q <= 90 of the standard table); DCTQ_EINVAL for the others.  capacity in
 * symbols; symbols 4-byte aligned. */
int dctq_encode_planes16(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                         uint32_t *offsets, uint16_t *symbols, long long symbols_capacity, void *workspace,
                         void *stream);
/* The most compact symbol format the plan admits: 2 (dctq_encode_planes16 may be
 * used) or 4 (dctq_encode_planes only). */
int dctq_plan_symbol_bytes(const dctq_plan *plan);

/* Forward DCT only, float coefficients coef[f][by][bx][64]
 * (|coef - dct_forward()| <= 1e-4; computed in fp64, rounded once to fp32). */
int dctq_forward_float(const dctq_plan *plan, const dctq_plane *src, float *coef, void *stream);

/* Inverse: dequantize (reference semantics incl. the non-adaptive 1/Q
 * multiplier, src/quantization.c:139,144) + dct_inverse + 128, per block:
 *   recon[b][64] = dct_inverse(dequantize(coef[b], var_num[b]/4096)) + 128
 * (float, unclamped), for ANY int16 coefficients and any int32 var_num: computed
 * in fp64 and rounded once to fp32, so
 *   |err| <= 2^-24 * |recon| (+ the fp64 arithmetic's own error, below 1e-9 per
 *   1024 of summed input magnitude),
 * which is below 1e-4 wherever |recon| < 2048.  That covers every block a
 * non-adaptive plan's forward produces from u8 pixels; it does not cover
 * arbitrary coefficients -- int16 values
 * under an adaptive plan, which multiplies by Q, reach |recon| ~ 1e7, where one
 * fp32 rounding alone is ~0.5.  var_num is required when adaptive. */
int dctq_inverse(const dctq_plan *plan, const int16_t *coef, const int32_t *var_num, long long nblocks,
                 float *recon, void *stream);

/* Decoder: quantized coefficients -> u8 pixels (the reference's decode loop
 * tests/test_entropy.c:350-393: dequantize -> dct_inverse -> + 128 -> clamp), for
 * up to 4 planes of independent geometry in ONE launch.  For plane k and block b
 * in raster order (frame, block row, block column: the order dctq_forward_quant
 * writes), the 8x8 pixels of coef[k][b][64] go to their image position in dst[k]
 * (stride and frame_stride honoured; dst[k].pixels is written through, as
 * dctq_synth does).  Bytes outside width x height of each frame -- row padding,
 * gaps between frames -- are not touched.
 *   pix = (uint8_t) rne(min(max(r, 0), 255)),  rne = round to nearest, ties to even,
 * where r is the fp32 value dctq_round_trip_planes stores as recon for the same
 * plan and coefficients (so the result equals clamping and rounding that recon,
 * bit for bit).  Against the reference value c = dct_inverse(dequantize(coef)) + 128:
 *   |pix - clamp(c, 0, 255)| <= 0.5 + e  for every pixel, and the clamp is exact
 *   beyond e (pix == 0 where c < -e, pix == 255 where c > 255 + e),
 * where e depends on the INPUT DOMAIN, since coef is the caller's and a symbol
 * stream can carry any int16:
 *   - coefficients within the plan's forward range, |coef_uv| <= round(128 *
 *     L1(D_u) * L1(D_v) / Q_uv) (D the DCT matrix; what a forward of u8 pixels can
 *     produce, and the range dctq_plan_symbol_bytes compares with 511): e <= 1e-4
 *     (5e-5 where the plan decodes through the fp32 inverse);
 *   - any other int16 input, plans that decode through the fp32 inverse
 *     (non-adaptive plans whose bound over the forward range is <= 5e-5: q <= 71
 *     of the standard table): e grows linearly with the block's coefficient
 *     magnitudes x_k = |coef_k| / Q_k * S_u S_v,
 *       e_p = (G[p].x)(1 + 2^-24) + 2^-24 (128 + |L[p]|.x) + 1e-9   for pixel p
 *     (G = kInvErrG, |L| = kInvAbsL of csrc/idct8_bound.h; tools/inv_bound.py
 *     block_error), up to ~1e-3 for blocks of arbitrary int16 at q50..71;
 *   - any other int16 input, all other plans (fp64 inverse, one rounding to
 *     fp32): e = 2^-24 * max(|c|, 128) plus the fp64 error (1e-9 per 1024 of summed
 *     magnitude), so e <= 1e-4 for every pixel inside [0, 255].
 * var_num is read as given: any int32 is accepted, var = var_num / 4096 goes
 * through the reference's clamp min(1, max(0.1, var / 1000)).
 * var_num[k] (per block, as dctq_forward_quant writes it) is required for
 * adaptive plans; non-adaptive plans ignore var_num, which may be NULL.
 * coef[k] 16-byte aligned; dst[k] as every dctq_plane (pixels 8-byte aligned,
 * stride a multiple of 8 and >= width, width and height multiples of 8).
 * 128 B read + 64 B written per block (+ 4 B adaptive), against 384 B for
 * dctq_inverse and a host-side clamp and un-tiling.  Allocates nothing. */
int dctq_decode_planes(const dctq_plan *plan, const int16_t *const *coef, const int32_t *const *var_num,
                       const dctq_plane *dst, int nplanes, void *stream);

/* Decoder from symbols: run-length symbols -> u8 pixels in ONE launch, with no
 * coefficient buffer.  The contract is an equivalence: the pixels are, bit for
 * bit, what these two calls produce --
 *   1. dctq_rle_decode (symbol_bytes 4) or dctq_rle_decode16 (symbol_bytes 2) of
 *      the N blocks into one buffer c;
 *   2. dctq_decode_planes(plan, {c + 64 * first_k}, var_num, dst, nplanes), where
 *      first_k is the number of blocks in the planes before plane k
 * -- including streams whose runs walk past position 63 of a block (those values
 * are dropped, as the reference's run_length_decode drops them), and with the
 * error bound of dctq_decode_planes for the domain the decoded coefficients fall
 * in: a 4-byte symbol carries any int16, a 2-byte symbol any value in [-512, 511]
 * (the payload 0x200, which no encoder here emits, is -512).
 * Blocks are numbered as dctq_encode_planes numbers them: plane 0 first, then
 * plane 1, ...; within a plane frame, block row, block column.  N is the total
 * over the planes, N < 2^26; offsets holds N + 1 entries, offsets[b] the first
 * symbol of block b.  symbol_bytes 4: uint32_t (uint16_t)value | run << 16;
 * symbol_bytes 2: uint16_t (run & 63) << 10 | (value & 0x3FF), 0x0000 = (0, 64);
 * anything else is DCTQ_EINVAL.  The format is the stream's, not the plan's: a
 * plan whose dctq_plan_symbol_bytes is 4 may decode a 2-byte stream.  symbols
 * must be 4-byte aligned.
 * Everything else as dctq_decode_planes: var_num[k] per plane is required for
 * adaptive plans and ignored (may be NULL) otherwise; dst[k] as every dctq_plane;
 * bytes outside width x height are not touched.  S + 4 B read (S: the block's
 * symbols) + 64 B written per block (+ 4 B adaptive), against S + 4 + 128 + 128
 * + 64 B for the two calls.  Asynchronous on stream; allocates nothing. */
int dctq_decode_symbols_planes(const dctq_plan *plan, const void *symbols, int symbol_bytes,
                               const uint32_t *offsets, const int32_t *const *var_num,
                               const dctq_plane *dst, int nplanes, void *stream);

/* Zigzag + run-length symbols of quantized blocks (the reference's
 * run_length_encode, src/entropy.c:216-256 over block_to_zigzag :158-178, for
 * every block, blocks concatenated in order).  symbol = (uint16_t)value |
 * run << 16.  A block has 1 + (nonzeros among its first 63 zigzag elements)
 * symbols, so the stream is built in two steps:
 *   dctq_rle_count: offsets[b] = symbols before block b, offsets[nblocks] =
 *                   total (nblocks + 1 entries); `workspace` is device memory
 *                   of dctq_rle_workspace_bytes(nblocks) bytes, 4-byte aligned;
 *   dctq_rle_emit:  symbols[offsets[b] .. offsets[b+1]) for every block
 *                   (the caller sizes `symbols` from offsets[nblocks], or
 *                   64 * nblocks for the worst case).
 * nblocks < 2^26 (offsets are 32-bit). */
size_t dctq_rle_workspace_bytes(long long nblocks);
int dctq_rle_count(const int16_t *coef, long long nblocks, uint32_t *offsets, void *workspace, void *stream);
int dctq_rle_emit(const int16_t *coef, long long nblocks, const uint32_t *offsets, uint32_t *symbols, void *stream);
/* The inverse, run_length_decode (src/entropy.c:327-351) + zigzag_to_block
 * (:183-210) of every block: coef[b][64] from symbols[offsets[b] ..).
 * By that rule (pos += run; the value lands while pos < 64; pos++) a block
 * with no symbols decodes to zeros, and symbols after position 63 is passed,
 * or beyond a block's 64th, change nothing -- any symbols are a valid input.
 * dctq_rle_decode16: the same from 2-byte symbols ((run & 63) << 10 | (value &
 * 0x3FF), 0x0000 = (0, 64); dctq_encode_planes16's output);
 * symbols 4-byte aligned. */
int dctq_rle_decode16(const uint16_t *symbols, const uint32_t *offsets, long long nblocks, int16_t *coef,
                      void *stream);
int dctq_rle_decode(const uint32_t *symbols, const uint32_t *offsets, long long nblocks, int16_t *coef,
                    void *stream);

/* Bit-packed coefficient streams, format "bits v1": a fixed, table-free
 * variable-length code for the run-length symbols above (the reference stops at a
 * size estimate and has no bitstream writer; tools/bits_ref.py states the format
 * in plain Python).
 *   Layout.   Block b of the concatenated block numbering owns bytes
 *             [offsets[b], offsets[b+1]) of one byte buffer; offsets has N + 1
 *             uint32_t entries, offsets[N] the total.  Blocks follow each other
 *             with no gap; each starts on a byte boundary, its last byte padded
 *             with zero bits.
 *   Bits.     Bit i of a block is bit 7 - (i % 8) of its byte i / 8 (MSB first).
 *   ue(k), k >= 0.  x = k + 1 of bit length n: n - 1 zero bits, then x in n bits
 *             (2n - 1 bits: Exp-Golomb of order 0).
 *   Symbol (value v, run r).  ue(min(r, 64)), then ue(m), m = 2v - 1 for v > 0,
 *             else -2v (v = -32768: m = 65536, 33 bits).
 *   Block.    Its symbols in order, at most the first 64 (neither that nor the run
 *             clamp changes what dctq_rle_decode makes of the block); at most
 *             64 * 46 bits = 368 B, below 272 B for a stream of this encoder.
 *   Decoding a block.  pos = 0; read ue -> r, ue -> m;
 *             v = (int16_t)(m & 1 ? (m + 1) >> 1 : -(m >> 1)); pos += r; store v at
 *             zigzag position pos if pos < 64; pos += 1.  Stop when pos >= 64, or
 *             after 64 symbols, or at a bad code: a zero prefix of more than 16
 *             bits, or a code that would use a bit past the block's last byte.  A
 *             bad code ends the block and its symbol is dropped; positions never
 *             written are 0; an empty block decodes to zeros.  ANY bytes are
 *             therefore a valid input (with non-decreasing offsets), and nothing
 *             outside [offsets[b0], offsets[b0 + nb]) of a 64-block tile is read.
 *
 * dctq_bits_pack: the packed stream of a symbol stream (symbol_bytes 4: uint32_t
 * (uint16_t)value | run << 16, any values and runs; 2: uint16_t (run & 63) << 10 |
 * (value & 0x3FF), 0x0000 = (0, 64): the outputs of dctq_encode_planes /
 * dctq_encode_planes16, or anybody's), sym_offsets[b] the first symbol of block b
 * (nblocks + 1 entries).  offsets (nblocks + 1 entries, not sym_offsets) is always
 * complete; bytes at index >= bytes_capacity are not written, and bytes == NULL or
 * bytes_capacity 0 computes the offsets only -- as dctq_encode_planes treats its
 * symbols.  For ANY symbol input
 *   dctq_bits_decode(dctq_bits_pack(S)) == dctq_rle_decode(S).
 * symbols, sym_offsets, offsets and bytes 4-byte aligned; workspace: device memory
 * of dctq_bits_workspace_bytes(nblocks) bytes, 4-byte aligned; 1 <= nblocks < 2^26 and
 * 368 * nblocks < 2^32 (offsets are 32-bit: nblocks <= 11 671 106), else
 * DCTQ_EINVAL.  Four launches on stream (count, scan, fix-up, emit); allocates
 * nothing. */
size_t dctq_bits_workspace_bytes(long long nblocks);
int dctq_bits_pack(const void *symbols, int symbol_bytes, const uint32_t *sym_offsets, long long nblocks,
                   uint32_t *offsets, uint8_t *bytes, long long bytes_capacity, void *workspace, void *stream);
/* The inverse, and the counterpart of dctq_rle_decode: coef[b][64] (natural
 * order) from bytes[offsets[b] .. offsets[b+1]).  bytes of any alignment, offsets
 * 4-byte and coef 16-byte aligned; 1 <= nblocks < 2^26. */
int dctq_bits_decode(const uint8_t *bytes, const uint32_t *offsets, long long nblocks, int16_t *coef, void *stream);
/* Decoder from the packed stream: "bits v1" bytes -> u8 pixels in ONE launch,
 * with no coefficient buffer.  The contract is an equivalence: the pixels are,
 * bit for bit, what these two calls produce --
 *   1. dctq_bits_decode of the N blocks into one buffer c;
 *   2. dctq_decode_planes(plan, {c + 64 * first_k}, var_num, dst, nplanes), where
 *      first_k is the number of blocks in the planes before plane k
 * -- for any bytes, with the error bound of dctq_decode_planes for the domain
 * the decoded coefficients fall in (a packed symbol carries any int16).
 * Block numbering, var_num (required for adaptive plans, ignored otherwise),
 * dst, the bytes outside width x height that are not touched and N < 2^26 are as
 * for dctq_decode_symbols_planes.  P + 4 B read (P: the block's packed bytes) +
 * 64 B written per block (+ 4 B adaptive).  Asynchronous on stream; allocates
 * nothing. */
int dctq_decode_bits_planes(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                            const int32_t *const *var_num, const dctq_plane *dst, int nplanes, void *stream);

/* Random access into a packed stream: a block region and a frame range of every
 * plane -> u8 pixels in ONE launch, reading only the blocks inside the windows
 * (every block of bits v1 has its own byte offset).  win[k] places dst[k] in
 * stored plane k; dst[k] is the window's own picture, so its width x height x
 * nframes is the window's extent (as every decoder destination: multiples of 8,
 * pixels 8-byte aligned, any stride).  offsets is the WHOLE stream's N + 1 entries,
 * N = the blocks of the stored geometries in win, numbered plane by plane;
 * var_num[k] (adaptive plans) is the whole stored plane's array.  The contract is
 * an equivalence: the pixels are, bit for bit, what
 *   dctq_decode_bits_planes(plan, bytes, offsets, var_num, full, nplanes)
 * writes into full planes of the stored geometries, copied out of
 *   [frame0, frame0 + nframes) x [y0, y0 + height) x [x0, x0 + width)
 * of each -- for any bytes and any non-decreasing offsets.  Bytes of dst outside
 * width x height of each frame are not touched.
 *   Runs.  The work unit is a run: up to 64 consecutive stored blocks of one block
 *   row of one frame of one plane, inside that plane's window; a window wb blocks
 *   wide has ceil(wb / 64) runs per block row, numbered over window rows, frames,
 *   planes (tools/window_ref.py states the mapping in plain Python).  A run of nb
 *   blocks from stored block s0 reads offsets[s0 .. s0 + nb] and nothing outside
 *   [offsets[s0], offsets[s0 + nb]) of the bytes: no payload byte of a block that
 *   is in no run is read.  A window narrower than 64 blocks leaves part of each
 *   wave idle.
 * DCTQ_EINVAL, before any launch: NULL win or dst; a stored width or height that
 * is not a positive multiple of 8, or stored nframes < 1; x0 or y0 negative or not
 * a multiple of 8, frame0 < 0; a window that leaves the stored plane or a frame
 * range that leaves the stored frames; N >= 2^26; nplanes outside 1..4; a dst
 * that dctq_decode_bits_planes would refuse; a NULL plan, bytes or offsets;
 * missing var_num on an adaptive plan.  The geometry is checked first and needs
 * no device.  Asynchronous on stream; allocates nothing. */
typedef struct dctq_window {
    int width, height, nframes;   /* the STORED plane: what the stream's blocks are numbered over */
    int x0, y0, frame0;           /* first pixel column and row (multiples of 8) and first frame of the window */
} dctq_window;
int dctq_decode_bits_window_planes(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                                   const int32_t *const *var_num, const dctq_window *win,
                                   const dctq_plane *dst, int nplanes, void *stream);

/* The same window at 1/2, 1/4 or 1/8 size, straight from the packed stream in ONE
 * launch (what libjpeg's scale_denom gives a JPEG viewer): log2_scale 1, 2 or 3,
 * scale s = 2, 4, 8 and n = 8 / s, so every stored 8 x 8 block gives n x n pixels.
 * bytes, offsets, var_num and win[k] are as for dctq_decode_bits_window_planes (a
 * whole stored plane is simply the full window).  dst[k] is the REDUCED picture:
 * its width * s x height * s x nframes is the window's extent; width and height
 * are positive multiples of n (they need not be multiples of 8), pixels, stride
 * and frame_stride multiples of n bytes, stride >= width.  Bytes of dst outside
 * width x height of each frame are not touched.
 *   Definition (tools/scaled_ref.py states it in plain numpy).  Everything is IEEE
 *   fp64; every multiply and add is rounded separately (no fma); sums run left to
 *   right in ascending index.  Only the coefficients q[u][v], u, v < n, of a block
 *   are used (Q: the plan's quantization table, var_num: the block's):
 *     non-adaptive plans   x[u][v] = (double)q[u][v] * (1.0 / Q[u][v])
 *                          (the multiplication by 1 / Q of every decoder here)
 *     adaptive plans       sc = 2.0 - fmin(1.0, fmax(0.1, (var_num / 4096.0) / 1000.0))
 *                          x[u][v] = ((double)q[u][v] * Q[u][v]) * sc
 *                          x[0][0] = (double)q[0][0] * Q[0][0]
 *     temp[u][j] = sum over v of x[u][v] * Dn[v][j]
 *     out[i][j]  = sum over u of Dn[u][i] * temp[u][j]
 *     R          = out[i][j] * (n / 8.0) + 128.0
 *     pixel      = (uint8_t)rint(fmin(fmax(R, 0.0), 255.0)), ties to even
 *   with Dn the n-point DCT matrix as these literals (never through cos):
 *     D1 = [[1.0]]
 *     D2 = [[r, r], [r, -r]],  r = 0x1.6a09e667f3bcdp-1
 *     D4 = [[h, h, h, h], [a, b, -b, -a], [h, -h, -h, h], [b, -a, a, -b]],
 *          h = 0.5, a = 0x1.4e7ae9144f0fcp-1, b = 0x1.1517a7bdb3896p-2
 *   For s = 8 a pixel is the dequantized DC / 8 + 128: the block's mean.
 *   The pixels are exactly these for any bytes and any non-decreasing offsets: the
 *   coefficients are those dctq_bits_decode gives.  In zigzag order the n x n corner
 *   ends at position 24, 4 or 0, and the bit walk of a block stops once it is past
 *   it (positions only increase).
 * The read contract is the window decoder's: a run of nb blocks from stored block
 * s0 reads offsets[s0 .. s0 + nb] and nothing outside [offsets[s0], offsets[s0 + nb])
 * of the bytes.  DCTQ_EINVAL, before any launch and before a device is looked at:
 * log2_scale outside 1..3; a dst that breaks the rules above (or NULL pixels,
 * nframes < 1, a frame_stride below one frame); every geometry
 * dctq_decode_bits_window_planes refuses.  Then, as there: a NULL plan, bytes or
 * offsets; missing var_num on an adaptive plan.  Asynchronous on stream; allocates
 * nothing. */
int dctq_decode_bits_window_scaled_planes(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                                          const int32_t *const *var_num, const dctq_window *win,
                                          const dctq_plane *dst, int nplanes, int log2_scale, void *stream);

/* A window of a packed stream as a packed stream of its own, without decoding: no
 * block of bits v1 depends on another (no DC prediction, no tables, var_num per
 * block), so the stream of a block-aligned sub-picture is the sub-sequence of the
 * stored stream's blocks, and these two calls only move bytes.  win[k] is as for
 * dctq_decode_bits_window_planes; ext[k] is the window's extent in stored plane k
 * (where the decoder's dst[k] gave it), width and height positive multiples of 8.
 * The destination numbers the window's N' blocks as the window's own picture does:
 * plane by plane, then frames, block rows, block columns -- what
 * dctq_decode_bits_planes expects for planes of the extents.  For destination
 * block d that is stored block s (d_k, s_k inside plane k)
 *   win_offsets[d + 1] - win_offsets[d] = offsets[s + 1] - offsets[s]  (mod 2^32,
 *                                         exact: no clamp to 368),  win_offsets[0] = 0
 *   win_bytes[win_offsets[d] .. win_offsets[d + 1]) = bytes[offsets[s] .. offsets[s + 1])
 *   win_var_num[d] = var_num[k][s_k]
 * for any bytes and any non-decreasing offsets (tools/extract_ref.py states it in
 * plain numpy).  The window's payload cannot exceed the stream's, so 32-bit
 * offsets cannot wrap.
 * dctq_bits_window_offsets writes win_offsets[0 .. N'] (win_offsets[N'] is the
 * window's payload size) and, when var_num is not NULL, win_var_num[0 .. N') (one
 * array, the planes concatenated; var_num[k] is the whole stored plane's).  It
 * reads offsets[s] and offsets[s + 1] of the window's blocks only.  workspace:
 * device memory of dctq_bits_window_workspace_bytes(N') bytes, 4-byte aligned.
 * dctq_bits_window_gather writes the bytes, given the win_offsets of the first
 * call: one wave per run of the window decoder, a run being one contiguous byte
 * copy.  Nothing outside [offsets[s0], offsets[s0 + nb]) of a run is read and
 * nothing outside [win_offsets[d0], min(win_offsets[d0 + nb], capacity)) is
 * written: no byte at or past win_bytes + capacity, so a short buffer gets the
 * payload's first `capacity` bytes.  bytes and win_bytes may sit at any alignment
 * (source and destination alignment of a run are independent anyway); offsets,
 * win_offsets, var_num[k] and win_var_num are 4-byte aligned.  About 8 B read and
 * 4 B written per block by the first call (+ 8 B adaptive), P read and P written by
 * the second (P: the block's packed bytes).
 * DCTQ_EINVAL, before any launch and before a device is looked at: NULL win or ext;
 * an extent whose width or height is not a positive multiple of 8, or nframes < 1;
 * every geometry dctq_decode_bits_window_planes refuses (through the same check);
 * then a NULL or misaligned pointer, or var_num without win_var_num.  Asynchronous
 * on stream; allocate nothing. */
typedef struct dctq_extent {
    int width, height, nframes;   /* a window's extent in its stored plane; width and height multiples of 8 */
} dctq_extent;
size_t dctq_bits_window_workspace_bytes(long long window_blocks);
int dctq_bits_window_offsets(const uint32_t *offsets, const int32_t *const *var_num, const dctq_window *win,
                             const dctq_extent *ext, int nplanes, uint32_t *win_offsets, int32_t *win_var_num,
                             void *workspace, void *stream);
int dctq_bits_window_gather(const uint8_t *bytes, const uint32_t *offsets, const dctq_window *win,
                            const dctq_extent *ext, int nplanes, const uint32_t *win_offsets, uint8_t *win_bytes,
                            size_t capacity, void *stream);

/* A window of a packed stream REPLACED by another packed stream's blocks, without
 * decoding: the inverse direction of the two calls above.  The base stream (bytes,
 * offsets, var_num) holds the N blocks of nplanes stored planes; win[k] and ext[k]
 * describe plane k's window exactly as above; the patch stream (patch_bytes,
 * patch_offsets, patch_var_num) holds the N' blocks of the windows' own pictures, in
 * the numbering dctq_bits_window_offsets produces.  The result has the stored
 * geometry: for its block s (s_k inside plane k)
 *   out block s = patch block d  when s lies in its plane's window, d the block's
 *                                number in the window's own picture (d_k inside it),
 *               = base block s   otherwise;
 *   out_offsets[s + 1] - out_offsets[s] = that block's length (mod 2^32, exact: no
 *                                clamp to 368),  out_offsets[0] = 0
 *   out_bytes[out_offsets[s] .. out_offsets[s + 1]) = that block's bytes
 *   out_var_num[s] = patch_var_num[k][d_k] or var_num[k][s_k]
 * for any bytes and any non-decreasing offsets (tools/paste_ref.py states it in
 * plain numpy).  payload_bytes and patch_payload_bytes are the caller's statement of
 * the two streams' sizes, offsets[N] - offsets[0] and patch_offsets[N'] -
 * patch_offsets[0]: the result is at most their sum, which must stay below 2^32
 * because the result's offsets are 32-bit.
 * dctq_bits_paste_offsets writes out_offsets[0 .. N] (out_offsets[N] is the result's
 * payload size) and, when var_num is not NULL, out_var_num[0 .. N) (one array, the
 * planes concatenated; var_num[k] is the whole stored plane's, patch_var_num[k] the
 * whole window's).  var_num and patch_var_num are both given or both NULL.
 * workspace: device memory of dctq_bits_paste_workspace_bytes(N) bytes, 4-byte
 * aligned.
 * dctq_bits_paste_copy writes the bytes, given the out_offsets of the first call: one
 * wave per tile of 64 result blocks, whose bytes are contiguous; the tile is split
 * where the source changes or stops being consecutive, and each piece is one byte
 * copy as in dctq_bits_window_gather.  Nothing outside the source blocks' bytes is
 * read, and nothing outside [out_offsets[t0], min(out_offsets[t0 + nb], capacity))
 * of a tile is written: no byte at or past out_bytes + capacity, so a short buffer
 * gets the payload's first `capacity` bytes.  bytes, patch_bytes and out_bytes may
 * sit at any alignment; every offsets and var_num array is 4-byte aligned.  A stored
 * plane or a window narrower than 64 blocks gives many short pieces per tile: correct,
 * not fast.  The first call reads about 8 B and writes 4 B per block (+ 8 B adaptive),
 * the second reads about 16 B per block and reads and writes the result's payload.
 * DCTQ_EINVAL, before any launch and before a device is looked at: everything
 * dctq_bits_window_offsets refuses in win, ext and nplanes (through the same check);
 * then payload_bytes + patch_payload_bytes >= 2^32; then a NULL or misaligned
 * pointer, var_num without patch_var_num or the reverse, or var_num without
 * out_var_num.  Asynchronous on stream; allocate nothing. */
size_t dctq_bits_paste_workspace_bytes(long long stored_blocks);
int dctq_bits_paste_offsets(const uint32_t *offsets, const int32_t *const *var_num, const uint32_t *patch_offsets,
                            const int32_t *const *patch_var_num, size_t payload_bytes, size_t patch_payload_bytes,
                            const dctq_window *win, const dctq_extent *ext, int nplanes, uint32_t *out_offsets,
                            int32_t *out_var_num, void *workspace, void *stream);
int dctq_bits_paste_copy(const uint8_t *bytes, const uint32_t *offsets, const uint8_t *patch_bytes,
                         const uint32_t *patch_offsets, const dctq_window *win, const dctq_extent *ext, int nplanes,
                         const uint32_t *out_offsets, uint8_t *out_bytes, size_t capacity, void *stream);

/* Self-contained container, format "frame v1": everything a decoder of a "bits
 * v1" stream needs, in one byte buffer (tools/frame_ref.py states it in plain
 * Python).  Little-endian.  A block of bits v1 is at most 368 B, so the N + 1
 * uint32_t offsets hold no more than one byte of length per block (two when a
 * block exceeds 255 B), and a scan on the device restores them.
 *   Header, 48 + 16 * nplanes bytes:
 *      0  8 B   magic "DCTQFRM1"
 *      8  u32   header_bytes = 48 + 16 * nplanes
 *     12  u8    quality, 1..100 (the plan's, after quant_init's clamp)
 *     13  u8    adaptive, 0 or 1
 *     14  u8    nplanes, 1..4
 *     15  u8    length_bytes, 1 or 2
 *     16  u8    colour: 0 = plain planes; 1 = the three planes are the Y, Cb, Cr
 *               of dctq_rgb_to_ycbcr_planes (nplanes 3; Cb and Cr of one size,
 *               plane 0's or half of it in both directions; equal nframes)
 *     17..23    reserved, written 0; a reader refuses anything else
 *     24  u64   nblocks = sum over the planes of nframes * (width / 8) *
 *               (height / 8); 1 <= nblocks <= 11 671 106
 *     32  u64   payload_bytes, < 2^32
 *     40  u64   total_bytes, the container's length
 *     48 + 16 k   4 x u32   plane k: width, height, nframes, 0; width and height
 *               multiples of 8 and >= 8, nframes >= 1
 *   Sections, each starting at the next multiple of 16 from the container's
 *   first byte (padding written 0, ignored on read), in this order:
 *     lengths   nblocks * length_bytes bytes: entry b = offsets[b+1] - offsets[b]
 *               as u8 or u16;
 *     var_num   4 * nblocks bytes of int32 in the concatenated block numbering,
 *               present only when adaptive;
 *     payload   payload_bytes bytes of bits v1.  total_bytes is its end.
 *   Reading.  A length above 368 reads as 368 (with the nblocks limit a 32-bit
 *   scan cannot wrap); offsets[0] = 0.  The sum of the lengths must equal
 *   payload_bytes.  Offsets rebuilt from lengths are non-decreasing, which with
 *   the sum check is the precondition under which bits v1 decodes any bytes
 *   without reading outside the payload.
 *   A reader refuses, before it decodes anything: a buffer shorter than 48 B,
 *   than header_bytes or than total_bytes; a bad magic; a field out of range;
 *   header_bytes or nblocks inconsistent with the plane records; a section that
 *   ends past total_bytes; a lengths sum that differs from payload_bytes.
 *
 * Cropped pictures, format "frame c1": magic "DCTQFRC1", identical to frame v1 in every
 * byte and rule but one: a plane record's fourth word is pad_right | pad_bottom << 16, the
 * columns and rows of that stored plane to drop after decoding (the edge padding of
 * dctq_rgb_to_ycbcr_pad_planes / dctq_pad_planes).  width, height and nblocks stay the
 * stored, padded ones, and the decode path is frame v1's.  Plain planes: each pad is 0..7.
 * colour: plane 0 carries 0..15 (4:2:0) or 0..7 (4:4:4), planes 1 and 2 carry 0.  pad_right <
 * width and pad_bottom < height.  At least one fourth word is non-zero: a picture that needs
 * no crop is written as frame v1, so every picture has one encoding.  A reader refuses
 * anything else before it decodes; frame v1 readers go on refusing a non-zero fourth word.
 *
 * dctq_block_lengths: lengths[b] = min(offsets[b+1] - offsets[b] (mod 2^32),
 * 255 or 65535), nblocks entries of length_bytes (1 or 2) bytes each; nothing
 * past the last entry is written.  max_length[0] = the largest unsaturated
 * difference (written by the call; no initialisation needed), so the caller
 * sees whether length_bytes sufficed.  offsets has nblocks + 1 entries.
 * dctq_block_offsets: the inverse: offsets[0 .. nblocks] = exclusive prefix
 * sums of min(length, 368); offsets[nblocks] = the total.  workspace: device
 * memory of dctq_block_offsets_workspace_bytes(nblocks) bytes, 4-byte aligned.
 * Both: offsets, lengths and max_length 4-byte aligned; 1 <= nblocks <=
 * 11 671 106 and length_bytes 1 or 2, else DCTQ_EINVAL, as for a NULL pointer.
 * Asynchronous on stream; allocate nothing.  About 4 + length_bytes bytes moved
 * per block. */
int dctq_block_lengths(const uint32_t *offsets, long long nblocks, int length_bytes, void *lengths,
                       uint32_t *max_length, void *stream);
size_t dctq_block_offsets_workspace_bytes(long long nblocks);
int dctq_block_offsets(const void *lengths, int length_bytes, long long nblocks, uint32_t *offsets,
                       void *workspace, void *stream);

/* Per-block Huffman size: bits[b] = what the reference's pipeline
 * reports for block b coded on its own (tests/test_entropy.c:329-341):
 * run_length_encode -> build_huffman_codes -> get_encoded_size
 * (src/entropy.c:216-256, 261-328, 363-399), i.e. sum over the block's RLE
 * symbols of (Huffman code length + 8).  The code lengths of one symbol depend
 * on the reference heap's tie order, their sum does not (Huffman trees are
 * optimal); the codes themselves are not produced.  coef 16-byte aligned. */
int dctq_huffman_bits(const int16_t *coef, long long nblocks, uint32_t *bits, void *stream);
/* The same per-block size straight from pixels: the whole per-block loop of
 * tests/test_entropy.c:300-341 (create_block_from_pixels -> dct_forward ->
 * quantize -> run_length_encode -> build_huffman_codes -> get_encoded_size) for
 * every block of up to 4 planes, blocks numbered plane 0 first (as
 * dctq_encode_planes).  Equal to dctq_forward_quant_planes followed by
 * dctq_huffman_bits over the concatenated coefficients, but the coefficients
 * never leave the chip.  bits: 4-byte aligned, one entry per block. */
int dctq_huffman_bits_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, uint32_t *bits,
                             void *stream);
/* Per-block distortion straight from pixels, the other column of the reference's
 * per-block report (tests/test_entropy.c:300-393: forward -> quantize ->
 * dequantize -> inverse -> clamp -> squared error), in ONE launch: for block b,
 *   sse[b] = sum over its 64 pixels of (src - dec)^2,
 * where dec is, bit for bit, the u8 pixel that dctq_forward_quant_planes(plan,
 * planes, ..., coef, var_num) followed by dctq_decode_planes(plan, coef, var_num,
 * dst) writes at that position: dec = (uint8) rne(clamp(r, 0, 255)) of the fp32
 * recon r of dctq_round_trip_planes (the fp32 inverse where the plan's bound
 * admits it, fp64 otherwise; adaptive plans use the block's own var_num, which
 * the caller neither supplies nor receives).  No coefficient, recon or picture
 * buffer exists: 64 B read and 4 B written per block.  Blocks are numbered as
 * dctq_huffman_bits_planes numbers them (plane 0 first; within a plane by frame,
 * block row, block column); their total N must stay below 2^26.  sse[b] <=
 * 64 * 255^2 = 4 161 600.  sse: 4-byte aligned, N entries.  Asynchronous on
 * stream; allocates nothing.  DCTQ_EINVAL: a NULL pointer, nplanes outside
 * 1..4, bad plane geometry, N >= 2^26.
 * Relation to the reference's PSNR: the reference squares the error of the
 * clamped but UNROUNDED double c = clamp(recon, 0, 255); this entry point
 * reports the error of the u8 picture a decoder outputs.  With |dec - c| <=
 * T = 0.5 + 1e-4 per pixel (rounding plus the recon bound; the coefficients are
 * this call's own forward of u8 pixels, inside the plan's forward range, so the
 * bound of dctq_decode_planes holds without condition) and e = src - c,
 *   sum max(|e| - T, 0)^2 <= sse[b] <= sum (|e| + T)^2.
 * PSNR over any set of blocks: 10 log10(255^2 * 64 * blocks / sum of sse). */
int dctq_distortion_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, uint32_t *sse,
                           void *stream);

/* Colour front and back end: an RGB picture stack to the Y, Cb, Cr planes the entry
 * points above take, and decoded planes back to a picture.  The reference has no
 * colour code; the definition is this library's own, exact and integer, and
 * tools/color_ref.py states it in plain Python.  Full-range BT.601 (JFIF) in 16-bit
 * fixed point on int32, >> an arithmetic shift:
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16
 * (all three lie in [0, 255] for every colour: no clamp), and back, with
 * cb = Cb - 128, cr = Cr - 128 and clamp to [0, 255]:
 *   R = clamp(Y + (( 91881 cr + 32768) >> 16))
 *   G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16))
 *   B = clamp(Y + ((116130 cb + 32768) >> 16))
 * Subsampling is read from the geometry: chroma planes of luma's width and height
 * are 4:4:4; of exactly half in both, 4:2:0, where chroma sample (i, j) =
 * (c00 + c01 + c10 + c11 + 2) >> 2 over the u8 Cb (Cr) of pixels (2i..2i+1,
 * 2j..2j+1), and on the way back serves those four pixels; anything else is
 * DCTQ_EINVAL.  In 4:4:4 the round trip is within 1 of the source in every channel.
 *
 * A packed or planar RGB picture stack in device memory.  RGB: pixel_step 3,
 * channel_stride +1; RGBX: 4, +1; BGR / BGRX: the same with channel_stride -1 and
 * pixels at the R byte (the third of the pixel); planar: pixel_step 1 and
 * channel_stride the distance between the channel planes, either sign. */
typedef struct {
    void *pixels;              /* the R byte of pixel (0,0) of frame 0 */
    long long stride;          /* bytes between rows */
    long long frame_stride;    /* bytes between frames */
    long long channel_stride;  /* bytes from R to G and from G to B: +1 (RGB/RGBX), -1 (BGR/BGRX),
                                  or a plane size, either sign (planar) */
    int pixel_step;            /* bytes between pixels of one channel: 1 (planar), 3 or 4 (interleaved) */
    int width, height, nframes;
} dctq_rgb;
/* No plan: the transform does not depend on quality.  y, cb, cr as every dctq_plane
 * (so 4:2:0 needs luma multiples of 16); all three and the RGB stack agree on
 * nframes, y and the RGB stack on width and height.  RGB alignment: the lowest byte
 * address of pixel (0,0) -- pixels, or pixels - 2 when channel_stride is -1 -- is
 * 4-byte aligned, stride and frame_stride are multiples of 4 (and, planar,
 * channel_stride too); stride covers a row, frame_stride a frame.  The fourth byte
 * of a 4-byte pixel is ignored on input and written as 255 on output.  Bytes outside
 * width x height of any destination -- row padding, the gaps between frames and
 * channels -- are not touched.  3 B read and 1.5 B written per pixel in 4:2:0 (4 and
 * 1.5 for 4-byte pixels; 3 and 3 in 4:4:4), the reverse for dctq_ycbcr_to_rgb_planes;
 * one launch each, asynchronous on stream; allocates nothing. */
int dctq_rgb_to_ycbcr_planes(const dctq_rgb *src, const dctq_plane *y, const dctq_plane *cb,
                             const dctq_plane *cr, void *stream);
int dctq_ycbcr_to_rgb_planes(const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr,
                             const dctq_rgb *dst, void *stream);

/* Pictures of any size: edge-pad on the way in, crop on the way out (tools/color_ref.py
 * pad_edge / forward_padded / inverse_cropped).  With m = 8 in 4:4:4 and m = 16 in 4:2:0, a
 * picture of W x H (both >= 1) is extended to W' = ceil(W / m) m by H' = ceil(H / m) m,
 *   pixel'(x, y) = pixel(min(x, W - 1), min(y, H - 1)),
 * and the transform and the 2x2 chroma averaging above apply to the extended picture
 * unchanged.  On the way back the inverse above runs on the W' x H' planes and only the
 * pixels with x < W and y < H are written.
 * The dctq_rgb carries the true width and height; y must be exactly W' x H', cb and cr equal
 * to it (4:4:4) or exactly half of it (4:2:0); nframes agree everywhere; the planes obey the
 * rules of every dctq_plane.  The RGB stack needs NO alignment: any address, any stride >=
 * width * pixel_step, any frame_stride that covers a frame; pixel_step 1, 3 or 4; channel_stride
 * +1 or -1 (interleaved) or, planar, any distance of at least one row, either sign.  Anything
 * else is DCTQ_EINVAL before any launch, and nothing is written.
 * Writes: the planes over their whole W' x H' and nowhere else; an RGB destination at exactly
 * the bytes of its W x H pixels (the fourth byte of a 4-byte pixel is written 255) -- row
 * padding, the bytes between W * pixel_step and stride, and the gaps between frames and
 * channels stay untouched.  Reads: only bytes of the source's W x H pixels (of a 4-byte pixel
 * also its fourth byte) -- no byte beside them, aligned or not; the planes are read only
 * inside W' x H'.  A picture that needs neither padding nor unaligned access gives the bytes
 * the aligned entry points give.  One launch each, asynchronous on stream; allocate nothing. */
int dctq_rgb_to_ycbcr_pad_planes(const dctq_rgb *src, const dctq_plane *y, const dctq_plane *cb,
                                 const dctq_plane *cr, void *stream);
int dctq_ycbcr_to_rgb_crop_planes(const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr,
                                  const dctq_rgb *dst, void *stream);
/* The same edge replication for 1..4 plain u8 planes in ONE launch: src[k] is any width x
 * height x nframes (all >= 1) with stride >= width and no alignment rule (its `multiples of
 * 8` do not apply); dst[k] is a dctq_plane of ceil(width / 8) 8 x ceil(height / 8) 8 and the
 * same nframes, written over its whole size: dst(x, y) = src(min(x, width - 1), min(y,
 * height - 1)).  A src that is already whole blocks is copied.  Reads only bytes of src's
 * width x height.  DCTQ_EINVAL: a NULL pointer, nplanes outside 1..4, a dst of another size, a
 * dst that starts where a src does (no padding in place). */
int dctq_pad_planes(const dctq_plane *src, const dctq_plane *dst, int nplanes, void *stream);

/* The calling thread forgets `stream` (call it before hipStreamDestroy): the
 * library keeps no per-stream device memory, only each thread's list of the
 * streams it has launched on, and a stream later created at the same handle
 * then gets its first call isolated again (that list is also keyed by the
 * runtime's stream id, so hosts that skip this call stay correct wherever the
 * runtime tells the two streams apart).  Returns DCTQ_OK. */
int dctq_stream_release(void *stream);

/* Optional diagnostics: if non-NULL, *counter (device, uint64) is incremented
 * by the number of coefficients resolved by the exact fp64 tie path in later
 * dctq_forward_quant / _planes / dctq_round_trip_planes calls on this plan (costs one atomic per affected wave). */
int dctq_plan_set_fallback_counter(dctq_plan *plan, unsigned long long *counter);

/* Synthetic frames (counter-based splitmix64; identical to the oracle's
 * generator): kind 0 uniform, 1 smooth, 2 constant 8x8 blocks, 3 extremes.
 * Frame f uses seed + f. */
int dctq_synth(uint64_t seed, int kind, const dctq_plane *dst, void *stream);

/* Device helpers so a plain C host needs no HIP headers. */
int dctq_device_count(int *count);
int dctq_set_device(int device);
int dctq_malloc(void **ptr, size_t bytes);
int dctq_free(void *ptr);
int dctq_memcpy_htod(void *dst, const void *src, size_t bytes);
int dctq_memcpy_dtoh(void *dst, const void *src, size_t bytes);
int dctq_synchronize(void *stream);
const char *dctq_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif
