// dct_amd/csrc/dctq_internal.h -- shared between the kernels and the C-ABI shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <optional>
#include <type_traits>

namespace dctq {

// The HSA runtime calls srand()/rand() (libhsa-runtime64 imports both), which
// would reseed or advance the HOST APPLICATION's rand() stream; the reference's
// own tests draw their blocks from rand() (tests/test_quantization.c:127,134).
// The entry points that allocate or free device memory or set up devices (plan
// create / destroy, the device-memory helpers, the legacy per-block API, the
// diagnostic library) hold one of these while they may reach the HIP runtime:
// glibc's global random state is swapped to a private one for the duration
// (initstate/setstate keep the caller's state and position intact).  Those entry
// points are serialised by it (recursive, so nesting is fine); the batched launch
// entry points are not (LaunchIsolation below).
class RandIsolation {
  public:
    RandIsolation();
    ~RandIsolation();
    RandIsolation(const RandIsolation &) = delete;
    RandIsolation &operator=(const RandIsolation &) = delete;

  private:
    char *saved_;
};
#define DCTQ_ENTRY ::dctq::RandIsolation dctq_rand_isolation_

// The batched launch entry points (and dctq_synchronize) do NOT serialise: the
// runtime's one rand() user (srand(now); rand() inside libhsa-runtime64, reached
// when the runtime initialises or creates device resources -- a stream's first
// hardware queue, a module's first load) can only run on a thread's FIRST call of
// an entry point on a stream, so that call is isolated as above; every later call
// of the thread with the same (device, stream, entry point) takes no lock and
// touches no global state (the reference API is reentrant and keeps
// no mutable global state).  `entry` names the entry point: one bit of a 64-bit mask each.
enum Entry : int {
    kEntryForwardQuantPlanes,
    kEntryRoundTripPlanes,
    kEntryEncodePlanes,
    kEntryEncodePlanes16,
    kEntryForwardFloat,
    kEntryInverse,
    kEntryDecodePlanes,
    kEntryDecodeSymbolsPlanes,
    kEntrySynth,
    kEntryRleCount,
    kEntryRleEmit,
    kEntryRleDecode,
    kEntryRleDecode16,
    kEntryHuffmanBits,
    kEntryHuffmanBitsPlanes,
    kEntryDistortionPlanes,
    kEntryBitsPack,
    kEntryBitsDecode,
    kEntryDecodeBitsPlanes,
    kEntryRgbToYcbcrPlanes,
    kEntryYcbcrToRgbPlanes,
    kEntryBlockLengths,
    kEntryBlockOffsets,
    kEntrySynchronize,
    kEntryRgbToYcbcrPadPlanes,
    kEntryYcbcrToRgbCropPlanes,
    kEntryPadPlanes,
    kEntryDecodeBitsWindowPlanes,
    kEntryDecodeBitsWindowScaledPlanes,
    kEntryBitsWindowOffsets,
    kEntryBitsWindowGather,
    kEntryBitsPasteOffsets,
    kEntryBitsPasteCopy,
};
static_assert(kEntryBitsPasteCopy < 64, "LaunchIsolation keeps one bit per entry point in a uint64_t");
class LaunchIsolation {
  public:
    LaunchIsolation(const void *stream, Entry entry);
    LaunchIsolation(const LaunchIsolation &) = delete;
    LaunchIsolation &operator=(const LaunchIsolation &) = delete;

  private:
    std::optional<RandIsolation> iso_;
};
#define DCTQ_LAUNCH(stream, entry) ::dctq::LaunchIsolation dctq_launch_isolation_((stream), (entry))

// Whether some entry point has already initialised the HIP runtime in this
// process: until then any HIP call (even hipGetDevice) may initialise it, and so
// must be isolated.  forget_stream: the calling thread drops `stream` from its
// launch-isolation list (dctq_stream_release).
bool runtime_started();
void note_runtime_started();
void forget_stream(const void *stream);
// legacy.hip: per-thread lanes of the per-block API created so far / pooled (diagnostics)
void legacy_lane_counts(int *made, int *pooled);


// Resident workgroups per CU of `kernel` at `threads` per workgroup (>= 1).
template <typename K>
inline int resident_per_cu(K kernel, int threads) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0) != hipSuccess || nb < 1) nb = 1;
    return nb;
}

// The diagnostic grid limit (isolation.hip; dctq_diag.h dctq_diag_set_grid_limit): 0 = none,
// else the most workgroups any persistent grid-stride launch of this library instance gets,
// so a test-sized input gives every wave several batches.  Only the diagnostic library
// exports a setter: in the product it stays 0.  t_last_grid: the grid of the calling
// thread's most recent such launch (dctq_diag_last_grid).
extern std::atomic<uint32_t> g_grid_limit;
extern thread_local uint32_t t_last_grid;
// The grid a persistent grid-stride launch gets for the `grid` workgroups it asks for.
inline uint32_t limited_grid(uint32_t grid) {
    const uint32_t limit = g_grid_limit.load(std::memory_order_relaxed);
    if (limit && grid > limit) grid = limit;
    t_last_grid = grid;
    return grid;
}

// The grid of a persistent grid-stride kernel over `nbatch` batches, one per wave and
// step: a workgroup per `Waves` batches, at most `mult` x the resident workgroups (and
// the diagnostic limit).
// The occupancy is cached per kernel (the kernel is a template argument, so every
// instantiation has its own static; thread-safe initialisation): every device this
// library runs on is a gfx950.
template <auto Kernel, int Threads, int Waves>
inline uint32_t persistent_grid(uint64_t nbatch, int num_cus, int mult) {
    static const int per_cu = resident_per_cu(Kernel, Threads);
    const uint64_t want = (nbatch + Waves - 1) / Waves;
    const uint64_t cap = (uint64_t)num_cus * per_cu * mult;
    return limited_grid((uint32_t)(want < cap ? want : cap));
}
// ... and its launch; Mult is the kernel's own grid multiplier (kGridMult below).
template <auto Kernel, int Threads, int Waves, int Mult, typename... A>
inline hipError_t launch_persistent(uint64_t nbatch, int num_cus, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(Kernel, dim3(persistent_grid<Kernel, Threads, Waves>(nbatch, num_cus, Mult)), dim3(Threads), 0,
                       stream, args...);
    return hipGetLastError();
}

// f(std::bool_constant<b0>(), std::bool_constant<b1>(), ...): run-time flags into the
// template arguments of a kernel, one leaf per combination.
template <typename F>
inline auto with_bools(F &&f) {
    return f();
}
template <typename F, typename... B>
inline auto with_bools(F &&f, bool b0, B... rest) {
    return with_bools(
        [&](auto... c) { return b0 ? f(std::true_type(), c...) : f(std::false_type(), c...); }, rest...);
}
// f(ADAPTIVE, INV32) for a plan's inverse: the three legal leaves (0,0), (0,1), (1,0) -- the
// fp32 inverse is the non-adaptive plans', so (1,1) is never instantiated.
template <typename F>
inline auto with_inverse(F &&f, bool adaptive, bool inv_f32) {
    if (adaptive) return f(std::true_type(), std::false_type());
    return inv_f32 ? f(std::false_type(), std::true_type()) : f(std::false_type(), std::false_type());
}

// Persistent grid-stride kernels launch kGridMult times their resident
// workgroups; the extra ones queue and start as the first wave of workgroups
// retires, which evens out batches of unequal cost and the launch tail
// (profiles/r02/grid_mult_ab.log: x8 is 2.4-7 % faster than x1 on the forward,
// round trip, inverse and encoder, outputs identical; x16/x32 regress on
// uniform input).
constexpr int kGridMult = 8;
// Cache policy of the bulk 1 KiB output stores of every streaming kernel
// (buffer-store aux bits, gfx950: 1 sc0, 2 nt, 16 sc1).  Non-temporal: the
// written lines are never re-read by the kernel that writes them.
constexpr int kNtAux = 2;
// Word 3 of every buffer descriptor here: DATA_FORMAT 32 (bit 17) and nothing else --
// a raw buffer, byte offsets, accesses at or past num_records dropped (loads read 0).
constexpr int kRsrcFlags = 0x00020000;
// s_waitcnt vmcnt(0): the wave's loads have arrived and its stores have read their
// data VGPRs (and left the CU).
__device__ __forceinline__ void retire_stores() { __builtin_amdgcn_s_waitcnt(0x0F70); }
// s_waitcnt lgkmcnt(0): the wave's LDS (and scalar) accesses are done.
__device__ __forceinline__ void lgkm_wait() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// n / d and n % d by multiply-high, valid for 0 <= n < 2^31 (host-built magic).
struct FastDiv {
    uint32_t d, m, s;
};
FastDiv make_fastdiv(uint32_t d);
__device__ __forceinline__ uint32_t fdiv(uint32_t n, FastDiv f) { return (__umulhi(n, f.m) + n) >> f.s; }

// Wave-uniform per-plan constants of the fp32 fast path, passed by value in the
// kernel arguments so every access is a scalar load into SGPRs.
struct FastTables {
    float w[64];    // S_i S_j / Q_ij  (AAN output scale folded into 1/Q)
    float thr[64];  // |frac| above which the exact fp64 path decides (guard band)
    float thr2[64]; // thr^2 rounded down: flag iff thr2 - f*f < 0
    // v2 processing order: slot p = 16*cp + 2*i + h holds coefficient 8*i + 2*cp + h
    float ws[64], t2s[64];
};

// Per-plan device-resident tables (runtime-indexed: exact tie path, inverse).
struct DevTables {
    double dct[64];    // D of src/dct.c:17-30, bit-identical to the host expression
    double quant[64];  // Q of src/quantization.c:51-99
    double dequant[64];// 1/Q (src/quantization.c:101-111)
    double iscale[64]; // inverse path: 1/Q * S_i S_j (non-adaptive dequant folded with AAN^T scale)
    double qscale[64]; // inverse path (adaptive): Q * S_i S_j
    double s2[64];     // S_i S_j
    double s1[8];      // S_k: AAN output scale X_k = S_k y_k (per-slot factors of the paired fp64 kernels)
    float iscale32[64];// fl32(iscale): the fused round trip's fp32 inverse (plans admitted by idct8_bound.h)
    FastTables fast;   // device copy of the fast-path tables (v2 reads them per batch)
    // quantized DC of a CONSTANT block of centred value v-128, computed on the
    // host in the reference's order (src/dct.c:57-74, src/quantization.c:124):
    // resolves the DC ties of flat blocks without the exact path.  The DC is
    // never adjusted by adaptive plans (src/quantization.c:198-199).
    int16_t dc_const[256];
};

struct PlaneArgs {
    const uint8_t *src;
    long long stride, frame_stride;
    int bw;             // blocks per row
    int nblk_frame;     // blocks per frame
    int nblk;           // total blocks (all frames), < 2^31
    FastDiv div_bw, div_frame;  // by bw and by nblk_frame
    uint32_t span;      // bytes from src to one past the last pixel when < 2^32, else 0 (load_rows<true>)
};

// Up to kMaxPlanes planes (e.g. Y, Cb, Cr) processed by ONE forward launch.
constexpr int kMaxPlanes = 4;
struct PlaneSet {
    PlaneArgs pl[kMaxPlanes];
    int16_t *coef[kMaxPlanes];
    int32_t *var[kMaxPlanes];          // all NULL or all set
    uint32_t first[kMaxPlanes + 1];    // global index of each plane's first 64-block batch; first[n] = total
    int n;
};

// The encoder's planes: PlaneSet (coef/var unused) plus each plane's first block
// in the concatenated block numbering of the offsets array; blk_first[n] = total.
struct EncodeSet {
    PlaneSet ps;
    uint32_t blk_first[kMaxPlanes + 1];
};

// The fused round trip's planes: forward outputs as PlaneSet, plus fp32 recon per plane.
struct RoundTripSet {
    PlaneSet ps;
    float *recon[kMaxPlanes];
};

// The pixel decoder's planes (decode.hip): pl[k].src is the DESTINATION plane, written
// through; coefficients (and var_num, adaptive plans) in, block-major.
struct DecodeSet {
    PlaneArgs pl[kMaxPlanes];
    const int16_t *coef[kMaxPlanes];
    const int32_t *var[kMaxPlanes];    // adaptive plans: all set; otherwise unused
    uint32_t first[kMaxPlanes + 1];    // global index of each plane's first 32-block batch; first[n..] = total
    int n;
};

// The symbol decoder's planes (decode_symbols.hip): pl[k].src is the DESTINATION plane;
// blocks numbered over the concatenated planes, as the encoder numbers them.
struct SymbolSet {
    PlaneArgs pl[kMaxPlanes];
    const int32_t *var[kMaxPlanes];        // adaptive plans: all set; otherwise unused
    uint32_t blk_first[kMaxPlanes + 1];    // each plane's first block; blk_first[n..] = total (< 2^26)
    int n;
};

// The window decoder's planes (decode_window.hip): pl[k].src is the DESTINATION, the window's
// own picture, so pl[k].bw is the window's width in blocks; win[k] places it in the stored
// plane.  A run is up to 64 consecutive stored blocks of one window row (tools/window_ref.py);
// runs are numbered over window rows, frames, planes.  The scaled decoder (decode_scaled.hip)
// takes the same set: there pl[k] describes the REDUCED picture, n = 8 / scale pixels a block
// side, so stride, frame_stride and span are the reduced picture's and bw, nblk_frame and nblk
// still count the window's blocks.
struct WindowPlane {
    uint32_t first;       // the window's first block in the concatenated stored numbering (offsets' index)
    uint32_t var_first;   // ... and inside its stored plane (var_num's index)
    uint32_t bw, nblk_frame;  // the STORED plane's blocks per row and per frame
    uint32_t rows;        // the window's block rows per frame
    uint32_t runs_row;    // runs per window row: ceil(pl[k].bw / 64)
    FastDiv div_runs, div_rows;  // by runs_row and by rows
};
struct WindowSet {
    PlaneArgs pl[kMaxPlanes];
    const int32_t *var[kMaxPlanes];        // adaptive plans: all set (the whole stored plane's); otherwise unused
    WindowPlane win[kMaxPlanes];
    uint32_t run_first[kMaxPlanes + 1];    // each plane's first run; run_first[n..] = total (< 2^26)
    int n;
};

// The colour kernels' arguments (color.hip): an RGB picture stack and its Y, Cb, Cr planes.
// A patch is 8 pixels by 2 rows (4:2:0) or 1 row (4:4:4); patches are numbered in raster
// order over the frames, npatch < 2^31.
struct ColorArgs {
    uint8_t *rgb;               // interleaved: the lowest byte of pixel (0,0) of frame 0; planar: its R byte
    long long rgb_stride, rgb_frame_stride;
    long long channel_stride;   // planar: bytes from the R plane to G's and from G's to B's
    int swap;                   // interleaved: the pixel's bytes are B, G, R in memory
    uint8_t *y, *cb, *cr;       // read by the inverse, written by the forward
    long long y_stride, y_frame_stride, cb_stride, cb_frame_stride, cr_stride, cr_frame_stride;
    uint32_t npatch, per_row, per_frame;
    FastDiv div_row, div_frame;  // by per_row and by per_frame
};

// The padding colour kernels' arguments (color_pad.hip): c describes the RGB stack (any
// alignment) and the planes of the EXTENDED picture, over which the patches are numbered;
// width x height is the true picture.
struct ColorPadArgs {
    ColorArgs c;
    uint32_t width, height;
};
// dctq_pad_planes (color_pad.hip): plane k's w x h source (any alignment) and its destination of
// per_row * 8 columns; a patch is 8 pixels of one destination row, npatch of them < 2^31.
struct PadPlane {
    const uint8_t *src;
    uint8_t *dst;
    long long src_stride, src_frame_stride, dst_stride, dst_frame_stride;
    uint32_t width, height, npatch, per_row, per_frame;
    FastDiv div_row, div_frame;  // by per_row and by per_frame
};
struct PadSet {
    PadPlane pl[kMaxPlanes];
    int n;
};

// Plane selection over a PlaneSet or a DecodeSet (64- or 32-block batches).
// Coefficient / var_num pointer of plane k (wave-uniform or not: a select chain, no
// indexed kernel-argument loads).
template <typename Set>
__device__ __forceinline__ auto coef_of(const Set &ps, uint32_t k) {
    auto c = ps.coef[0];
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) c = k == (uint32_t)i ? ps.coef[i] : c;
    return c;
}
template <typename Set>
__device__ __forceinline__ auto var_of(const Set &ps, uint32_t k) {
    auto v = ps.var[0];
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) v = k == (uint32_t)i ? ps.var[i] : v;
    return v;
}
// First global batch of plane k (wave-uniform k): a select chain over the batch
// prefixes, which sit in SGPRs for the whole kernel -- an indexed kernel-argument
// load here was one more scalar-cache round trip in front of every prefetch.
template <typename Set>
__device__ __forceinline__ uint32_t first_of(const Set &ps, int k) {
    uint32_t f = 0u;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) f = k == i ? ps.first[i] : f;
    return f;
}
// Plane of global batch g (wave-uniform).
template <typename Set>
__device__ __forceinline__ int plane_of(const Set &ps, uint32_t g) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) k += (i < ps.n && g >= ps.first[i]) ? 1 : 0;
    return k;
}
// Plane of block b < blk_first[kMaxPlanes] of a SymbolSet's concatenated numbering, and a
// plane's first block (select chains: b and k may differ by lane).
__device__ __forceinline__ int plane_of_block(const SymbolSet &ss, uint32_t b) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) k += b >= ss.blk_first[i] ? 1 : 0;
    return k;
}
__device__ __forceinline__ uint32_t block_first_of(const SymbolSet &ss, int k) {
    uint32_t f = 0u;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) f = k == i ? ss.blk_first[i] : f;
    return f;
}

// The product forward (fdct8.hip): fdct8_quant_v3 over every plane of ps, every plan.
hipError_t launch_fdct8_quant(const PlaneSet &ps, const DevTables *dev, int adaptive, unsigned long long *fallbacks,
                              hipStream_t stream, int num_cus);
// diagnostic library (fdct8_diag.hip): the forward kernel (1, 2 or 3 = fdct8_quant_v1/v2/v3)
// a plan of `variant` runs (the product: 3 for every plan and size)
int forward_kernel_for(int variant, uint32_t nbatch, int num_cus, bool tie_heavy);
// diagnostic: the forward's data movement without arithmetic (fdct8_diag.hip): shape 3 =
// fdct8_quant_v3's (the product kernel), 2 = fdct8_quant_v2's (the queue kernel);
// grid_mult 0 = the product kernel's grid
hipError_t launch_fdct8_movement(const PlaneSet &ps, const DevTables *dev, hipStream_t stream, int num_cus, int shape,
                                 int grid_mult = 0);
hipError_t launch_roundtrip(const RoundTripSet &rt, const DevTables *dev, int adaptive, bool inv_f32,
                            unsigned long long *fallbacks, hipStream_t stream, int num_cus);
// dequantize + inverse DCT + 128 + clamp to u8 pixels in the planes of ds (decode.hip)
hipError_t launch_decode(const DecodeSet &ds, const DevTables *dev, int adaptive, bool inv_f32, hipStream_t stream,
                         int num_cus);
// run-length symbols -> u8 pixels in the planes of ss, no coefficients in memory (decode_symbols.hip)
hipError_t launch_decode_symbols(const SymbolSet &ss, const void *symbols, int symbol_bytes, const uint32_t *offsets,
                                 const DevTables *dev, int adaptive, bool inv_f32, hipStream_t stream, int num_cus);
// diagnostic: roundtrip8_f32's data movement without arithmetic (fdct8_diag.hip)
hipError_t launch_roundtrip_movement(const RoundTripSet &rt, hipStream_t stream, int num_cus);
size_t encode_workspace_bytes(long long nbatch);
// symbol_bytes 4: (uint16)value | run << 16; 2: run << 10 | (value & 0x3FF), |value| <= 511 (rle.hip)
hipError_t launch_encode(const EncodeSet &es, const DevTables *dev, int adaptive, uint32_t *offsets, void *symbols,
                         int symbol_bytes, unsigned long long capacity, void *ws, hipStream_t stream, int num_cus);
hipError_t launch_fdct8_float_pair(const PlaneArgs &p, const DevTables *dev, float *coef, hipStream_t stream,
                                   int num_cus);
hipError_t launch_idct8_pair(const DevTables *dev, int adaptive, const int16_t *coef, const int32_t *var_num,
                             long long nblk, float *recon, hipStream_t stream, int num_cus);
size_t rle_workspace_bytes(long long nblk);
size_t rle_scan_workspace_bytes(long long ntiles);
hipError_t launch_rle_scan(void *ws, long long ntiles, hipStream_t stream);
hipError_t launch_rle_fixup(uint32_t *offsets, long long nblk, const void *ws, long long ntiles, long long tile0,
                            uint32_t *total_out, hipStream_t stream);
hipError_t launch_rle_count(const int16_t *coef, long long nblk, uint32_t *offsets, void *ws, hipStream_t stream,
                            int num_cus);
hipError_t launch_rle_emit(const int16_t *coef, long long nblk, const uint32_t *offsets, void *symbols,
                           int symbol_bytes, unsigned long long capacity, hipStream_t stream, int num_cus);
// per-block Huffman size estimate (huffman.hip)
hipError_t launch_huffman_bits(const int16_t *coef, long long nblk, uint32_t *bits, hipStream_t stream, int num_cus);
hipError_t launch_huffman_from_pixels(const EncodeSet &es, const DevTables *dev, int adaptive, uint32_t *bits,
                                      hipStream_t stream, int num_cus);
// per-block squared error of the decoded u8 picture against its source, from pixels (distortion.hip)
hipError_t launch_distortion(const EncodeSet &es, const DevTables *dev, int adaptive, bool inv_f32, uint32_t *sse,
                             hipStream_t stream, int num_cus);
hipError_t launch_rle_decode(const void *symbols, int symbol_bytes, const uint32_t *offsets, long long nblk,
                             int16_t *coef, hipStream_t stream, int num_cus);
// run-length symbols -> the bit-packed stream "bits v1" (bits.hip): byte offsets (complete), then the
// bytes below `capacity`; ws: rle_workspace_bytes(nblk)
hipError_t launch_bits_pack(const void *symbols, int symbol_bytes, const uint32_t *sym_offsets, long long nblk,
                            uint32_t *offsets, uint8_t *bytes, unsigned long long capacity, void *ws,
                            hipStream_t stream, int num_cus);
// ... back to coefficients (bits.hip), and straight to u8 pixels in the planes of ss (decode_bits.hip)
hipError_t launch_bits_decode(const uint8_t *bytes, const uint32_t *offsets, long long nblk, int16_t *coef,
                              hipStream_t stream, int num_cus);
hipError_t launch_decode_bits(const SymbolSet &ss, const uint8_t *bytes, const uint32_t *offsets, const DevTables *dev,
                              int adaptive, bool inv_f32, hipStream_t stream, int num_cus);
// ... and a window of those planes: a block region and a frame range of each (decode_window.hip)
hipError_t launch_decode_bits_window(const WindowSet &ws, const uint8_t *bytes, const uint32_t *offsets,
                                     const DevTables *dev, int adaptive, bool inv_f32, hipStream_t stream,
                                     int num_cus);
// ... at 1/2, 1/4 or 1/8 size (log2_scale 1, 2, 3): n x n pixels a block, n = 8 >> log2_scale (decode_scaled.hip)
hipError_t launch_decode_bits_window_scaled(const WindowSet &ws, const uint8_t *bytes, const uint32_t *offsets,
                                            const DevTables *dev, int adaptive, int log2_scale, hipStream_t stream,
                                            int num_cus);
// a window of a packed stream as a stream of its own (extract.hip): its offsets (and gathered var_num, if
// win_var is set; ws.var is then the stored planes'), then its bytes below `capacity`; wsp:
// rle_workspace_bytes(the window's blocks)
hipError_t launch_bits_window_offsets(const WindowSet &ws, const uint32_t *offsets, uint32_t *win_offsets,
                                      int32_t *win_var, void *wsp, hipStream_t stream, int num_cus);
hipError_t launch_bits_window_gather(const WindowSet &ws, const uint8_t *bytes, const uint32_t *offsets,
                                     const uint32_t *win_offsets, uint8_t *win_bytes, unsigned long long capacity,
                                     hipStream_t stream, int num_cus);
// a window of a packed stream replaced by a patch stream's blocks (paste.hip): ws as for the extraction
// (ws.var the base's stored planes' var_num when out_var is set, patch_var then the patch's per plane),
// first[k] each stored plane's first block and first[n..kMaxPlanes] the stored blocks in all; the
// result's offsets (and var_num), then its bytes below `capacity`; wsp: rle_workspace_bytes(stored blocks)
hipError_t launch_bits_paste_offsets(const WindowSet &ws, const uint32_t *first, const uint32_t *offsets,
                                     const uint32_t *patch_offsets, const int32_t *const *patch_var,
                                     uint32_t *out_offsets, int32_t *out_var, void *wsp, hipStream_t stream,
                                     int num_cus);
hipError_t launch_bits_paste_copy(const WindowSet &ws, const uint32_t *first, const uint8_t *bytes,
                                  const uint32_t *offsets, const uint8_t *patch_bytes, const uint32_t *patch_offsets,
                                  const uint32_t *out_offsets, uint8_t *out_bytes, unsigned long long capacity,
                                  hipStream_t stream, int num_cus);
// byte offsets of a packed stream <-> one or two bytes of length per block (frame.hip); ws: rle_workspace_bytes(nblk)
hipError_t launch_block_lengths(const uint32_t *offsets, long long nblk, int length_bytes, void *lengths,
                                uint32_t *max_length, hipStream_t stream, int num_cus);
hipError_t launch_block_offsets(const void *lengths, int length_bytes, long long nblk, uint32_t *offsets, void *ws,
                                hipStream_t stream, int num_cus);
// RGB <-> Y/Cb/Cr planes (color.hip); pixel_step 1, 3 or 4
hipError_t launch_rgb_to_ycc(const ColorArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus);
hipError_t launch_ycc_to_rgb(const ColorArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus);
// the same for a picture of any size and alignment, edge-padded on the way in and cropped on the
// way out, and the edge padding of plain planes (color_pad.hip)
hipError_t launch_rgb_to_ycc_pad(const ColorPadArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus);
hipError_t launch_ycc_to_rgb_crop(const ColorPadArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus);
hipError_t launch_pad_planes(const PadSet &s, hipStream_t stream, int num_cus);
// diagnostic library (fdct8_diag.hip): the lane-per-block fp64 kernels (variant 1)
hipError_t launch_fdct8_float(const PlaneArgs &p, const DevTables *dev, float *coef, hipStream_t stream);
hipError_t launch_idct8(const DevTables *dev, int adaptive, const int16_t *coef, const int32_t *var_num,
                        long long nblk, float *recon, hipStream_t stream);
hipError_t launch_synth(uint64_t seed, int kind, uint8_t *dst, long long stride, long long frame_stride,
                        int width, int height, int nframes, hipStream_t stream);

}  // namespace dctq
