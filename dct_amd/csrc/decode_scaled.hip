// dct_amd/csrc/decode_scaled.hip -- dctq_decode_bits_window_scaled_planes: a window of up to 4
// planes of a "bits v1" stream -> u8 pixels at 1/2, 1/4 or 1/8 size in ONE launch (scale s,
// n = 8 / s: every stored 8 x 8 block gives n x n pixels).  bits_window_to_pixels
// (decode_window.hip) with a new sink: the same runs (for_window_runs, window_core.h) and the
// same bit source (bits_rebuild_half, bits_core.h), whose walk stops once it is past the last
// zigzag position of the block's n x n corner (24, 4, 0); the sink reads that corner of each
// rebuilt row set from LDS and applies the definition of include/dct_amd.h (stated in plain
// numpy in tools/scaled_ref.py) in fp64, every multiply and add rounded on its own
// (-ffp-contract=off) and every sum in ascending index.
//
// Lanes.  Lane (hh, j) = (lane / 32, lane % 32) takes block h + j of the half.  n = 4: its pixel
// rows 2 hh and 2 hh + 1, one dword each; n = 2: row hh, two bytes; n = 1: lanes hh = 0, one
// byte.  The blocks of a run are neighbours in one block row, so the 32 lanes of a half-wave
// write 32 n consecutive bytes of an image row.
//
// The store-data hazard rule at the top of tile_decode_core.h holds unchanged: every chunk of
// bits_rebuild_half waits (vmcnt(0)) before its first LDS access, and nothing here issues a
// store or a load between that wait and the read-out of the corner.
#include "bits_core.h"
#include "pair_core.h"
#include "window_core.h"
#include "zigzag.h"

namespace dctq {

constexpr int kScaledGridMult = 64;  // as bits_window_to_pixels: about one run per wave

// Dn[u][i], the n-point DCT matrix of the definition, as the header's literals (never through cos)
template <int N>
__device__ constexpr double dct_n(int u, int i) {
    constexpr double r = 0x1.6a09e667f3bcdp-1;
    constexpr double h = 0.5, a = 0x1.4e7ae9144f0fcp-1, b = 0x1.1517a7bdb3896p-2;
    if (N == 1) return 1.0;
    if (N == 2) return u == 1 && i == 1 ? -r : r;
    const double d4[4][4] = {{h, h, h, h}, {a, b, -b, -a}, {h, -h, -h, h}, {b, -a, a, -b}};
    return d4[u & 3][i & 3];
}
// the walk's end: one past the last zigzag position of the n x n corner
template <int N>
constexpr uint32_t corner_end() {
    return N == 4 ? 25u : N == 2 ? 5u : 1u;
}
static_assert(corner_end<4>() == 25u && corner_end<2>() == 5u && corner_end<1>() == 1u, "zigzag.h: 27 -> 24, 9 -> 4, 0 -> 0");

// The sink for blocks [h, he) of a run, which lies in ONE block row of one frame of one plane:
// block i of the run is block var0 + i of its stored plane (var_num) and sits in block column
// c0 + i of block row y of frame f of the reduced picture p; `rebuild` leaves the half's rows
// in lt at pitch kDecPitch, of which the first N values of the first N rows are read.
template <bool ADAPTIVE, int N, typename R>
__device__ __forceinline__ void scaled_rows_out(const PlaneArgs &p, const int32_t *__restrict__ var, uint32_t var0,
                                                uint32_t f, uint32_t y, uint32_t c0, const DevTables *__restrict__ dev,
                                                int h, int he, int lane, const char *lt, R &&rebuild) {
    constexpr int RPL = N >= 2 ? N / 2 : 1;  // pixel rows of its block a lane computes
    const int hh = lane >> 5, j = lane & 31;
    // (a) past the half's end: its last block (computed, not stored).  var_num is asked for
    // ahead of the rebuild, which hides its latency
    const bool inside = h + j < he;
    const bool valid = inside && (N > 1 || hh == 0);
    const uint32_t i = (uint32_t)(inside ? h + j : he - 1);
    int32_t vn = 0;
    if (ADAPTIVE) vn = __builtin_nontemporal_load(var + (var0 + i));

    rebuild();
    // (b) the corner of block j: values 0..N-1 of rows 0..N-1
    uint32_t cw[N][(N + 1) / 2];
#pragma unroll
    for (int u = 0; u < N; ++u)
#pragma unroll
        for (int v = 0; v < (N + 1) / 2; ++v)
            cw[u][v] = *reinterpret_cast<const uint32_t *>(lt + j * kDecPitch + 16 * u + 4 * v);
    wave_sync_lds();  // every lane's corner is in registers before the next half zeroes the tile

    //   non-adaptive: q * (1/Q)                     (src/quantization.c:139,144)
    //   adaptive:     (q * Q) * (2 - nv), DC: q * Q (:137,144,193,198-199)
    ConstTables *tp = tables(dev);
    double sc = 1.0;
    if (ADAPTIVE) {
        const double vr = (double)vn / 4096.0;
        sc = 2.0 - fmin(1.0, fmax(0.1, vr / 1000.0));
    }
    double x[N][N];
#pragma unroll
    for (int u = 0; u < N; ++u)
#pragma unroll
        for (int v = 0; v < N; ++v) {
            const uint32_t wd = cw[u][v >> 1];
            const double q = (v & 1) ? (double)((int)wd >> 16) : (double)(int)(int16_t)(wd & 0xFFFFu);
            if (ADAPTIVE) {
                const double t = q * tp->quant[8 * u + v];
                x[u][v] = (u | v) ? t * sc : t;
            } else {
                x[u][v] = q * tp->dequant[8 * u + v];
            }
        }
    // temp[u][c] = sum over v of x[u][v] * Dn[v][c]
    double temp[N][N];
#pragma unroll
    for (int u = 0; u < N; ++u)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            double s = x[u][0] * dct_n<N>(0, c);
#pragma unroll
            for (int v = 1; v < N; ++v) s = s + x[u][v] * dct_n<N>(v, c);
            temp[u][c] = s;
        }
    // out[r][c] = sum over u of Dn[u][r] * temp[u][c] for the lane's rows r = RPL hh + k, then
    // * n / 8, + 128, clamp, round to nearest even: byte c of the row's word
    uint32_t word[RPL];
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
        double d[N];
#pragma unroll
        for (int u = 0; u < N; ++u) d[u] = N > 1 && hh ? dct_n<N>(u, (RPL + k) % N) : dct_n<N>(u, k);
        word[k] = 0u;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            double s = d[0] * temp[0][c];
#pragma unroll
            for (int u = 1; u < N; ++u) s = s + d[u] * temp[u][c];
            const double r = s * (N / 8.0) + 128.0;
            word[k] |= (uint32_t)__builtin_rint(fmin(fmax(r, 0.0), 255.0)) << (8 * c);
        }
    }

    // (c) N bytes a row at byte column (c0 + i) N of image row y N + RPL hh + k of frame f:
    // through a descriptor over the plane, so an address that went wrong drops the write, or
    // with 64-bit addresses for a plane of 4 GiB or more (span == 0)
    uint8_t *base = const_cast<uint8_t *>(p.src);
    const uint32_t row0 = y * (uint32_t)N + (uint32_t)(RPL * hh), col = (c0 + i) * (uint32_t)N;
    if (p.span) {  // kernel argument: wave-uniform.  Every offset inside the plane is < 2^32
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)p.span, kRsrcFlags);
        const uint32_t st = (uint32_t)p.stride;
        const uint32_t off = f * (uint32_t)p.frame_stride + row0 * st + col;
        if (valid) {
#pragma unroll
            for (int k = 0; k < RPL; ++k) {
                if constexpr (N == 4) __builtin_amdgcn_raw_buffer_store_b32(word[k], rs, off + k * st, 0, kNtAux);
                else if constexpr (N == 2) __builtin_amdgcn_raw_buffer_store_b16((uint16_t)word[k], rs, off + k * st, 0, kNtAux);
                else __builtin_amdgcn_raw_buffer_store_b8((uint8_t)word[k], rs, off + k * st, 0, kNtAux);
            }
        }
    } else if (valid) {  // a plane of 4 GiB or more: 64-bit addresses
        uint8_t *px = base + (long long)f * p.frame_stride + (long long)row0 * p.stride + (long long)col;
#pragma unroll
        for (int k = 0; k < RPL; ++k) {
            uint8_t *at = px + k * p.stride;
            if constexpr (N == 4) __builtin_nontemporal_store(word[k], reinterpret_cast<uint32_t *>(at));
            else if constexpr (N == 2) __builtin_nontemporal_store((uint16_t)word[k], reinterpret_cast<uint16_t *>(at));
            else __builtin_nontemporal_store((uint8_t)word[k], at);
        }
    }
}

template <bool ADAPTIVE, int LOG2S>
__global__ __launch_bounds__(kThreadsP, 4) void bits_window_to_scaled_pixels(WindowSet ws,
                                                                             const uint8_t *__restrict__ bytes,
                                                                             const uint32_t *__restrict__ offsets,
                                                                             const DevTables *__restrict__ dev) {
    constexpr int N = 8 >> LOG2S;
    static_assert(N == 4 || N == 2 || N == 1, "scale 2, 4 or 8");
    __shared__ u4r wave_lds[kWavesP][kBitsLds / 16];
    __shared__ uint8_t zz[64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 64) zz[threadIdx.x] = kZigzag[threadIdx.x];
    __syncthreads();
    char *lt = reinterpret_cast<char *>(wave_lds[wv]);
    for_window_runs<kWavesP>(ws, offsets, lane, wv,
                             [&](int k, uint32_t, uint32_t f, uint32_t y, uint32_t j, uint32_t rel, int nb, uint32_t offv,
                                 uint32_t oend) __attribute__((always_inline)) {
        for (int h = 0; h < nb; h += kHalf) {
            const int he = nb < h + kHalf ? nb : h + kHalf;
            scaled_rows_out<ADAPTIVE, N>(ws.pl[k], var_of(ws, (uint32_t)k), ws.win[k].var_first + rel, f, y, 64u * j, dev,
                                         h, he, lane, lt, [=]() __attribute__((always_inline)) {
                                             return bits_rebuild_half<corner_end<N>()>(bytes, offv, oend, 0u, h, he, lane,
                                                                                       lt, &zz);
                                         });
        }
    });
}

hipError_t launch_decode_bits_window_scaled(const WindowSet &ws, const uint8_t *bytes, const uint32_t *offsets,
                                            const DevTables *dev, int adaptive, int log2_scale, hipStream_t stream,
                                            int num_cus) {
    return with_bools(
        [&](auto a) {
            const auto go = [&](auto l) {
                return launch_persistent<bits_window_to_scaled_pixels<a, l>, kThreadsP, kWavesP, kScaledGridMult>(
                    ws.run_first[kMaxPlanes], num_cus, stream, ws, bytes, offsets, dev);
            };
            return log2_scale == 1   ? go(std::integral_constant<int, 1>())
                   : log2_scale == 2 ? go(std::integral_constant<int, 2>())
                                     : go(std::integral_constant<int, 3>());
        },
        adaptive != 0);
}

}  // namespace dctq
