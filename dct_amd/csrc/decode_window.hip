// dct_amd/csrc/decode_window.hip -- dctq_decode_bits_window_planes: a block region and a frame
// range of up to 4 planes of a "bits v1" stream -> u8 pixels in ONE launch, reading only the
// blocks inside the windows.  bits_to_pixels (decode_bits.hip) with another answer to "which
// blocks does a wave take, and where do their pixels land": the source is the same bit walk
// (bits_rebuild_half, bits_core.h), the sink the same inverse and pixel stores
// (inverse_half_*_rows, store_pixel_rows), and the loop below is decode_tiles
// (tile_decode_core.h) over RUNS instead of 64-block tiles.
//
// A run (tools/window_ref.py states the mapping in plain Python): up to 64 consecutive stored
// blocks of one block row of one frame of one plane, inside that plane's window.  A window wb
// blocks wide has ceil(wb / 64) runs per block row; runs are numbered over window rows, then
// frames, then planes, and never straddle any of them.  Consecutive stored blocks are
// contiguous in the payload, so a run is to the bit source what a tile is: lanes hold
// offsets[s0 + min(lane, nb)], oend = offsets[s0 + nb], and nothing outside [offsets[s0], oend)
// is read.  A window narrower than 64 blocks leaves lanes idle; rows are not packed into one
// wave, which would break that contiguity.
//
// The store-data hazard rule at the top of tile_decode_core.h holds unchanged: every chunk of
// bits_rebuild_half waits (vmcnt(0)) before its first LDS access, and nothing here issues a
// store or a load between that wait and the read-out of the rows.
#include "bits_core.h"
#include "decode_core.h"
#include "pair_core.h"
#include "zigzag.h"

namespace dctq {

constexpr int kWindowGridMult = 64;  // as bits_to_pixels: about one run per wave

// Plane of run r (wave-uniform; a select chain over prefixes that stay in SGPRs).
__device__ __forceinline__ int plane_of_run(const WindowSet &ws, uint32_t r) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) k += r >= ws.run_first[i] ? 1 : 0;
    return k;
}

// pixel_rows_out (decode_core.h) for blocks [h, he) of a run, which lies in ONE plane: block i
// of the run is block var0 + i of its stored plane (var_num) and block d0 + i of the window's
// own picture p (the destination); `rebuild` leaves the half's rows in lt at pitch kDecPitch.
template <bool ADAPTIVE, bool INV32, typename R>
__device__ __forceinline__ void window_rows_out(const PlaneArgs &p, const int32_t *__restrict__ var, uint32_t var0,
                                                uint32_t d0, const DevTables *__restrict__ dev, int h, int he,
                                                int lane, const char *lt, R &&rebuild) {
    const int hh = lane >> 5, j = lane & 31;
    // (a) lane (hh, j): block h + j of the run; past the half's end, its last block (computed,
    // not stored).  var_num is asked for ahead of the rebuild, which hides its latency
    const bool valid = h + j < he;
    const uint32_t i = (uint32_t)(valid ? h + j : he - 1);
    int32_t vn = 0;
    if (ADAPTIVE) vn = __builtin_nontemporal_load(var + (var0 + i));

    rebuild();
    // (b) rows 4hh..4hh+3 of block j
    uint4 cur[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u4r v = *reinterpret_cast<const u4r *>(lt + j * kDecPitch + 16 * (4 * hh + r));
        cur[r] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    wave_sync_lds();  // every lane's rows are in registers before the next half zeroes the tile

    // the whole wave runs the arithmetic (exec-masked scales and lane-half swaps inside)
    u2p pix[4];
    const auto pack = [&pix](int r, int c, const float (&o)[4]) { pix[r][c >> 2] = pack_u8x4(o[0], o[1], o[2], o[3]); };
    if constexpr (INV32) inverse_half_f32_rows(dev, cur, hh, pack);
    else inverse_half_rows<ADAPTIVE>(dev, cur, vn, hh, pack);

    store_pixel_rows(p, d0 + i, valid, hh, pix);
}

template <bool ADAPTIVE, bool INV32>
__global__ __launch_bounds__(kThreadsP, 4) void bits_window_to_pixels(WindowSet ws, const uint8_t *__restrict__ bytes,
                                                                      const uint32_t *__restrict__ offsets,
                                                                      const DevTables *__restrict__ dev) {
    __shared__ u4r wave_lds[kWavesP][kBitsLds / 16];
    __shared__ uint8_t zz[64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 64) zz[threadIdx.x] = kZigzag[threadIdx.x];
    __syncthreads();
    const uint32_t nruns = ws.run_first[kMaxPlanes];
    const uint32_t stride = gridDim.x * kWavesP;
    char *lt = reinterpret_cast<char *>(wave_lds[wv]);
    for (uint32_t t = blockIdx.x * kWavesP + wv; t < nruns; t += stride) {
        // run t -> plane k, window row q (over the window's frames), run j of that row
        const int k = plane_of_run(ws, t);
        uint32_t rf = 0u;
#pragma unroll
        for (int i = 1; i < kMaxPlanes; ++i) rf = k == i ? ws.run_first[i] : rf;
        const PlaneArgs &p = ws.pl[k];
        const WindowPlane &w = ws.win[k];
        const uint32_t rp = t - rf;
        const uint32_t q = fdiv(rp, w.div_runs), j = rp - q * w.runs_row;
        const uint32_t f = fdiv(q, w.div_rows), y = q - f * w.rows;
        // the run's first block: behind the window's first by f frames, y rows and 64 j blocks
        // of the STORED plane; in the window's own picture it is block q * bw + 64 j
        const uint32_t rel = f * w.nblk_frame + y * w.bw + 64u * j;
        const uint32_t s0 = w.first + rel, d0 = q * (uint32_t)p.bw + 64u * j;
        const uint32_t left = (uint32_t)p.bw - 64u * j;
        const int nb = left < 64u ? (int)left : 64;
        const uint32_t offv = offsets[s0 + (uint32_t)(lane < nb ? lane : nb)];  // lanes >= nb: the end of the run
        const uint32_t oend = offsets[s0 + (uint32_t)nb];
        for (int h = 0; h < nb; h += kHalf) {
            const int he = nb < h + kHalf ? nb : h + kHalf;
            window_rows_out<ADAPTIVE, INV32>(p, var_of(ws, (uint32_t)k), w.var_first + rel, d0, dev, h, he, lane, lt,
                                             [=]() __attribute__((always_inline)) {
                                                 return bits_rebuild_half(bytes, offv, oend, 0u, h, he, lane, lt, &zz);
                                             });
        }
    }
}

hipError_t launch_decode_bits_window(const WindowSet &ws, const uint8_t *bytes, const uint32_t *offsets,
                                     const DevTables *dev, int adaptive, bool inv_f32, hipStream_t stream,
                                     int num_cus) {
    return with_inverse(
        [&](auto a, auto f32) {
            return launch_persistent<bits_window_to_pixels<a, f32>, kThreadsP, kWavesP, kWindowGridMult>(
                ws.run_first[kMaxPlanes], num_cus, stream, ws, bytes, offsets, dev);
        },
        adaptive != 0, inv_f32);
}

}  // namespace dctq
