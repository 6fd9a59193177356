// dct_amd/csrc/tile_decode_core.h -- the wave-per-tile loop of the four stream decoders
// (rle_decode_kernel, bits_to_coef, symbols_to_pixels, bits_to_pixels) and the
// coefficient sink of the first two.  The pixel sink of the other two is decode_core.h's
// (it needs the inverse; this header does not).
#pragma once
#include "rle_decode_core.h"
#include "zigzag.h"

namespace dctq {

// One wave per 64-block tile of a stream whose block b starts at offsets[b] (nblk + 1
// entries), grid-stride over `ntiles` tiles, each tile as two 32-block halves.  Per half
//     sink(b0, h, he, lane, lt, rebuild)
// runs once: blocks [b0 + h, b0 + he) of the stream; lt: the wave's LDS (LDS_BYTES).
// The sink calls rebuild() where it wants the half's natural-order int16 rows in lt;
// rebuild() is
//     source(offv, oend, cnt_lane, h, he, lane, lt, zz)
// and returns the rows' pitch.  offv / oend as off_at (rle_decode_core.h); cnt_lane: lane
// b holds block b's length (the bit sources do not use it, and it folds away there); zz:
// points to the zigzag order in LDS.  I is the block index type: long long for a plain coefficient
// array, uint32_t where the blocks are bounded below 2^26 (SymbolSet).
//
// Store-data hazard, stated here for all four kernels: the sink's stores of
// one half may still be reading their data VGPRs when the next half starts, so every LDS
// read into registers follows a vmcnt(0) that retired them.  The sources issue it: each
// path of rebuild_half and every chunk of bits_rebuild_half waits before its first LDS
// access, rebuild_half's callers wait once more (the walk's last clipped loads) before the
// read-out, and neither source nor sink issues a store or a load between the last wait and
// the read-out of the rows.
template <typename I, int WAVES, int LDS_BYTES, typename Source, typename Sink>
__device__ __forceinline__ void decode_tiles(const uint32_t *__restrict__ offsets, I nblk, I ntiles, Source &&source,
                                             Sink &&sink) {
    __shared__ u4r wave_lds[WAVES][LDS_BYTES / 16];
    __shared__ uint8_t zz[64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 64) zz[threadIdx.x] = kZigzag[threadIdx.x];
    __syncthreads();
    const I stride = (I)gridDim.x * WAVES;
    char *lt = reinterpret_cast<char *>(wave_lds[wv]);
    for (I t = (I)blockIdx.x * WAVES + wv; t < ntiles; t += stride) {
        const I b0 = t * 64;
        // spelled out for 32-bit block numbers: the compiler simplifies an always-inline function on
        // its own before it inlines it, and behind a call 0 <= nb <= 64 is not known when the
        // min and compare forms below are chosen (signed ones came out; the parent's are unsigned)
        int nb;
        if constexpr (sizeof(I) == 4) nb = nblk - b0 < 64u ? (int)(nblk - b0) : 64;
        else nb = tile_blocks(t, nblk);
        const uint32_t offv = offsets[b0 + (I)(lane < nb ? lane : nb)];  // lanes >= nb: the end of the tile
        const uint32_t oend = offsets[b0 + (I)nb];
        // per-lane block length (lane b: block b of the tile)
        const uint32_t nxt_off = (uint32_t)__shfl_down((int)offv, 1);
        const uint32_t cnt_lane = (lane == 63 ? oend : nxt_off) - offv;
        for (int h = 0; h < nb; h += kHalf) {
            const int he = nb < h + kHalf ? nb : h + kHalf;
            sink(b0, h, he, lane, lt, [=]() __attribute__((always_inline)) {
                return source(offv, oend, cnt_lane, h, he, lane, lt, &zz);
            });
        }
    }
}

// The run-length source: symbols of W bytes (LANE_PITCH: the lane path's row pitch), with the
// two waits rebuild_half leaves to its caller.  (The bit source is bits_rebuild_half itself.)
template <int W, int LANE_PITCH>
__device__ __forceinline__ int symbols_source(const void *__restrict__ symbols, uint32_t offv, uint32_t oend,
                                              uint32_t cnt_lane, int h, int he, int lane, char *lt,
                                              const uint8_t (*zz)[64]) {
    uint32_t *lsym = reinterpret_cast<uint32_t *>(lt + kHalf * LANE_PITCH);
    const bool lane_path = rebuild_half<W, LANE_PITCH>(symbols, offv, oend, cnt_lane, h, he, lane, lt, lsym, *zz);
    wave_sync_lds();
    retire_stores();  // vmcnt(0): the walk's last (clipped) loads before the read-out
    return lane_path ? LANE_PITCH : kDecPitch;
}

// The coefficient sink: the half's rows as 1 KiB stores (8 lane-addresses per block); chunk
// 64k + lane = 16 B of row 8k + lane/8.  SYNC_AFTER: a wave barrier between the read-out and
// the stores (bits_to_coef: every lane's rows are in registers before the next half zeroes
// the tile; rle_decode_kernel never had one).
template <bool SYNC_AFTER, typename R>
__device__ __forceinline__ void coef_rows_out(int16_t *__restrict__ coef, long long b0, int h, int he, int lane,
                                              const char *lt, R &&rebuild) {
    const int pitch = rebuild();
    u4r val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        val[k] = *reinterpret_cast<const u4r *>(lt + (8 * k + (lane >> 3)) * pitch + 16 * (lane & 7));
    if constexpr (SYNC_AFTER) wave_sync_lds();
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(coef + (b0 + h) * 64, (short)0, (he - h) * 128, kRsrcFlags);
#pragma unroll
    for (int k = 0; k < 4; ++k) __builtin_amdgcn_raw_buffer_store_b128(val[k], rs, lane * 16, k * 1024, kNtAux);
}

}  // namespace dctq
