// dct_amd/csrc/frame.hip -- dctq_block_lengths and dctq_block_offsets: the byte offsets of a
// "bits v1" stream as one or two bytes per block, and back (the container "frame v1",
// include/dct_amd.h).
//
//   dctq_block_lengths: lane i owns output dword i -- four u8 or two u16 lengths -- so no two
//                       lanes store into one dword.  Its 5 (3) offsets come in as one 16-B
//                       (8-B) load and one dword load, consecutive lanes at consecutive
//                       addresses.  The dword that holds the last, partial group of lengths is
//                       written by its lane as single lengths, so nothing past the last length
//                       is touched.  The largest unsaturated difference is kept per lane over
//                       the grid-stride loop, reduced per wave and per workgroup, and leaves
//                       as one atomic max per workgroup into a word zeroed on the stream.
//   dctq_block_offsets: one wave per 64-block tile: lane b reads length b, clamps it to the
//                       format's 368, the wave scan gives the tile-local offsets and the tile
//                       total; then the tile scan and fix-up of rle.hip, as bits.hip uses them.
#include "rle_decode_core.h"
#include "scan_core.h"

namespace dctq {

constexpr int kFrameWaves = 4;
constexpr int kFrameThreads = 64 * kFrameWaves;
constexpr int kOffsetsGridMult = 64;    // as the bits kernels: about one tile per wave on large inputs
constexpr int kLengthsGridMult = 1;     // the resident workgroups only: one atomic per workgroup
constexpr uint32_t kMaxBlockBytes = 368;  // bits v1: 64 symbols of 46 bits

// P consecutive dwords at a 4-byte aligned address: one global load of 4 P bytes
template <int P>
struct __attribute__((aligned(4))) Dwords {
    uint32_t v[P];
};

// ---- lengths: W = length_bytes; P = 4 / W lengths per lane and output dword
template <int W>
__global__ __launch_bounds__(kFrameThreads) void block_lengths_kernel(const uint32_t *__restrict__ offsets,
                                                                     long long nblk, void *__restrict__ lengths,
                                                                     uint32_t *__restrict__ max_length,
                                                                     long long ngroups) {
    constexpr int P = 4 / W;
    constexpr uint32_t kSat = W == 1 ? 0xFFu : 0xFFFFu;
    __shared__ uint32_t wmax[kFrameWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * kFrameThreads;
    uint32_t mx = 0;
    for (long long g = (long long)blockIdx.x * kFrameThreads + threadIdx.x; g < ngroups; g += stride) {
        const long long b0 = g * P;
        if (b0 + P <= nblk) {  // offsets[b0 .. b0 + P] exist
            const Dwords<P> q = *reinterpret_cast<const Dwords<P> *>(offsets + b0);
            const uint32_t last = offsets[b0 + P];
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const uint32_t d = (k + 1 < P ? q.v[k + 1] : last) - q.v[k];
                mx = d > mx ? d : mx;
                word |= (d < kSat ? d : kSat) << (8 * W * k);
            }
            reinterpret_cast<uint32_t *>(lengths)[g] = word;
        } else {  // the last group: nblk - b0 < P lengths, one store each
            for (long long b = b0; b < nblk; ++b) {
                const uint32_t d = offsets[b + 1] - offsets[b];
                mx = d > mx ? d : mx;
                const uint32_t s = d < kSat ? d : kSat;
                if constexpr (W == 1) reinterpret_cast<uint8_t *>(lengths)[b] = (uint8_t)s;
                else reinterpret_cast<uint16_t *>(lengths)[b] = (uint16_t)s;
            }
        }
    }
#pragma unroll
    for (int sh = 32; sh; sh >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)mx, sh);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kFrameWaves; ++w) mx = wmax[w] > mx ? wmax[w] : mx;
        if (mx) atomicMax(max_length, mx);
    }
}

// ---- offsets: offsets[b] = clamped lengths of the tile's blocks before b; tiles[t] = the tile's bytes
template <int W>
__global__ __launch_bounds__(kFrameThreads) void block_offsets_kernel(const void *__restrict__ lengths, long long nblk,
                                                                     uint32_t *__restrict__ offsets,
                                                                     uint32_t *__restrict__ tiles, long long ntiles) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * kFrameWaves;
    for (long long t = (long long)blockIdx.x * kFrameWaves + wv; t < ntiles; t += stride) {
        const long long b0 = t * 64;
        const int nb = tile_blocks(t, nblk);
        uint32_t len = 0;
        if (lane < nb) {
            if constexpr (W == 1) len = reinterpret_cast<const uint8_t *>(lengths)[b0 + lane];
            else len = reinterpret_cast<const uint16_t *>(lengths)[b0 + lane];
        }
        len = len < kMaxBlockBytes ? len : kMaxBlockBytes;
        const uint32_t inc = wave_inclusive_scan(len);
        if (lane < nb) offsets[b0 + lane] = inc - len;
        if (lane == 63) tiles[t] = inc;
    }
}

hipError_t launch_block_lengths(const uint32_t *offsets, long long nblk, int length_bytes, void *lengths,
                                uint32_t *max_length, hipStream_t stream, int num_cus) {
    hipError_t e = hipMemsetAsync(max_length, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const int per = 4 / length_bytes;
    const long long ngroups = (nblk + per - 1) / per;
    return with_bools(
        [&](auto w2) {
            return launch_persistent<block_lengths_kernel<(decltype(w2)::value ? 2 : 1)>, kFrameThreads, kFrameWaves,
                                     kLengthsGridMult>((uint64_t)((ngroups + 63) / 64), num_cus, stream, offsets, nblk,
                                                       lengths, max_length, ngroups);
        },
        length_bytes == 2);
}

hipError_t launch_block_offsets(const void *lengths, int length_bytes, long long nblk, uint32_t *offsets, void *ws,
                                hipStream_t stream, int num_cus) {
    const long long ntiles = (nblk + 63) / 64;
    hipError_t e = with_bools(
        [&](auto w2) {
            return launch_persistent<block_offsets_kernel<(decltype(w2)::value ? 2 : 1)>, kFrameThreads, kFrameWaves,
                                     kOffsetsGridMult>((uint64_t)ntiles, num_cus, stream, lengths, nblk, offsets,
                                                       (uint32_t *)ws, ntiles);
        },
        length_bytes == 2);
    if (e != hipSuccess) return e;
    if ((e = launch_rle_scan(ws, ntiles, stream)) != hipSuccess) return e;
    return launch_rle_fixup(offsets, nblk, ws, ntiles, 0, offsets + nblk, stream);
}

}  // namespace dctq
