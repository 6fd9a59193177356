// dct_amd/csrc/decode_bits.hip -- dctq_decode_bits_planes: the bit-packed stream "bits v1"
// -> u8 pixels, for every block of up to 4 planes in ONE launch and with no coefficient in
// memory.  Bit for bit dctq_bits_decode followed by dctq_decode_planes, because it is both
// kernels' code: the half tile is rebuilt by bits_to_coef's bit walk (bits_rebuild_half,
// bits_core.h), and its rows go through decode8's inverse and pixel sink (inverse_core.h,
// decode_core.h) -- the structure of symbols_to_pixels (decode_symbols.hip), with the packed
// bytes in the symbols' place.
//
// P + 4 B in + 64 B out per block (P = the block's packed bytes; + 4 B of var_num, adaptive
// plans) against P + 4 + 128 + 128 + 64 B of the two launches.
//
// One wave per 64-block tile of the concatenated block numbering, two 32-block halves; a
// block's plane, its number inside the plane and its var_num are per lane, the store
// descriptor per plane and wave-uniform, as in symbols_to_pixels.
//
// Store-data hazard: the half's pixel stores are retired by the vmcnt(0)
// that bits_rebuild_half issues in every chunk before its first LDS access; no store and no
// load is issued between that and the read-out of the rows.
#include "bits_core.h"
#include "decode_core.h"
#include "zigzag.h"

namespace dctq {

constexpr int kBitsPixGridMult = 64;  // as symbols_to_pixels: about one tile per wave

// Plane of block b < blk_first[kMaxPlanes] of the concatenated numbering, and a plane's
// first block (select chains: k may differ by lane); as decode_symbols.hip's.
__device__ __forceinline__ int bits_plane_of_block(const SymbolSet &ss, uint32_t b) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) k += b >= ss.blk_first[i] ? 1 : 0;
    return k;
}
__device__ __forceinline__ uint32_t bits_block_first_of(const SymbolSet &ss, int k) {
    uint32_t f = 0u;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) f = k == i ? ss.blk_first[i] : f;
    return f;
}

template <bool ADAPTIVE, bool INV32>
__global__ __launch_bounds__(kThreadsP, 4) void bits_to_pixels(SymbolSet ss, const uint8_t *__restrict__ bytes,
                                                               const uint32_t *__restrict__ offsets,
                                                               const DevTables *__restrict__ dev) {
    __shared__ u4r wave_lds[kWavesP][kBitsLds / 16];
    __shared__ uint8_t zz[64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 64) zz[threadIdx.x] = kZigzag[threadIdx.x];
    __syncthreads();
    const int hh = lane >> 5, j = lane & 31;
    const uint32_t nblk = ss.blk_first[kMaxPlanes], ntiles = (nblk + 63u) >> 6;
    const uint32_t step = gridDim.x * kWavesP;
    char *lt = reinterpret_cast<char *>(wave_lds[wv]);
    uint8_t *lst = reinterpret_cast<uint8_t *>(lt + kHalf * kDecPitch);
    for (uint32_t t = blockIdx.x * kWavesP + wv; t < ntiles; t += step) {
        const uint32_t b0 = t * 64u;
        const int nb = nblk - b0 < 64u ? (int)(nblk - b0) : 64;
        const uint32_t offv = offsets[b0 + (uint32_t)(lane < nb ? lane : nb)];  // lanes >= nb: the end of the tile
        const uint32_t oend = offsets[b0 + (uint32_t)nb];
        for (int h = 0; h < nb; h += kHalf) {
            const int he = nb < h + kHalf ? nb : h + kHalf;
            // lane (hh, j): block h + j of the tile; past the half's end, its last block (computed, not stored)
            const uint32_t last = b0 + (uint32_t)he - 1u;
            const bool valid = h + j < he;
            const uint32_t gb = valid ? b0 + (uint32_t)(h + j) : last;
            const int kl = bits_plane_of_block(ss, gb);
            const uint32_t n = gb - bits_block_first_of(ss, kl);
            int32_t vn = 0;
            if (ADAPTIVE) vn = __builtin_nontemporal_load(var_of(ss, (uint32_t)kl) + n);

            bits_rebuild_half(bytes, offv, oend, h, he, lane, lt, lst, zz);
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

            // the planes present in the half, one descriptor each
            const int k_lo = __builtin_amdgcn_readfirstlane(bits_plane_of_block(ss, b0 + (uint32_t)h));
            const int k_hi = __builtin_amdgcn_readfirstlane(bits_plane_of_block(ss, last));
            for (int k = k_lo; k <= k_hi; ++k) store_pixel_rows(ss.pl[k], n, valid && kl == k, hh, pix);
        }
    }
}

hipError_t launch_decode_bits(const SymbolSet &ss, const uint8_t *bytes, const uint32_t *offsets, const DevTables *dev,
                              int adaptive, bool inv_f32, hipStream_t stream, int num_cus) {
    const uint64_t ntiles = ((uint64_t)ss.blk_first[kMaxPlanes] + 63) / 64;
    return with_bools(
        [&](auto a, auto f32) {
            if constexpr (a && f32) {
                return hipErrorInvalidValue;  // never dispatched: the fp32 inverse is the non-adaptive plans'
            } else {
                return launch_persistent<bits_to_pixels<a, f32>, kThreadsP, kWavesP, kBitsPixGridMult>(
                    ntiles, num_cus, stream, ss, bytes, offsets, dev);
            }
        },
        adaptive != 0, inv_f32 && !adaptive);
}

}  // namespace dctq
