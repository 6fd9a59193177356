// dct_amd/csrc/decode.hip -- dctq_decode_planes: quantized coefficients -> u8 pixels,
// for every block of up to 4 planes in ONE launch,
//   pix = (uint8) rne(min(max(r, 0), 255)),  r = fp32(dct_inverse(dequantize(coef)) + 128)
// with r exactly the value the fused round trip stores as recon for the same plan
// (inverse_core.h: inverse_half_f32 for plans the fp32 bound admits, the fp64
// inverse_half<ADAPTIVE> rounded once to fp32 otherwise), i.e. the last arrow of the
// reference's pipeline tests/test_entropy.c:350-393 (dequantize, dct_inverse, clamp).
// The fp32 inverse's 5e-5 holds for every block of u8 pixels (coefficients inside the
// plan's forward range); the coefficients here are the caller's, and outside that range
// its bound grows linearly with the block's magnitudes (include/dct_amd.h,
// tools/inv_bound.py block_error; tests/test_decode_foreign_gpu.py).
//
// 128 B in + 64 B out per block (+ 4 B of var_num, adaptive plans) against the 384 B
// of dctq_inverse, whose fp32 block-major recon a host then has to clamp and un-tile.
//
// Paired-lane layout of idct8_pair (f64_pair.hip): one wave, one 32-block batch, lane
// (h, j) = rows 4h..4h+3 of block j.  Persistent grid-stride loop over the global
// batch numbering of all planes; the next batch's four 16 B coefficient rows (and
// var_num) are prefetched into registers with non-temporal loads.  The lane's four
// rows are clamped, rounded and packed to 8 B each in registers and stored straight
// to their image position: lanes j, j+1, ... of one block row are contiguous, so a
// wave writes runs of up to 256 B per image row.  No LDS, so the store-data hazard
// of DESIGN.md does not arise.  The stores are non-temporal and go through a buffer
// descriptor over the plane (PlaneArgs::span bytes from its first pixel): an address
// that went wrong drops the write instead of faulting, as load_rows<true> does for
// reads.  Lanes past the plane's last block store nothing.
#include "decode_core.h"

namespace dctq {

// The grid (launch_persistent): up to 64 x the resident workgroups, as the paired kernels of f64_pair.hip.
constexpr int kDecodeGridMult = 64;

// Coefficient rows 4h..4h+3 (16 B each) of block j of global batch g, and its variance
// numerator; read once, so non-temporal.  Past the plane's end (and past the last
// batch, for the final prefetch): block 0 of the last plane.
template <bool ADAPTIVE>
__device__ __forceinline__ void prefetch_coefs(const DecodeSet &ds, uint32_t g, int h, int j, uint4 (&rows)[4],
                                               int32_t &vn) {
    const int k = plane_of(ds, g);
    const uint32_t n = (g - first_of(ds, k)) * 32u + (uint32_t)j;
    const uint32_t m = n < (uint32_t)ds.pl[k].nblk ? n : 0u;
    const u4p *src = reinterpret_cast<const u4p *>(coef_of(ds, k) + (size_t)m * 64) + 4 * h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u4p t = __builtin_nontemporal_load(src + r);
        rows[r] = make_uint4(t.x, t.y, t.z, t.w);
    }
    if (ADAPTIVE) vn = __builtin_nontemporal_load(var_of(ds, k) + m);
}

template <bool ADAPTIVE, bool INV32>
__global__ __launch_bounds__(kThreadsP, 4) void decode8(DecodeSet ds, const DevTables *__restrict__ dev) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const uint32_t nbatch = ds.first[kMaxPlanes];
    const uint32_t step = gridDim.x * kWavesP;
    uint32_t g = blockIdx.x * kWavesP + wv;
    uint4 nxt[4];
    int32_t nvn = 0;
    prefetch_coefs<ADAPTIVE>(ds, g, h, j, nxt, nvn);
    for (; g < nbatch; g += step) {
        const int k = plane_of(ds, g);
        const PlaneArgs &p = ds.pl[k];
        const uint32_t n = (g - first_of(ds, k)) * 32u + (uint32_t)j;
        const bool valid = n < (uint32_t)p.nblk;
        uint4 cur[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) cur[r] = nxt[r];
        const int32_t vn = nvn;
        prefetch_coefs<ADAPTIVE>(ds, g + step, h, j, nxt, nvn);

        // the whole wave runs the arithmetic (exec-masked scales and lane-half swaps inside)
        u2p pix[4];
        const auto pack = [&pix](int r, int c, const float (&o)[4]) { pix[r][c >> 2] = pack_u8x4(o[0], o[1], o[2], o[3]); };
        if constexpr (INV32) inverse_half_f32_rows(dev, cur, h, pack);
        else inverse_half_rows<ADAPTIVE>(dev, cur, vn, h, pack);

        // rows 4h..4h+3 of block n, to their image position (decode_core.h)
        store_pixel_rows(p, n, valid, h, pix);
    }
}

hipError_t launch_decode(const DecodeSet &ds, const DevTables *dev, int adaptive, bool inv_f32, hipStream_t stream,
                         int num_cus) {
    return with_inverse(
        [&](auto a, auto f32) {
            return launch_persistent<decode8<a, f32>, kThreadsP, kWavesP, kDecodeGridMult>(ds.first[kMaxPlanes],
                                                                                         num_cus, stream, ds, dev);
        },
        adaptive != 0, inv_f32);
}

}  // namespace dctq
