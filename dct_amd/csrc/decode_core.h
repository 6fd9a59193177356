// dct_amd/csrc/decode_core.h -- the pixel sink of the decoders: a lane's four fp32 rows
// of a half block clamped, rounded and packed to u8, and stored at their image position.
// Shared by decode8 (decode.hip: coefficients in) and, with the read-out of the rebuilt rows
// and the inverse in front of it (pixel_rows_out), by symbols_to_pixels and bits_to_pixels
// (decode_symbols.hip, decode_bits.hip: a stream in).
#pragma once
#include "inverse_core.h"
#include "rle_decode_core.h"

namespace dctq {

// Four fp32 pixels -> 4 bytes: clamp to [0, 255] (v_med3_f32), round to nearest even
// (v_rndne_f32), then the conversion of an exact integer (v_cvt_pk_u8_f32 inserts byte
// k of the word).
__device__ __forceinline__ uint32_t pack_u8x4(float a, float b, float c, float d) {
    uint32_t w = 0u;
    w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(__builtin_amdgcn_fmed3f(a, 0.0f, 255.0f)), 0u, w);
    w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(__builtin_amdgcn_fmed3f(b, 0.0f, 255.0f)), 1u, w);
    w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(__builtin_amdgcn_fmed3f(c, 0.0f, 255.0f)), 2u, w);
    w = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_rintf(__builtin_amdgcn_fmed3f(d, 0.0f, 255.0f)), 3u, w);
    return w;
}

// pix[r] = the 8 pixels of row 4h + r of block n of plane p (wave-uniform p; frame, block
// row, block column), stored non-temporally by the lanes that are `valid`: through a
// buffer descriptor over the plane, so an address that went wrong drops the write, or
// with 64-bit addresses for a plane of 4 GiB or more (span == 0).
__device__ __forceinline__ void store_pixel_rows(const PlaneArgs &p, uint32_t n, bool valid, int h,
                                                 const u2p (&pix)[4]) {
    const uint32_t m = valid ? n : 0u;
    const uint32_t f = fdiv(m, p.div_frame);
    const uint32_t rem = m - f * (uint32_t)p.nblk_frame;
    const uint32_t by = fdiv(rem, p.div_bw);
    const uint32_t bx = rem - by * (uint32_t)p.bw;
    uint8_t *base = const_cast<uint8_t *>(p.src);
    if (p.span) {  // kernel argument: wave-uniform.  Every offset inside the plane is < 2^32
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)p.span, kRsrcFlags);
        const uint32_t st = (uint32_t)p.stride;
        const uint32_t off = f * (uint32_t)p.frame_stride + (by * 8u + 4u * (uint32_t)h) * st + bx * 8u;
        if (valid) {
#pragma unroll
            for (int r = 0; r < 4; ++r) __builtin_amdgcn_raw_buffer_store_b64(pix[r], rs, off + r * st, 0, kNtAux);
        }
    } else if (valid) {  // a plane of 4 GiB or more: 64-bit addresses
        uint8_t *px = base + (long long)f * p.frame_stride + (long long)(by * 8u + 4u * (uint32_t)h) * p.stride +
                      (long long)bx * 8;
#pragma unroll
        for (int r = 0; r < 4; ++r) __builtin_nontemporal_store(pix[r], reinterpret_cast<u2p *>(px + r * p.stride));
    }
}

// The pixel sink of decode_tiles (tile_decode_core.h): blocks [b0 + h, b0 + he) of the planes
// of ss, from the rows `rebuild` leaves in lt at pitch kDecPitch (four 16-B reads per lane
// without bank conflicts), through decode8's paired-lane inverse.  A half can straddle
// planes (the tiles run over the concatenated planes), so a block's plane, its number inside
// the plane and its var_num are per lane.  The store descriptor is per plane and
// wave-uniform: the wave loops over the planes present in the half (a wave-uniform range,
// at most four) with the lanes of other planes masked off.
template <bool ADAPTIVE, bool INV32, typename R>
__device__ __forceinline__ void pixel_rows_out(const SymbolSet &ss, const DevTables *__restrict__ dev, uint32_t b0,
                                               int h, int he, int lane, const char *lt, R &&rebuild) {
    const int hh = lane >> 5, j = lane & 31;
    // (a) lane (hh, j): block h + j of the tile; past the half's end, its last block (computed,
    // not stored).  var_num is asked for ahead of the rebuild, which hides its latency
    const uint32_t last = b0 + (uint32_t)he - 1u;
    const bool valid = h + j < he;
    const uint32_t gb = valid ? b0 + (uint32_t)(h + j) : last;
    const int kl = plane_of_block(ss, gb);
    const uint32_t n = gb - block_first_of(ss, kl);
    int32_t vn = 0;
    if (ADAPTIVE) vn = __builtin_nontemporal_load(var_of(ss, (uint32_t)kl) + n);

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

    // the planes present in the half, one descriptor each
    const int k_lo = __builtin_amdgcn_readfirstlane(plane_of_block(ss, b0 + (uint32_t)h));
    const int k_hi = __builtin_amdgcn_readfirstlane(plane_of_block(ss, last));
    for (int k = k_lo; k <= k_hi; ++k) store_pixel_rows(ss.pl[k], n, valid && kl == k, hh, pix);
}

}  // namespace dctq
