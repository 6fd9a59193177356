// dct_amd/csrc/decode_core.h -- the pixel sink of the decoders: a lane's four fp32 rows
// of a half block clamped, rounded and packed to u8, and stored at their image position.
// Shared by decode8 (decode.hip: coefficients in) and symbols_to_pixels
// (decode_symbols.hip: run-length symbols in).
#pragma once
#include "inverse_core.h"

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

}  // namespace dctq
