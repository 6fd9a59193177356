// dct_amd/csrc/color.hip -- dctq_rgb_to_ycbcr_planes / dctq_ycbcr_to_rgb_planes: the colour
// front and back end of the codec, one launch each, no temporaries.
//
// Full-range BT.601 (JFIF) in 16-bit fixed point on int32, exactly as tools/color_ref.py
// states it (>> is an arithmetic shift):
//   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//   Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
//   Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16         (all in [0, 255]: no clamp)
//   4:2:0 chroma sample = (c00 + c01 + c10 + c11 + 2) >> 2 of the u8 Cb (Cr) of its 2x2 pixels
//   R = clamp(Y + (( 91881 cr + 32768) >> 16)),  cb = Cb - 128, cr = Cr - 128
//   G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16))
//   B = clamp(Y + ((116130 cb + 32768) >> 16));  4:2:0: a chroma sample serves its 2x2 pixels
// No floating point.  Every product is of a byte (or a centred byte) and a constant below
// 2^17, so the multiplies are 24-bit ones.
//
// A lane owns a patch of 8 pixels by 2 rows (4:2:0) or 1 row (4:4:4), patches in raster order
// (frame, patch row, patch column by fastdiv), grid-stride over all of them: consecutive
// lanes read consecutive 24 B (RGB), 32 B (RGBX) or 8 B per channel (planar) of a row -- whole
// dwords (dwordx2 / dwordx4; the RGB stack is only guaranteed dword-aligned) -- and write 8 B
// of Y per row and 4 B (4:2:0) or 8 B (4:4:4) each of Cb and Cr.  The inverse mirrors it.
// Every byte is touched once: non-temporal loads and stores.  A patch never reaches past
// width x height (widths are multiples of 8), so padding is untouched without any masking,
// and the loop bound p < npatch is the only guard an address needs.
// BGR / BGRX: the same instantiation; `swap` exchanges two registers per pixel after the
// load (before the store on the way back).
#include "color_core.h"

namespace dctq {

// vectors of dwords at dword alignment (what the RGB alignment rule guarantees)
typedef uint32_t u2a __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u4a __attribute__((ext_vector_type(4), aligned(4)));

// the lowest byte of pixel (8 col, y) of frame f: interleaved, the pixel's first byte in
// memory; planar, its R byte
template <int STEP>
__device__ __forceinline__ uint8_t *rgb_ptr(const ColorArgs &a, uint32_t f, uint32_t y, uint32_t col) {
    return a.rgb + (long long)f * a.rgb_frame_stride + (long long)y * a.rgb_stride + (long long)col * (8 * STEP);
}
template <int STEP, bool S420>
__global__ __launch_bounds__(kColorThreads) void rgb_to_ycc_kernel(ColorArgs a) {
    constexpr int kRows = S420 ? 2 : 1;
    const uint32_t step = gridDim.x * kColorThreads;
    for (uint32_t p = blockIdx.x * kColorThreads + threadIdx.x; p < a.npatch; p += step) {
        const PatchPos q = patch_pos(a, p);
        int sb[4] = {2, 2, 2, 2}, sr[4] = {2, 2, 2, 2};  // 4:2:0: the 2x2 sums, + 2 for the rounding
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const uint32_t y = q.row * kRows + j;
            int r[8], g[8], b[8], yy[8], cb[8], cr[8];
            load_rgb8<STEP, u2a, u4a>(a, rgb_ptr<STEP>(a, q.f, y, q.col), r, g, b);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                yy[i] = (19595 * r[i] + 38470 * g[i] + 7471 * b[i] + 32768) >> 16;
                cb[i] = (-11059 * r[i] - 21709 * g[i] + 32768 * b[i] + 8388608 + 32767) >> 16;
                cr[i] = (32768 * r[i] - 27439 * g[i] - 5329 * b[i] + 8388608 + 32767) >> 16;
            }
            store8(plane_ptr(a.y, a.y_stride, a.y_frame_stride, q.f, y, q.col * 8), yy);
            if constexpr (S420) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sb[i] += cb[2 * i] + cb[2 * i + 1], sr[i] += cr[2 * i] + cr[2 * i + 1];
            } else {
                store8(plane_ptr(a.cb, a.cb_stride, a.cb_frame_stride, q.f, y, q.col * 8), cb);
                store8(plane_ptr(a.cr, a.cr_stride, a.cr_frame_stride, q.f, y, q.col * 8), cr);
            }
        }
        if constexpr (S420) {
            __builtin_nontemporal_store(
                pack4(sb[0] >> 2, sb[1] >> 2, sb[2] >> 2, sb[3] >> 2),
                reinterpret_cast<uint32_t *>(plane_ptr(a.cb, a.cb_stride, a.cb_frame_stride, q.f, q.row, q.col * 4)));
            __builtin_nontemporal_store(
                pack4(sr[0] >> 2, sr[1] >> 2, sr[2] >> 2, sr[3] >> 2),
                reinterpret_cast<uint32_t *>(plane_ptr(a.cr, a.cr_stride, a.cr_frame_stride, q.f, q.row, q.col * 4)));
        }
    }
}

template <int STEP, bool S420>
__global__ __launch_bounds__(kColorThreads) void ycc_to_rgb_kernel(ColorArgs a) {
    constexpr int kRows = S420 ? 2 : 1;
    const uint32_t step = gridDim.x * kColorThreads;
    for (uint32_t p = blockIdx.x * kColorThreads + threadIdx.x; p < a.npatch; p += step) {
        const PatchPos q = patch_pos(a, p);
        int cb[8], cr[8];  // per pixel of a row, centred
        if constexpr (S420) {
            const uint32_t wb = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(
                plane_ptr(a.cb, a.cb_stride, a.cb_frame_stride, q.f, q.row, q.col * 4)));
            const uint32_t wr = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(
                plane_ptr(a.cr, a.cr_stride, a.cr_frame_stride, q.f, q.row, q.col * 4)));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                cb[i] = (int)((wb >> (8 * (i >> 1))) & 0xFFu) - 128;
                cr[i] = (int)((wr >> (8 * (i >> 1))) & 0xFFu) - 128;
            }
        } else {
            load8(plane_ptr(a.cb, a.cb_stride, a.cb_frame_stride, q.f, q.row, q.col * 8), cb);
            load8(plane_ptr(a.cr, a.cr_stride, a.cr_frame_stride, q.f, q.row, q.col * 8), cr);
#pragma unroll
            for (int i = 0; i < 8; ++i) cb[i] -= 128, cr[i] -= 128;
        }
        int dr[8], dg[8], db[8];  // the chroma terms, shared by the patch's rows
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dr[i] = (91881 * cr[i] + 32768) >> 16;
            dg[i] = (-22554 * cb[i] - 46802 * cr[i] + 32768) >> 16;
            db[i] = (116130 * cb[i] + 32768) >> 16;
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const uint32_t y = q.row * kRows + j;
            int yy[8], r[8], g[8], b[8];
            load8(plane_ptr(a.y, a.y_stride, a.y_frame_stride, q.f, y, q.col * 8), yy);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                r[i] = clamp255(yy[i] + dr[i]);
                g[i] = clamp255(yy[i] + dg[i]);
                b[i] = clamp255(yy[i] + db[i]);
            }
            store_rgb8<STEP, u2a, u4a>(a, rgb_ptr<STEP>(a, q.f, y, q.col), r, g, b);
        }
    }
}

hipError_t launch_rgb_to_ycc(const ColorArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus) {
    return with_layout(
        [&](auto step, auto s) {
            return launch_persistent<rgb_to_ycc_kernel<step, s>, kColorThreads, kColorWaves, kGridMult>(
                ((uint64_t)a.npatch + 63) / 64, num_cus, stream, a);
        },
        pixel_step, s420);
}

hipError_t launch_ycc_to_rgb(const ColorArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus) {
    return with_layout(
        [&](auto step, auto s) {
            return launch_persistent<ycc_to_rgb_kernel<step, s>, kColorThreads, kColorWaves, kGridMult>(
                ((uint64_t)a.npatch + 63) / 64, num_cus, stream, a);
        },
        pixel_step, s420);
}

}  // namespace dctq
