// dct_amd/csrc/color_pad.hip -- dctq_rgb_to_ycbcr_pad_planes / dctq_ycbcr_to_rgb_crop_planes /
// dctq_pad_planes: the colour front and back end of color.hip for a picture of ANY size at ANY
// alignment, one launch each, no temporaries.
//
// The picture W x H is extended to W' x H' (the next multiples of 8, or of 16 in 4:2:0) by
//   pixel'(x, y) = pixel(min(x, W - 1), min(y, H - 1)),
// the transform of color.hip runs on the extended picture, and the way back writes only the
// pixels with x < W and y < H (tools/color_ref.py: forward_padded, inverse_cropped).
//
// The lane-per-patch layout of color.hip, patches numbered over the EXTENDED picture.  A patch
// column is one of three kinds:
//   interior    8 col + 8 <= W: the row's 24 / 32 / 8 B per channel move as dwordx2 / dwordx4,
//               exactly as in color.hip, but at byte alignment: gfx950 under HSA runs global
//               memory in unaligned access mode, so the compiler emits the same global_load /
//               global_store_dwordx2 / x4 for a vector type of alignment 1 (read off the
//               disassembly).  This is the hot path: every patch but one column.
//   straddling  8 col < W < 8 col + 8: a byte load per pixel and channel at x = min(x, W - 1);
//               on the way back a byte store per pixel and channel with x < W.
//   outside     8 col >= W (4:2:0 only: W' - W >= 8): the same clamped byte loads, which all hit
//               pixel W - 1 of the row; on the way back nothing is loaded or stored.
// Rows at y >= H read row H - 1 on the way in and are skipped on the way back.
// Reads: the forward reads bytes of the W x H pixels only (of a 4-byte pixel also its fourth
// byte), never a byte beside them -- there is no over-read to bound.  Writes: the forward writes
// whole 8-byte granules of the W' x H' planes, which are dctq_planes (8-byte aligned); the
// inverse writes exactly the bytes of the W x H pixels.  No LDS, no scratch.
#include "color_core.h"

namespace dctq {

// vectors of dwords at byte alignment
typedef uint32_t u2u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u4u __attribute__((ext_vector_type(4), aligned(1)));

// the lowest byte of pixel (0, y) of frame f
__device__ __forceinline__ uint8_t *rgb_row(const ColorArgs &a, uint32_t f, uint32_t y) {
    return a.rgb + (long long)f * a.rgb_frame_stride + (long long)y * a.rgb_stride;
}

// pixels min(x0 + i, xmax), i = 0..7, of one row -> r, g, b: a byte per pixel and channel
template <int STEP>
__device__ __forceinline__ void load_rgb8_clamped(const ColorArgs &a, const uint8_t *row, uint32_t x0, uint32_t xmax,
                                                  int (&r)[8], int (&g)[8], int (&b)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t x = x0 + i < xmax ? x0 + i : xmax;
        const uint8_t *p = row + (long long)x * STEP;
        if constexpr (STEP == 1) {
            r[i] = p[0], g[i] = p[a.channel_stride], b[i] = p[2 * a.channel_stride];
        } else {
            const int c0 = p[0], c2 = p[2];
            r[i] = a.swap ? c2 : c0;
            g[i] = p[1];
            b[i] = a.swap ? c0 : c2;
        }
    }
}

// the first n (1..7) of 8 pixels -> one row at px: a byte per pixel and channel
template <int STEP>
__device__ __forceinline__ void store_rgb8_first(const ColorArgs &a, uint8_t *px, uint32_t n, const int (&r)[8],
                                                 const int (&g)[8], const int (&b)[8]) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        if ((uint32_t)i < n) {
            uint8_t *p = px + i * STEP;
            if constexpr (STEP == 1) {
                p[0] = (uint8_t)r[i], p[a.channel_stride] = (uint8_t)g[i], p[2 * a.channel_stride] = (uint8_t)b[i];
            } else {
                p[0] = (uint8_t)(a.swap ? b[i] : r[i]);
                p[1] = (uint8_t)g[i];
                p[2] = (uint8_t)(a.swap ? r[i] : b[i]);
                if constexpr (STEP == 4) p[3] = 255;
            }
        }
    }
}

template <int STEP, bool S420>
__global__ __launch_bounds__(kColorThreads) void rgb_to_ycc_pad_kernel(ColorPadArgs ap) {
    constexpr int kRows = S420 ? 2 : 1;
    const ColorArgs &a = ap.c;
    const uint32_t step = gridDim.x * kColorThreads;
    for (uint32_t p = blockIdx.x * kColorThreads + threadIdx.x; p < a.npatch; p += step) {
        const PatchPos q = patch_pos(a, p);
        const uint32_t x0 = q.col * 8;
        const bool interior = x0 + 8 <= ap.width;
        // both rows' loads under ONE branch, so that they are all in flight before the first is used
        int rr[kRows][8], gg[kRows][8], bb[kRows][8];
        if (interior) {
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                const uint32_t y = q.row * kRows + j;
                load_rgb8<STEP, u2u, u4u>(a, rgb_row(a, q.f, y < ap.height ? y : ap.height - 1) + (long long)x0 * STEP,
                                          rr[j], gg[j], bb[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < kRows; ++j) {
                const uint32_t y = q.row * kRows + j;
                load_rgb8_clamped<STEP>(a, rgb_row(a, q.f, y < ap.height ? y : ap.height - 1), x0, ap.width - 1, rr[j],
                                        gg[j], bb[j]);
            }
        }
        int sb[4] = {2, 2, 2, 2}, sr[4] = {2, 2, 2, 2};  // 4:2:0: the 2x2 sums, + 2 for the rounding
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const uint32_t y = q.row * kRows + j;
            const int(&r)[8] = rr[j], (&g)[8] = gg[j], (&b)[8] = bb[j];
            int yy[8], cb[8], cr[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                yy[i] = (19595 * r[i] + 38470 * g[i] + 7471 * b[i] + 32768) >> 16;
                cb[i] = (-11059 * r[i] - 21709 * g[i] + 32768 * b[i] + 8388608 + 32767) >> 16;
                cr[i] = (32768 * r[i] - 27439 * g[i] - 5329 * b[i] + 8388608 + 32767) >> 16;
            }
            store8(plane_ptr(a.y, a.y_stride, a.y_frame_stride, q.f, y, x0), yy);
            if constexpr (S420) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sb[i] += cb[2 * i] + cb[2 * i + 1], sr[i] += cr[2 * i] + cr[2 * i + 1];
            } else {
                store8(plane_ptr(a.cb, a.cb_stride, a.cb_frame_stride, q.f, y, x0), cb);
                store8(plane_ptr(a.cr, a.cr_stride, a.cr_frame_stride, q.f, y, x0), cr);
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
__global__ __launch_bounds__(kColorThreads) void ycc_to_rgb_crop_kernel(ColorPadArgs ap) {
    constexpr int kRows = S420 ? 2 : 1;
    const ColorArgs &a = ap.c;
    const uint32_t step = gridDim.x * kColorThreads;
    for (uint32_t p = blockIdx.x * kColorThreads + threadIdx.x; p < a.npatch; p += step) {
        const PatchPos q = patch_pos(a, p);
        const uint32_t x0 = q.col * 8;
        if (x0 >= ap.width || q.row * kRows >= ap.height) continue;  // a patch of padding only: nothing to write
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
            load8(plane_ptr(a.cb, a.cb_stride, a.cb_frame_stride, q.f, q.row, x0), cb);
            load8(plane_ptr(a.cr, a.cr_stride, a.cr_frame_stride, q.f, q.row, x0), cr);
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
            if (y >= ap.height) continue;
            int yy[8], r[8], g[8], b[8];
            load8(plane_ptr(a.y, a.y_stride, a.y_frame_stride, q.f, y, x0), yy);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                r[i] = clamp255(yy[i] + dr[i]);
                g[i] = clamp255(yy[i] + dg[i]);
                b[i] = clamp255(yy[i] + db[i]);
            }
            uint8_t *px = rgb_row(a, q.f, y) + (long long)x0 * STEP;
            if (x0 + 8 <= ap.width)
                store_rgb8<STEP, u2u, u4u>(a, px, r, g, b);
            else
                store_rgb8_first<STEP>(a, px, ap.width - x0, r, g, b);
        }
    }
}

// Plain planes: every destination granule of 8 bytes from the source row min(y, h - 1); an
// interior granule is one 8-byte load at byte alignment, the others a clamped byte per pixel.
// One plane after the other inside the launch, each over the whole grid: the plane index is a
// compile-time constant after unrolling, so its arguments stay in SGPRs.
__global__ __launch_bounds__(kColorThreads) void pad_planes_kernel(PadSet s) {
    const uint32_t step = gridDim.x * kColorThreads;
#pragma unroll
    for (int k = 0; k < kMaxPlanes; ++k) {
        if (k >= s.n) break;
        const PadPlane &pl = s.pl[k];
        for (uint32_t p = blockIdx.x * kColorThreads + threadIdx.x; p < pl.npatch; p += step) {
            const uint32_t f = fdiv(p, pl.div_frame), rem = p - f * pl.per_frame;
            const uint32_t y = fdiv(rem, pl.div_row), x0 = (rem - y * pl.per_row) * 8;
            const uint8_t *row = pl.src + (long long)f * pl.src_frame_stride +
                                 (long long)(y < pl.height ? y : pl.height - 1) * pl.src_stride;
            u2c t;
            if (x0 + 8 <= pl.width) {
                t = (u2c)__builtin_nontemporal_load(reinterpret_cast<const u2u *>(row + x0));
            } else {
                int v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = row[x0 + i < pl.width - 1 ? x0 + i : pl.width - 1];
                t = u2c{pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7])};
            }
            __builtin_nontemporal_store(t, reinterpret_cast<u2c *>(pl.dst + (long long)f * pl.dst_frame_stride +
                                                                   (long long)y * pl.dst_stride + x0));
        }
    }
}

hipError_t launch_rgb_to_ycc_pad(const ColorPadArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus) {
    return with_layout(
        [&](auto step, auto s) {
            return launch_persistent<rgb_to_ycc_pad_kernel<step, s>, kColorThreads, kColorWaves, kGridMult>(
                ((uint64_t)a.c.npatch + 63) / 64, num_cus, stream, a);
        },
        pixel_step, s420);
}

hipError_t launch_ycc_to_rgb_crop(const ColorPadArgs &a, int pixel_step, bool s420, hipStream_t stream, int num_cus) {
    return with_layout(
        [&](auto step, auto s) {
            return launch_persistent<ycc_to_rgb_crop_kernel<step, s>, kColorThreads, kColorWaves, kGridMult>(
                ((uint64_t)a.c.npatch + 63) / 64, num_cus, stream, a);
        },
        pixel_step, s420);
}

hipError_t launch_pad_planes(const PadSet &s, hipStream_t stream, int num_cus) {
    uint32_t most = 0;  // the grid is sized for the largest plane: the others take fewer trips
    for (int k = 0; k < s.n; ++k) most = s.pl[k].npatch > most ? s.pl[k].npatch : most;
    return launch_persistent<pad_planes_kernel, kColorThreads, kColorWaves, kGridMult>(((uint64_t)most + 63) / 64,
                                                                                      num_cus, stream, s);
}

}  // namespace dctq
