// dct_amd/csrc/color_core.h -- what the colour kernels of color.hip (aligned, whole patches) and
// color_pad.hip (any size, any alignment) share: the patch numbering, the byte packing and the
// 8-byte plane accesses.  The transform itself is stated at the top of color.hip.
#ifndef DCTQ_COLOR_CORE_H
#define DCTQ_COLOR_CORE_H
#include "dctq_internal.h"

namespace dctq {

typedef uint32_t u2c __attribute__((ext_vector_type(2)));

constexpr int kColorThreads = 256;
constexpr int kColorWaves = kColorThreads / 64;

// byte k (a compile-time index after unrolling) of a row of dwords
template <int N>
__device__ __forceinline__ int byte_at(const uint32_t (&w)[N], int k) {
    return (int)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
}
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {  // four values in [0, 255]
    return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24;
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// (frame, patch row, patch column) of patch p
struct PatchPos {
    uint32_t f, row, col;
};
__device__ __forceinline__ PatchPos patch_pos(const ColorArgs &a, uint32_t p) {
    const uint32_t f = fdiv(p, a.div_frame), rem = p - f * a.per_frame;
    const uint32_t row = fdiv(rem, a.div_row);
    return PatchPos{f, row, rem - row * a.per_row};
}
__device__ __forceinline__ uint8_t *plane_ptr(uint8_t *base, long long stride, long long frame_stride, uint32_t f,
                                              uint32_t y, uint32_t byte) {
    return base + (long long)f * frame_stride + (long long)y * stride + byte;
}

__device__ __forceinline__ void store8(uint8_t *dst, const int (&v)[8]) {
    const u2c t = {pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7])};
    __builtin_nontemporal_store(t, reinterpret_cast<u2c *>(dst));
}
__device__ __forceinline__ void load8(const uint8_t *src, int (&v)[8]) {
    const u2c t = __builtin_nontemporal_load(reinterpret_cast<const u2c *>(src));
    const uint32_t w[2] = {t.x, t.y};
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = byte_at(w, i);
}

// 8 pixels of one row -> r, g, b.  V2 / V4: vectors of 2 / 4 dwords at the alignment the caller can promise
// (color.hip: 4; color_pad.hip: 1)
template <int STEP, typename V2, typename V4>
__device__ __forceinline__ void load_rgb8(const ColorArgs &a, const uint8_t *px, int (&r)[8], int (&g)[8], int (&b)[8]) {
    if constexpr (STEP == 1) {
        uint32_t w[3][2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const V2 t = __builtin_nontemporal_load(reinterpret_cast<const V2 *>(px + c * a.channel_stride));
            w[c][0] = t.x, w[c][1] = t.y;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = byte_at(w[0], i), g[i] = byte_at(w[1], i), b[i] = byte_at(w[2], i);
    } else {
        uint32_t w[2 * STEP];
        if constexpr (STEP == 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const V2 t = __builtin_nontemporal_load(reinterpret_cast<const V2 *>(px) + k);
                w[2 * k] = t.x, w[2 * k + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const V4 t = __builtin_nontemporal_load(reinterpret_cast<const V4 *>(px) + k);
                w[4 * k] = t.x, w[4 * k + 1] = t.y, w[4 * k + 2] = t.z, w[4 * k + 3] = t.w;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c0 = byte_at(w, STEP * i), c2 = byte_at(w, STEP * i + 2);
            r[i] = a.swap ? c2 : c0;
            g[i] = byte_at(w, STEP * i + 1);
            b[i] = a.swap ? c0 : c2;
        }
    }
}

// r, g, b in [0, 255] -> 8 pixels of one row; the fourth byte of a 4-byte pixel is 255
template <int STEP, typename V2, typename V4>
__device__ __forceinline__ void store_rgb8(const ColorArgs &a, uint8_t *px, const int (&r)[8], const int (&g)[8],
                                           const int (&b)[8]) {
    if constexpr (STEP == 1) {
        const u2c vr = {pack4(r[0], r[1], r[2], r[3]), pack4(r[4], r[5], r[6], r[7])};
        const u2c vg = {pack4(g[0], g[1], g[2], g[3]), pack4(g[4], g[5], g[6], g[7])};
        const u2c vb = {pack4(b[0], b[1], b[2], b[3]), pack4(b[4], b[5], b[6], b[7])};
        __builtin_nontemporal_store((V2)vr, reinterpret_cast<V2 *>(px));
        __builtin_nontemporal_store((V2)vg, reinterpret_cast<V2 *>(px + a.channel_stride));
        __builtin_nontemporal_store((V2)vb, reinterpret_cast<V2 *>(px + 2 * a.channel_stride));
    } else {
        int v[8 * STEP];  // the row's bytes in memory order
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[STEP * i] = a.swap ? b[i] : r[i];
            v[STEP * i + 1] = g[i];
            v[STEP * i + 2] = a.swap ? r[i] : b[i];
            if constexpr (STEP == 4) v[4 * i + 3] = 255;
        }
        uint32_t w[2 * STEP];
#pragma unroll
        for (int k = 0; k < 2 * STEP; ++k) w[k] = pack4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
        if constexpr (STEP == 3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const u2c t = {w[2 * k], w[2 * k + 1]};
                __builtin_nontemporal_store((V2)t, reinterpret_cast<V2 *>(px) + k);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const V4 t = {w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
                __builtin_nontemporal_store(t, reinterpret_cast<V4 *>(px) + k);
            }
        }
    }
}

// pixel_step and the subsampling into the template arguments, one leaf per combination
template <typename F>
static hipError_t with_layout(F &&f, int pixel_step, bool s420) {
    return with_bools(
        [&](auto s) {
            if (pixel_step == 1) return f(std::integral_constant<int, 1>(), s);
            if (pixel_step == 3) return f(std::integral_constant<int, 3>(), s);
            return f(std::integral_constant<int, 4>(), s);
        },
        s420);
}

}  // namespace dctq
#endif
