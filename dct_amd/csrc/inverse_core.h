// dct_amd/csrc/inverse_core.h -- dequantize + inverse DCT + 128 of one 32-block
// sub-batch in the paired-lane layout (lane (h, j): rows 4h..4h+3 of block j),
// shared by the fused round trip (roundtrip.hip: rows staged to LDS as fp32) and
// the pixel decoder (decode.hip: rows clamped and packed to u8 in registers).
// The *_rows functions hand the lane's four fp32 rows, in registers, to a sink as soon
// as each is final, four pixels at a time (sink(r, c, o): o = pixels c..c+3 of row r of
// the half block, c = 0 or 4); the inverse_half / inverse_half_f32 wrappers are the
// round trip's staging sink.
#pragma once
#include "fdct8_core.h"
#include "pair_core.h"

namespace dctq {

// Pixels c..c+3 of row r of the lane's half block -> their 16 B of the wave's stage
// (layout of idct8_pair).
struct StageSink {
    char *mine;
    __device__ __forceinline__ void operator()(int r, int c, const float (&o)[4]) const {
        *reinterpret_cast<float4 *>(mine + r * 32 + c * 4) = make_float4(o[0], o[1], o[2], o[3]);
    }
};

// Dequantize + inverse DCT + 128 of one 32-block sub-batch in fp64, lane (h, j)
// holding rows 4h..4h+3 of block j (8 int16 per uint4) and the block's var_num;
// one rounding to fp32 per pixel.  Adaptive plans and the non-adaptive plans the
// fp32 bound does not admit.
template <bool ADAPTIVE, typename Sink>
__device__ __forceinline__ void inverse_half_rows(const DevTables *__restrict__ dev, const uint4 (&q)[4], int32_t vn,
                                                  int h, const Sink &sink) {
    double v[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t w[4] = {q[r].x, q[r].y, q[r].z, q[r].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[r][2 * k] = (double)(int)(int16_t)(w[k] & 0xFFFFu);
            v[r][2 * k + 1] = (double)((int)w[k] >> 16);
        }
    }
    //   non-adaptive: q * (1/Q) S_u S_c      (src/quantization.c:139,144)
    //   adaptive:     q * Q S_u S_c * (2-nv), DC: q * Q S_0 S_0 (:137,144,193)
    ConstTables *tp = tables(dev);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ConstDouble *tlo = ADAPTIVE ? &tp->qscale[8 * r] : &tp->iscale[8 * r];
        ConstDouble *thi = ADAPTIVE ? &tp->qscale[8 * (r + 4)] : &tp->iscale[8 * (r + 4)];
        half_wave_scale(v[r], tlo, thi);
    }
    if (ADAPTIVE) {
        const double var = (double)vn / 4096.0;
        const double sc = 2.0 - fmin(1.0, fmax(0.1, var / 1000.0));
        const double dc = v[0][0];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) v[r][c] *= sc;
        if (h == 0) v[0][0] = dc;  // the DC keeps Q (src/quantization.c:198-199)
    }
    // + 128 on every output pixel = + 128 on the scaled DC (row 0 of the AAN
    // transpose graph is all ones and S_0^2 = 1/8 is already applied)
    if (h == 0) v[0][0] += 128.0;
    transpose_halves(v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        aan8t_d(v[0][k], v[1][k], v[2][k], v[3][k], v[0][k + 4], v[1][k + 4], v[2][k + 4], v[3][k + 4]);
    transpose_halves(v);
#pragma unroll
    for (int r = 0; r < 4; ++r) aan8t_d(v[r][0], v[r][1], v[r][2], v[r][3], v[r][4], v[r][5], v[r][6], v[r][7]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lo[4] = {(float)v[r][0], (float)v[r][1], (float)v[r][2], (float)v[r][3]};
        sink(r, 0, lo);
        const float hi[4] = {(float)v[r][4], (float)v[r][5], (float)v[r][6], (float)v[r][7]};
        sink(r, 4, hi);
    }
}

// ... fp32 rows into the wave's stage (the round trip).
template <bool ADAPTIVE>
__device__ __forceinline__ void inverse_half(const DevTables *__restrict__ dev, const uint4 (&q)[4], int32_t vn,
                                             int h, char *mine) {
    inverse_half_rows<ADAPTIVE>(dev, q, vn, h, StageSink{mine});
}

// The 8-point transposed AAN graph in fp32, operation for operation
// tools/aan_model.py aan8t (the graph tools/inv_bound.py bounds; aan8t_d in fp64),
// with the fp32 constants of fdct8_bound.h.  Every op is a separately rounded fp32
// add / sub / mul or an explicit fma (-ffp-contract=off).
__device__ __forceinline__ void aan8t_f(float &v0, float &v1, float &v2, float &v3, float &v4, float &v5, float &v6,
                                        float &v7) {
    const float gz13 = v5 + v3, gz2 = v5 - v3, gz11 = v1 + v7, gz4 = v1 - v7;
    float gb0 = gz11 + gz13;
    const float gz3 = gz11 - gz13;
    const float go1 = gz3 * DCTQ_C4;
    const float gz5 = (gz2 + gz4) * DCTQ_C6;
    const float go0 = __builtin_fmaf(DCTQ_C2MC6, gz2, gz5);
    const float go2 = __builtin_fmaf(DCTQ_C2PC6, gz4, -gz5);
    const float gb3 = go0, gb2 = go0 + go1, gb1 = go1 + go2;
    gb0 = gb0 + go2;
    float ge3 = v2 + v6;
    const float gm = v2 - v6;
    const float gs = gm * DCTQ_C4;
    const float ge2 = gs;
    ge3 = ge3 + gs;
    const float ge0 = v0 + v4, ge1 = v0 - v4;
    const float ga0 = ge0 + ge3, ga3 = ge0 - ge3, ga1 = ge1 + ge2, ga2 = ge1 - ge2;
    v0 = ga0 + gb0;
    v1 = ga1 + gb1;
    v2 = ga2 + gb2;
    v3 = ga3 + gb3;
    v4 = ga3 - gb3;
    v5 = ga2 - gb2;
    v6 = ga1 - gb1;
    v7 = ga0 - gb0;
}

// The fp32 inverse (non-adaptive plans admitted by plan_tables.hip inverse_f32_bound:
// |recon - reference| <= 5e-5 for every block of u8 pixels, e.g. q <= 71 of the standard
// table; for coefficients outside the plan's forward range, which the decoders accept,
// the bound grows linearly with the block's magnitudes (tools/inv_bound.py block_error);
// their dequantisation is the reference's q * (1/Q), src/quantization.c:139,
// 144), in inverse_half's paired-lane layout (lane (h, j): rows 4h..4h+3 of block j):
// x_uv = fl32(q_uv * fl32(iscale_uv)) (one v_pk_mul per coefficient pair, the scale
// pair of the lane's half-wave in SGPRs), the columns (after the exact lane-half
// transpose) then the rows through aan8t_f (src/dct.c:80-105 as D^T X D), then
// + 128 -- exactly the sequence tools/inv_bound.py bounds.  Half the fp64 kernel's
// VALU issue (profiles/r05/pmc_rt_*).  Lane per block (every lane inverting its own
// block in registers, no transposes, the 16 KiB of recon then leaving as two 8 KiB
// halves back to back) issued less still but ran 4.4-4.6 % slower on the bench step
// (profiles/r05/rt_ab.log): the paired layout's stores leave in three spaced
// groups (coefficients, half A after inverse A, half B after inverse B), which this
// write-heavy stream (64 B read : 384 B written per block) takes better than bursts.
__device__ __forceinline__ void swap_halves_f(float &x, float &y) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]);
    y = __uint_as_float(r[1]);
}
// v[k] (a row's pairs of coefficients) *= lo[k] in lanes 0-31 and *= hi[k] in lanes
// 32-63, both scale rows in SGPR pairs: two exec-masked v_pk_mul_f32 per pair (a
// per-lane select of the factor costs 2 v_mov + 1 v_cndmask per value, and spilled).
// The wave is fully active here; exec is saved and restored inside the block, and the
// block ends with the wait states a v_permlane read of its outputs needs (hipcc cannot
// see inside it).
typedef const __attribute__((address_space(4))) uint64_t ConstPair;
__device__ __forceinline__ void half_wave_scale_f32(f2 (&v)[4], ConstPair *lo, ConstPair *hi) {
    uint64_t save;
    asm volatile(
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b32 exec_hi, 0\n\t"
        "v_pk_mul_f32 %0, %0, %5\n\tv_pk_mul_f32 %1, %1, %6\n\tv_pk_mul_f32 %2, %2, %7\n\tv_pk_mul_f32 %3, %3, %8\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_mov_b32 exec_lo, 0\n\t"
        "v_pk_mul_f32 %0, %0, %9\n\tv_pk_mul_f32 %1, %1, %10\n\tv_pk_mul_f32 %2, %2, %11\n\tv_pk_mul_f32 %3, %3, %12\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_nop 1"  // VALU write -> v_permlane32_swap read (swap_halves_f next): 2 wait states, ours to pad
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), [sv] "=&s"(save)
        : "s"(lo[0]), "s"(lo[1]), "s"(lo[2]), "s"(lo[3]), "s"(hi[0]), "s"(hi[1]), "s"(hi[2]), "s"(hi[3]));
}

template <typename Sink>
__device__ __forceinline__ void inverse_half_f32_rows(const DevTables *__restrict__ dev, const uint4 (&q)[4], int h,
                                                      const Sink &sink) {
    float v[4][8];
    ConstTables *tp = tables(dev);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t w[4] = {q[r].x, q[r].y, q[r].z, q[r].w};
        f2 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = f2{(float)(int)(int16_t)(w[k] & 0xFFFFu), (float)((int)w[k] >> 16)};
        // row r of the half-wave: row r (lanes 0-31) or r + 4 (lanes 32-63) of the block
        half_wave_scale_f32(x, reinterpret_cast<ConstPair *>(&tp->iscale32[8 * r]),
                            reinterpret_cast<ConstPair *>(&tp->iscale32[8 * (r + 4)]));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[r][2 * k] = x[k].x;
            v[r][2 * k + 1] = x[k].y;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) swap_halves_f(v[r][k], v[r][k + 4]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        aan8t_f(v[0][k], v[1][k], v[2][k], v[3][k], v[0][k + 4], v[1][k + 4], v[2][k + 4], v[3][k + 4]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) swap_halves_f(v[r][k], v[r][k + 4]);
#pragma unroll
    for (int r = 0; r < 4; ++r) aan8t_f(v[r][0], v[r][1], v[r][2], v[r][3], v[r][4], v[r][5], v[r][6], v[r][7]);
    const f2 k128 = {128.0f, 128.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        f2 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = f2{v[r][2 * k], v[r][2 * k + 1]} + k128;
        const float lo[4] = {t[0].x, t[0].y, t[1].x, t[1].y}, hi[4] = {t[2].x, t[2].y, t[3].x, t[3].y};
        sink(r, 0, lo);
        sink(r, 4, hi);
    }
}

__device__ __forceinline__ void inverse_half_f32(const DevTables *__restrict__ dev, const uint4 (&q)[4], int h,
                                                 char *mine) {
    inverse_half_f32_rows(dev, q, h, StageSink{mine});
}

}  // namespace dctq
