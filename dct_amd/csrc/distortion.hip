// dct_amd/csrc/distortion.hip -- dctq_distortion_planes: per-block squared error of the
// decoded u8 picture against its source, from pixels, in ONE launch and with no
// coefficient, recon or picture buffer:
//   sse[b] = sum over the 64 pixels of block b of (src - dec)^2,
//   dec    = (uint8) rne(min(max(r, 0), 255)),  r = fp32(dct_inverse(dequantize(q)) + 128),
//   q      = quantize(dct_forward(src - 128))
// i.e. dec is, bit for bit, the pixel dctq_forward_quant_planes + dctq_decode_planes write
// for that position (the reference's per-block loop tests/test_entropy.c:300-393 up to its
// squared error).  64 B in + 4 B out per block against the 192 + 192 + 128 B of that
// composition followed by a reduction over both pictures.
//
// The fused round trip (roundtrip.hip) with every picture-sized store removed.  One wave,
// one 64-block batch, over the wave's 8.5 KiB LDS stage:
//  1. forward, lane per block (fdct8_core.h), ties resolved in place: the inverse must see
//     the final ints.  Adaptive plans use the block's own var_num, which stays in registers;
//  2. lane (h, j) reads rows 4h..4h+3 of the quantized blocks j and 32 + j.  The stage is
//     free from then on (these inverses keep their rows in registers), so every lane writes
//     the 64 source bytes of its block into it and lane (h, j) reads back the matching
//     2 x 32 B: the source never goes through HBM twice;
//  3. two paired-lane inverses (inverse_core.h, the arithmetic of decode8 operation for
//     operation: fp32 for the plans its bound admits, fp64 otherwise) whose sink clamps and
//     rounds each pixel as pack_u8x4 does and accumulates (src - pix)^2: exact integers in
//     fp32 (<= 64 * 255^2 = 4 161 600 < 2^24).  One v_permlane32_swap adds the two half
//     blocks, after which lane l holds the error of block l of the batch;
//  4. one coalesced, non-temporal 256 B store per wave through a descriptor that ends at
//     the batch's last valid block: lanes past it store nothing, and an offset that went
//     wrong is dropped instead of faulting.
// Store-data hazard: the wave's only store is that one; the vmcnt(0) in
// front of the tie pass retires it (and the prefetch) before the batch's first LDS read.
#include "fdct8_core.h"
#include "inverse_core.h"
#include "pair_core.h"

namespace dctq {

// As roundtrip8: tie passes of <= 8 entries run 8 lanes per entry, no wide rounds (they
// spill at the 128-VGPR bound), pixel rows through a plane-bounded buffer descriptor.
constexpr bool kDistGroup8 = true;
constexpr int kDistWide = 0;
constexpr bool kDistBufRows = true;

// acc + (src - pix)^2 for pix = rne(clamp(r, 0, 255)): v_med3_f32 then v_rndne_f32, the
// value pack_u8x4 (decode_core.h) converts to a byte; that conversion is of an exact integer.
__device__ __forceinline__ float add_sq_err(float acc, float src, float r) {
    const float pix = __builtin_rintf(__builtin_amdgcn_fmed3f(r, 0.0f, 255.0f));
    const float e = src - pix;
    return __builtin_fmaf(e, e, acc);
}

// The inverse's sink: pixels c..c+3 of row r of the lane's half block against the four
// source bytes of the same position (src[r]: the row's 8 pixels).
struct SseSink {
    const uint2 (&src)[4];
    float &acc;
    __device__ __forceinline__ void operator()(int r, int c, const float (&o)[4]) const {
        const uint32_t w = c ? src[r].y : src[r].x;
        acc = add_sq_err(acc, cvt_ubyte<0>(w), o[0]);
        acc = add_sq_err(acc, cvt_ubyte<1>(w), o[1]);
        acc = add_sq_err(acc, cvt_ubyte<2>(w), o[2]);
        acc = add_sq_err(acc, cvt_ubyte<3>(w), o[3]);
    }
};

template <bool ADAPTIVE, bool INV32>
__global__ __launch_bounds__(kThreads, kRtOcc) void distortion8(EncodeSet es, const DevTables *__restrict__ dev,
                                                                uint32_t *__restrict__ sse) {
    __shared__ uint4 stage[kThreads * kPitch2 / 16];
    __shared__ ExactTables tab;
    __shared__ uint16_t scr[kWaves * 64];  // resolve_ties_compact's entries
    load_exact_tables(&tab, dev);
    const PlaneSet &ps = es.ps;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nbatch = ps.first[ps.n];
    const uint32_t step = gridDim.x * kWaves;
    uint32_t g = blockIdx.x * kWaves + wv;
    uint2 nxt[8];
    prefetch_batch<true, kDistBufRows>(ps, g, lane, nxt);
    fence_rows(nxt);
    char *wstage = reinterpret_cast<char *>(stage) + wv * 64 * kPitch2;
    for (; g < nbatch; g += step) {
        const int k = plane_of(ps, g);
        const PlaneArgs &p = ps.pl[k];
        const uint32_t b = g - first_of(ps, k);
        uint2 cur[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) cur[r] = nxt[r];
        const bool valid = b * 64 + lane < (uint32_t)p.nblk;
        prefetch_batch<false, kDistBufRows>(ps, g + step, lane, nxt);
        // the batch's 64 words of the output and the blocks it holds
        const uint32_t left = (uint32_t)p.nblk - b * 64;
        const uint32_t nb = left < 64u ? left : 64u;
        uint32_t *dst = sse + es.blk_first[k] + (size_t)b * 64;

        // ---- 1. forward into the stage; ties resolved in place
        int32_t var_num;
        uint32_t mlo, mhi;
        forward_flags_batch<ADAPTIVE, false>(dev, cur, stage, lane, wv, valid, var_num, mlo, mhi);
        // vmcnt(0): the previous batch's store (store-data hazard) and this batch's
        // prefetch before any LDS read
        retire_stores();
        resolve_ties_compact<ADAPTIVE, kDistGroup8, kDistWide>(&tab, cur, stage, scr + wv * 64, lane, wv, mlo, mhi);
        wave_sync();

        // ---- 2. read-back: the inverse's half blocks, then the source through the stage
        // (the lane roles from an opaque copy of the lane id, as roundtrip8)
        int ol = lane;
        asm volatile("" : "+v"(ol));
        const int h = ol >> 5, j = ol & 31;
        const uint2 *st64 = reinterpret_cast<const uint2 *>(wstage);
        const uint2 *sa = st64 + j * (kPitch2 / 8) + h * 8;  // block j, rows 4h..4h+3 (64 B of int16)
        const uint2 *sb = sa + 32 * (kPitch2 / 8);            // block 32 + j
        uint4 qa[4], qb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint2 a0 = sa[2 * r], a1 = sa[2 * r + 1], b0 = sb[2 * r], b1 = sb[2 * r + 1];
            qa[r] = make_uint4(a0.x, a0.y, a1.x, a1.y);
            qb[r] = make_uint4(b0.x, b0.y, b1.x, b1.y);
        }
        // lanes j / 32+j: var of block j in x, of block 32+j in y
        const auto vv = __builtin_amdgcn_permlane32_swap((uint32_t)var_num, (uint32_t)var_num, false, false);
        wave_sync();  // every lane has its coefficients: the stage is free
        {
            uint2 *own = reinterpret_cast<uint2 *>(wstage) + ol * (kPitch2 / 8);  // the lane's block: 64 B of pixels
#pragma unroll
            for (int r = 0; r < 8; ++r) own[r] = cur[r];
        }
        wave_sync();
        const uint2 *pa = st64 + j * (kPitch2 / 8) + h * 4;  // block j, pixel rows 4h..4h+3 (32 B)
        const uint2 *pb = pa + 32 * (kPitch2 / 8);            // block 32 + j
        uint2 src[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) src[r] = pa[r];

        // ---- 3. paired inverses, blocks 0-31 then 32-63 of the batch, into the error sums
        float ea = 0.0f, eb = 0.0f;
        if constexpr (INV32) inverse_half_f32_rows(dev, qa, h, SseSink{src, ea});
        else inverse_half_rows<ADAPTIVE>(dev, qa, (int32_t)vv[0], h, SseSink{src, ea});
#pragma unroll
        for (int r = 0; r < 4; ++r) src[r] = pb[r];
        wave_sync();  // the next batch's forward rewrites the stage only after these reads
        // keep inverse B's inputs packed until here (converted early they are 64 more live VGPRs)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(qb[r].x), "+v"(qb[r].y), "+v"(qb[r].z), "+v"(qb[r].w));
        if constexpr (INV32) inverse_half_f32_rows(dev, qb, h, SseSink{src, eb});
        else inverse_half_rows<ADAPTIVE>(dev, qb, (int32_t)vv[1], h, SseSink{src, eb});

        // ---- 4. lanes j / 32+j: both halves of block j / 32+j; lane l stores block l of the batch
        const auto ee = __builtin_amdgcn_permlane32_swap((uint32_t)ea, (uint32_t)eb, false, false);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst, (short)0, (int)(nb * 4u), kRsrcFlags);
        __builtin_amdgcn_raw_buffer_store_b32(ee[0] + ee[1], rs, lane * 4, 0, kNtAux);
    }
}

hipError_t launch_distortion(const EncodeSet &es, const DevTables *dev, int adaptive, bool inv_f32, uint32_t *sse,
                             hipStream_t stream, int num_cus) {
    return with_inverse(
        [&](auto a, auto f32) {
            return launch_persistent<distortion8<a, f32>, kThreads, kWaves, kRtGridMult>(es.ps.first[es.ps.n], num_cus,
                                                                                       stream, es, dev, sse);
        },
        adaptive != 0, inv_f32);
}

}  // namespace dctq
