// dct_amd/csrc/roundtrip.hip -- the fused round trip (BASELINE configs[4],
// SURVEY 8(f) rank 1): for every block of up to 4 planes, in ONE launch,
//   coef  = quantize(dct_forward(px - 128))                 (bit-exact, as dctq_forward_quant)
//   recon = dct_inverse(dequantize(coef)) + 128              (fp32, |err| <= 1e-4, as dctq_inverse)
// i.e. the reference's per-block pipeline tests/test_entropy.c:300-330
// (create_block_from_pixels, dct_forward, calculate_block_variance, quantize,
// dequantize, dct_inverse) with the quantized ints handed to the inverse in LDS
// instead of through HBM: 64 B in, 128 + 256 B out per block (448 B) against
// 584 B for the two kernels back to back (coef and var_num written and re-read).
//
// One wave, one 64-block batch, three phases over the same 8.5 KiB LDS stage:
//  1. forward, lane per block (fdct8_core.h): fp32 AAN, quantization into the
//     stage, tie flags.  Flagged coefficients are recomputed in the reference's
//     exact fp64 order right here, by the lane that owns the block (its pixels
//     are still in registers), and patched into the stage -- the inverse must see
//     the final ints, so there is no deferral queue as in the forward kernel;
//  2. the stage is read back for the 1 KiB coefficient stores AND, per lane, the
//     two half blocks the paired inverse needs (lane (h, j): rows 4h..4h+3 of
//     blocks j and 32 + j); var_num follows by one v_permlane32_swap;
//  3. two paired-lane inverses (pair_core.h, as idct8_pair), 32 blocks each,
//     staged as fp32 rows and written as 1 KiB stores: fp32 arithmetic for the
//     plans a rigorous error bound admits (inverse_half_f32), fp64 otherwise.
// Store-data hazard: every LDS read-back that lands in VGPRs comes
// after a wait that retires the wave's pending stores -- the prefetch fence for
// phase 2, an explicit vmcnt(0) before each recon read-back.
#include "fdct8_core.h"
#include "inverse_core.h"
#include "pair_core.h"

namespace dctq {

// Passes of <= 8 tie entries run 8 lanes per entry (exact_grouped<8>): -4.9 % on the bench
// step (round 3); the wide rounds spill at these kernels' 128-VGPR bound.
constexpr bool kRtGroup8 = true;
constexpr int kRtWide = 0;
// Pixel rows through a plane-bounded buffer descriptor (load_rows<true>): a wrong row
// address reads zeros instead of faulting; within noise of global loads
// (profiles/r05/rt_ab_keep_late_rows.log).
constexpr bool kRtBufRows = true;

static_assert(kThreads == kThreadsP && 64 * kPitch2 == 32 * kPitchP, "forward and inverse share the wave's stage");

// The paired inverses (inverse_half<ADAPTIVE>, inverse_half_f32) live in inverse_core.h,
// shared with the pixel decoder (decode.hip).

template <bool ADAPTIVE, bool VAR, bool STATS, bool INV32 = false>
__global__ __launch_bounds__(kThreads, kRtOcc) void roundtrip8(RoundTripSet rt, const DevTables *__restrict__ dev,
                                                          unsigned long long *fallbacks) {
    __shared__ uint4 stage[kThreads * kPitch2 / 16];
    __shared__ ExactTables tab;
    __shared__ uint16_t scr[kWaves * 64];  // resolve_ties_compact's entries
    load_exact_tables(&tab, dev);
    const PlaneSet &ps = rt.ps;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nbatch = ps.first[ps.n];
    const uint32_t step = gridDim.x * kWaves;
    uint32_t g = blockIdx.x * kWaves + wv;
    uint2 nxt[8];
    prefetch_batch<true, kRtBufRows>(ps, g, lane, nxt);
    fence_rows(nxt);
    uint32_t exact_count = 0;
    char *wstage = reinterpret_cast<char *>(stage) + wv * 64 * kPitch2;
    for (; g < nbatch; g += step) {
        const int k = plane_of(ps, g);
        const PlaneArgs &p = ps.pl[k];
        const uint32_t b = g - first_of(ps, k);
        uint2 cur[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) cur[r] = nxt[r];
        const bool valid = b * 64 + lane < (uint32_t)p.nblk;
        prefetch_batch<false, kRtBufRows>(ps, g + step, lane, nxt);
        const BatchOut out = batch_out(ps, k, b);  // resolved before the fences (fdct8_core.h)
        char *recon = reinterpret_cast<char *>(rt.recon[k]) + (size_t)b * 64 * 256;
        asm volatile("" : "+s"(recon));

        // ---- 1. forward into the stage; ties resolved in place
        int32_t var_num;
        uint32_t mlo, mhi;
        forward_flags_batch<ADAPTIVE, VAR>(dev, cur, stage, lane, wv, valid, var_num, mlo, mhi);
        // vmcnt(0): the previous batch's recon stores (store-data hazard) and this
        // batch's prefetch before any LDS read.  Waiting later (the rows requested after the
        // forward, vmcnt(8)) or not at all before the recon read-backs (the pending stores' data
        // kept live instead) measured within noise (profiles/r05/rt_ab_keep_late_rows.log)
        retire_stores();
        const uint32_t ne =
            resolve_ties_compact<ADAPTIVE, kRtGroup8, kRtWide>(&tab, cur, stage, scr + wv * 64, lane, wv, mlo, mhi);
        if (STATS) exact_count += ne;
        wave_sync();

        // ---- 2. read-back: coefficient chunks + the inverse's half blocks
        const uint32_t nb = out.nb;
        // the inverse's lane roles from an opaque copy of the lane id: hoisted out of the
        // loop, these indices and the LDS addresses made of them sat in VGPRs across the
        // forward and pushed a prefetched row into scratch
        int ol = lane;
        asm volatile("" : "+v"(ol));
        const int h = ol >> 5, j = ol & 31;
        u4v val[8];
        stage_chunks(stage, wv, lane, val);
        const uint2 *st64 = reinterpret_cast<const uint2 *>(wstage);
        uint4 qa[4], qb[4];
        {
            const uint2 *sa = st64 + j * (kPitch2 / 8) + h * 8;  // block j, rows 4h..4h+3 (64 B)
            const uint2 *sb = sa + 32 * (kPitch2 / 8);            // block 32 + j
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint2 a0 = sa[2 * r], a1 = sa[2 * r + 1], b0 = sb[2 * r], b1 = sb[2 * r + 1];
                qa[r] = make_uint4(a0.x, a0.y, a1.x, a1.y);
                qb[r] = make_uint4(b0.x, b0.y, b1.x, b1.y);
            }
        }
        // lanes j / 32+j: var of block j in x, of block 32+j in y
        const auto vv = __builtin_amdgcn_permlane32_swap((uint32_t)var_num, (uint32_t)var_num, false, false);
        {  // store_batch<VAR>, spelled out (fdct8_core.h)
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(out.base, (short)0, (int)(nb * 128u), kRsrcFlags);
#pragma unroll
            for (int c = 0; c < 8; ++c) __builtin_amdgcn_raw_buffer_store_b128(val[c], rs, lane * 16, c * 1024, kNtAux);
            if (VAR) {
                const __amdgpu_buffer_rsrc_t rv =
                    __builtin_amdgcn_make_buffer_rsrc(out.var, (short)0, (int)(nb * 4u), kRsrcFlags);
                __builtin_amdgcn_raw_buffer_store_b32(var_num, rv, lane * 4, 0, kNtAux);
            }
        }

        // ---- 3. paired inverses, blocks 0-31 then 32-63 of the batch
        char *mine = wstage + j * kPitchP + h * 128;
        if constexpr (INV32) inverse_half_f32(dev, qa, h, mine);
        else inverse_half<ADAPTIVE>(dev, qa, (int32_t)vv[0], h, mine);
        retire_stores();
        wave_sync();
        store_stage(stage, wv, lane, recon, (nb < 32u ? nb : 32u) * 256u);
        // keep inverse B's inputs packed until here (converted early they are 64 more live VGPRs)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(qb[r].x), "+v"(qb[r].y), "+v"(qb[r].z), "+v"(qb[r].w));
        if constexpr (INV32) inverse_half_f32(dev, qb, h, mine);
        else inverse_half<ADAPTIVE>(dev, qb, (int32_t)vv[1], h, mine);
        retire_stores();
        wave_sync();
        store_stage(stage, wv, lane, recon + 32 * 256, (nb > 32u ? nb - 32u : 0u) * 256u);
    }
    if (STATS) {
        uint32_t tot = exact_count;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
        if (lane == 0 && tot) atomicAdd(fallbacks, (unsigned long long)tot);
    }
}

hipError_t launch_roundtrip(const RoundTripSet &rt, const DevTables *dev, int adaptive, bool inv_f32,
                            unsigned long long *fallbacks, hipStream_t stream, int num_cus) {
    return with_bools(
        [&](auto v, auto s) {
            return with_inverse(
                [&](auto a, auto f32) {
                    return launch_persistent<roundtrip8<a, decltype(v)::value, decltype(s)::value, f32>, kThreads,
                                             kWaves, kRtGridMult>(rt.ps.first[rt.ps.n], num_cus, stream, rt, dev,
                                                                  fallbacks);
                },
                adaptive != 0, inv_f32);
        },
        rt.ps.var[0] != nullptr, fallbacks != nullptr);
}

}  // namespace dctq
