// dct_amd/csrc/rle_decode_core.h -- the run-length decoder's half tile: 32 blocks of a
// symbol stream rebuilt as natural-order int16 rows in a wave's LDS.  Shared by
// rle_decode_kernel (rle.hip: the rows leave as coefficients) and symbols_to_pixels
// (decode_symbols.hip: the rows go straight into the inverse DCT).
#pragma once
#include "dctq_internal.h"

namespace dctq {

// A symbol of value v (int16 bits in the low half of `v16`) and run r in format W.
template <int W>
__device__ __forceinline__ uint32_t pack_sym(uint32_t v16, uint32_t r) {
    if constexpr (W == 4) return (v16 & 0xFFFFu) | (r << 16);
    else return ((r & 63u) << 10) | (v16 & 0x3FFu);  // (0, 64) -> 0x0000
}
// ... and back: the run, and the value as int16 bits (sign-extended from 10 bits for W = 2)
template <int W>
__device__ __forceinline__ uint32_t sym_run(uint32_t s) {
    if constexpr (W == 4) return s >> 16;
    else return (s & 0xFFFFu) ? (s >> 10) & 0x3Fu : 64u;
}
template <int W>
__device__ __forceinline__ int16_t sym_value(uint32_t s) {
    if constexpr (W == 4) return (int16_t)(s & 0xFFFFu);
    else return (int16_t)((int32_t)(s << 22) >> 22);
}

__device__ __forceinline__ int tile_blocks(long long t, long long nblk) {
    const long long r = nblk - t * 64;
    return r < 0 ? 0 : r < 64 ? (int)r : 64;
}
typedef uint32_t u4r __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- decode: one wave per 64-block tile, rebuilt 32 blocks at a time in a
// natural-order LDS copy.  Each half takes one of three paths by its symbol
// count: lane (<= 240), walk (<= kDecWalkMax) or quad (denser halves);
// all three place each symbol at zigzag position pos (run_length_decode: pos +=
// run; zigzag[pos++] = value, dropped past the end, src/entropy.c:327-351) of
// its block's natural-order row (zigzag_to_block, :183-210, through an LDS copy
// of the order).  Every symbol load goes through a buffer descriptor whose
// num_records ends at the half's last symbol, so no path reads past the
// stream.  Each half tile's LDS work starts after a vmcnt(0) that retires the
// previous half's stores (store-data hazard); no store is issued inside the half.
constexpr int kHalf = 32;

// offv: lane b holds offsets[64t + b] (b < nb); oend = offsets[64t + nb], the end
// of the tile's symbols (lane 64 does not exist, and readlane(64) would wrap).
__device__ __forceinline__ uint32_t off_at(uint32_t offv, uint32_t oend, int b) {
    return b < 64 ? __builtin_amdgcn_readlane(offv, b) : oend;
}

// Walk path (a half tile of at most kDecWalkMax symbols): lane i < 32 rebuilds
// block h+i on its own -- its symbols as 16-B loads (four per lane-address,
// the next kDecBatch in flight while these are placed), each value written at
// zigzag[pos] of its row in a zeroed natural-order half tile (pos += run; put
// while pos < 64; pos++).  The row pitch is 144 B: a symbol past position 63
// or past the block's count lands in the row's 16-B padding, so placement is
// branch-free.  A block's count is clamped to 64, which bounds the walk for
// any offsets.  Denser halves take the scan-and-scatter path (same pitch).
//
// Lane path (a half tile of at most kDecLaneMax symbols: natural content): the
// half's symbols come in as coalesced dword loads and go to LDS behind the
// zeroed half tile (pitch LANE_PITCH), and lane i < 32 walks block h+i's symbols
// from there, clamped to the half's symbols.  Faster than the walk path at this
// density (one coalesced load per 64 symbols instead of per-lane 16-B loads).
constexpr uint32_t kDecLaneMax = 240, kDecWalkMax = 1024;
constexpr int kDecPitch = 144;
constexpr int kDecBatch = 16;  // symbols per lane per step
// a wave's LDS for a lane-path row pitch: the half tile, then the lane path's symbols
constexpr int dec_lds_bytes(int lane_pitch) { return kHalf * lane_pitch + (int)kDecLaneMax * 4; }
static_assert(dec_lds_bytes(128) >= kHalf * kDecPitch, "walk path tile");

// 2-B symbols widened to the 4-B format in registers: the decode paths below then
// run unchanged.  Units sit two per dword; a lane whose units start at an odd unit
// loads from the dword before and shifts by 16 bits (v_alignbit).
__device__ __forceinline__ uint32_t widen16(uint32_t u) {
    return pack_sym<4>((uint32_t)(uint16_t)sym_value<2>(u), sym_run<2>(u));
}
// units [u, u + 2N) from dword-aligned `d` (N + 1 dwords: d[0] holds unit u & ~1)
template <int N>
__device__ __forceinline__ void align_units(const uint32_t (&d)[N + 1], uint32_t odd, uint32_t (&out)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], odd * 16u);
}

// Blocks [h, he) of a tile (he - h <= kHalf) into the wave's LDS `lt` (dec_lds_bytes(LANE_PITCH)
// bytes; lsym = lt + kHalf * LANE_PITCH, where the lane path keeps its symbols): block h+i's natural-order row at lt + i * pitch,
// pitch = LANE_PITCH when the lane path ran (the return value), kDecPitch otherwise.
// offv / oend as off_at; cnt_lane: lane b holds block b's symbol count; zz: the zigzag
// order in LDS.  Issues no store; the caller follows with wave_sync_lds() and
// retire_stores() (the walk's last clipped loads) before it reads the rows.
template <int W, int LANE_PITCH>
__device__ __forceinline__ bool rebuild_half(const void *__restrict__ symbols, uint32_t offv, uint32_t oend,
                                             uint32_t cnt_lane, int h, int he, int lane, char *lt, uint32_t *lsym,
                                             const uint8_t (&zz)[64]) {
    static_assert(LANE_PITCH >= 128 && LANE_PITCH % 16 == 0, "a row is 128 B, zeroed 16 B at a time");
    constexpr int kZero16 = kHalf * LANE_PITCH / 16;  // 16-B units of the lane path's half tile
    const uint32_t s0 = __builtin_amdgcn_readlane(offv, h), nh = off_at(offv, oend, he) - s0;
    const bool lane_path = kDecLaneMax && nh <= kDecLaneMax;
    const bool walk = !lane_path && kDecWalkMax && nh <= kDecWalkMax;
    if (lane_path) {
        const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char *>(reinterpret_cast<const char *>(symbols)) + (unsigned long long)s0 * W, (short)0,
            (int)(nh * W), kRsrcFlags);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // past nh: clipped to 0, no traffic
            if constexpr (W == 4)
                v[j] = __builtin_amdgcn_raw_buffer_load_b32(rsy, (j * 64 + lane) * 4, 0, 0);
            else
                v[j] = widen16(__builtin_amdgcn_raw_buffer_load_b16(rsy, (j * 64 + lane) * 2, 0, 0));
        }
        // block h+i's start and count, to lane i
        const uint32_t my_off = (uint32_t)__shfl((int)offv, (lane + h) & 63);
        const uint32_t my_cnt = (uint32_t)__shfl((int)cnt_lane, (lane + h) & 63);
        // vmcnt(0): these loads, and the previous half's stores before any LDS read (store-data hazard)
        retire_stores();
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < 3 || lane < 48) lsym[j * 64 + lane] = v[j];
#pragma unroll
        for (int k = 0; k < kZero16 / 64; ++k) reinterpret_cast<u4r *>(lt)[k * 64 + lane] = u4r{0u, 0u, 0u, 0u};
        if constexpr (kZero16 % 64 != 0) {
            if (lane < kZero16 % 64) reinterpret_cast<u4r *>(lt)[kZero16 / 64 * 64 + lane] = u4r{0u, 0u, 0u, 0u};
        }
        wave_sync_lds();
        // a block's symbols must lie inside the half's (bounds the walk for any offsets)
        const uint32_t base = my_off - s0;
        const uint32_t cnt = lane < he - h && base <= nh ? (my_cnt < nh - base ? my_cnt : nh - base) : 0u;
        int16_t *row = reinterpret_cast<int16_t *>(lt + (lane & 31) * LANE_PITCH);
        uint32_t pos = 0;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t sym = lsym[base + i];
            pos += sym >> 16;
            if (pos < 64u) row[zz[pos]] = (int16_t)(sym & 0xFFFFu);
            pos += 1u;
        }
    } else if (walk) {
        // the half's symbols; loads past them (any lane, any offsets) are clipped to 0.
        // 2-B units: the descriptor starts at the even unit at or before s0 and ends on
        // a whole dword (one unit past the half at most: inside the stream's 4-B-aligned
        // allocation)
        const uint32_t pad = W == 2 ? (s0 & 1u) : 0u;
        const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char *>(reinterpret_cast<const char *>(symbols)) + (unsigned long long)(s0 - pad) * W,
            (short)0, (int)(W == 4 ? nh * 4u : ((pad + nh + 1u) & ~1u) * 2u), kRsrcFlags);
        const uint32_t my_off = (uint32_t)__shfl((int)offv, (lane + h) & 63);
        const uint32_t my_cnt = (uint32_t)__shfl((int)cnt_lane, (lane + h) & 63);
        const uint32_t cnt = lane < he - h ? (my_cnt < 64u ? my_cnt : 64u) : 0u;
        const uint32_t urel = my_off - s0 + pad;  // the block's first unit from the descriptor base
        const uint32_t rel = W == 4 ? (my_off - s0) * 4u : (urel & ~1u) * 2u, odd = urel & 1u;
        auto load_batch = [&](uint32_t i, u4r (&q)[kDecBatch / 4]) {
            if constexpr (W == 4) {
#pragma unroll
                for (int k = 0; k < kDecBatch / 4; ++k)
                    q[k] = i + 4 * k < cnt ? __builtin_amdgcn_raw_buffer_load_b128(rsy, rel + (i + 4 * k) * 4u, 0, 0)
                                           : u4r{0u, 0u, 0u, 0u};
            } else {  // kDecBatch units = 8 dwords, from 9 aligned ones
                uint32_t d[kDecBatch / 2 + 1];
#pragma unroll
                for (int k = 0; k < kDecBatch / 8; ++k) {
                    // dwords 4k..4k+3 hold units i + 8k - odd .. i + 8k - odd + 7
                    const u4r t = i + 8 * k < cnt + odd
                                      ? __builtin_amdgcn_raw_buffer_load_b128(rsy, rel + (i + 8 * k) * 2u, 0, 0)
                                      : u4r{0u, 0u, 0u, 0u};
                    d[4 * k] = t[0], d[4 * k + 1] = t[1], d[4 * k + 2] = t[2], d[4 * k + 3] = t[3];
                }
                d[kDecBatch / 2] = odd && i + kDecBatch - 1 < cnt
                                       ? __builtin_amdgcn_raw_buffer_load_b32(rsy, rel + (i + kDecBatch) * 2u, 0, 0)
                                       : 0u;
                uint32_t a[kDecBatch / 2];
                align_units<kDecBatch / 2>(d, odd, a);
#pragma unroll
                for (int k = 0; k < kDecBatch / 4; ++k)
                    q[k] = u4r{widen16(a[2 * k]), widen16(a[2 * k] >> 16), widen16(a[2 * k + 1]),
                               widen16(a[2 * k + 1] >> 16)};
            }
        };
        u4r cur[kDecBatch / 4];
        load_batch(0, cur);
        // vmcnt(0) before any LDS read into registers: the previous half's stores
        // (store-data hazard); the walk's own loads are in the same count
        retire_stores();
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < 4 || lane < 32) reinterpret_cast<u4r *>(lt)[k * 64 + lane] = u4r{0u, 0u, 0u, 0u};
        wave_sync_lds();
        char *row = lt + (lane & 31) * kDecPitch;
        uint32_t pos = 0;
        for (uint32_t i = 0; __builtin_amdgcn_ballot_w64(i < cnt); i += kDecBatch) {
            u4r nxt[kDecBatch / 4];
            load_batch(i + kDecBatch, nxt);
#pragma unroll
            for (int j = 0; j < kDecBatch; ++j) {
                const uint32_t sym = cur[j >> 2][j & 3];
                pos += sym >> 16;
                const bool put = pos < 64u && i + j < cnt;
                const uint32_t at = put ? 2u * zz[pos < 64u ? pos : 63u] : 128u;  // 128: the padding
                *reinterpret_cast<int16_t *>(row + at) = (int16_t)(sym & 0xFFFFu);
                pos += 1u;
            }
#pragma unroll
            for (int k = 0; k < kDecBatch / 4; ++k) cur[k] = nxt[k];
        }
    } else {
        // Quad path: 4 blocks per step, one per 16-lane row; lane s of a row holds its
        // block's symbols 4s..4s+3 (one 16-B load: 4 symbols per lane-address). Positions:
        // a 4-element prefix in the lane, then a row-segmented DPP scan of the lane totals.
        const uint32_t pad = W == 2 ? (s0 & 1u) : 0u;  // as the walk path
        const __amdgpu_buffer_rsrc_t rsy = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char *>(reinterpret_cast<const char *>(symbols)) + (unsigned long long)(s0 - pad) * W,
            (short)0, (int)(W == 4 ? nh * 4u : ((pad + nh + 1u) & ~1u) * 2u), kRsrcFlags);
        const int r = lane >> 4, s4 = 4 * (lane & 15);
        auto group_load = [&](int g, u4r &q, uint32_t &cnt) {
            const int b = h + 4 * g + r;  // this row's block (past `he`: none)
            const uint32_t ob = (uint32_t)__shfl((int)offv, b & 63);
            const uint32_t cb = (uint32_t)__shfl((int)cnt_lane, b & 63);
            cnt = b < he ? (cb < 64u ? cb : 64u) : 0u;
            if constexpr (W == 4) {
                q = (uint32_t)s4 < cnt ? __builtin_amdgcn_raw_buffer_load_b128(rsy, (ob - s0 + s4) * 4u, 0, 0)
                                       : u4r{0u, 0u, 0u, 0u};
            } else {  // units s4..s4+3 = 2 dwords, from 3 aligned ones
                const uint32_t u = ob - s0 + pad + (uint32_t)s4, odd = u & 1u;
                uint32_t d[3] = {0u, 0u, 0u};
                if ((uint32_t)s4 < cnt) {
                    const auto t = __builtin_amdgcn_raw_buffer_load_b96(rsy, (u & ~1u) * 2u, 0, 0);
                    d[0] = t[0], d[1] = t[1], d[2] = t[2];
                }
                uint32_t a[2];
                align_units<2>(d, odd, a);
                q = u4r{widen16(a[0]), widen16(a[0] >> 16), widen16(a[1]), widen16(a[1] >> 16)};
            }
        };
        const int ng = (he - h + 3) >> 2;
        u4r q;
        uint32_t cnt;
        group_load(0, q, cnt);
        // vmcnt(0) before any LDS read into registers: the previous half's stores (store-data hazard)
        retire_stores();
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < 4 || lane < 32) reinterpret_cast<u4r *>(lt)[k * 64 + lane] = u4r{0u, 0u, 0u, 0u};
        wave_sync_lds();
        for (int g = 0; g < ng; ++g) {
            u4r nq;
            uint32_t ncnt;
            group_load(g + 1 < ng ? g + 1 : g, nq, ncnt);
            uint32_t p[4], run = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                run += (uint32_t)s4 + j < cnt ? (q[j] >> 16) + 1u : 0u;
                p[j] = run;
            }
            uint32_t incl = run;  // row-segmented inclusive scan of the lane totals
            incl += __builtin_amdgcn_update_dpp(0u, incl, 0x111, 0xF, 0xF, false);  // row_shr:1
            incl += __builtin_amdgcn_update_dpp(0u, incl, 0x112, 0xF, 0xF, false);  // row_shr:2
            incl += __builtin_amdgcn_update_dpp(0u, incl, 0x114, 0xF, 0xF, false);  // row_shr:4
            incl += __builtin_amdgcn_update_dpp(0u, incl, 0x118, 0xF, 0xF, false);  // row_shr:8
            const uint32_t before = incl - run;
            char *row = lt + (4 * g + r) * kDecPitch;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t pos = before + p[j] - 1u;
                const bool put = (uint32_t)s4 + j < cnt && pos < 64u;
                const uint32_t at = put ? 2u * zz[pos < 64u ? pos : 63u] : 128u;  // 128: the padding
                *reinterpret_cast<int16_t *>(row + at) = (int16_t)(q[j] & 0xFFFFu);
            }
            q = nq;
            cnt = ncnt;
        }
    }
    return lane_path;
}

}  // namespace dctq
