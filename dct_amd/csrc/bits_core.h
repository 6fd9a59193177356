// dct_amd/csrc/bits_core.h -- the bit-packed coefficient stream "bits v1" (include/dct_amd.h,
// DESIGN.md 3.13; stated in plain Python in tools/bits_ref.py): the code itself, and the
// decoders' half tile -- 32 blocks of a packed stream rebuilt as natural-order int16 rows in
// a wave's LDS.  Shared by the packer and bits_to_coef (bits.hip: the rows leave as
// coefficients) and bits_to_pixels (decode_bits.hip: the rows go into the inverse DCT).
//
//   ue(k), k >= 0: x = k + 1 of bit length n -> n - 1 zero bits, then x in n bits: x itself
//                  in a field of 2n - 1 bits (Exp-Golomb of order 0).
//   symbol (v, r): ue(min(r, 64)), ue(m), m = 2v - 1 for v > 0, else -2v; at most 13 + 33 bits.
//   block:         its first 64 symbols at most, MSB first, from a byte boundary, the last
//                  byte padded with zero bits.
#pragma once
#include "rle_decode_core.h"

namespace dctq {

constexpr uint32_t kBitsMaxSymbols = 64;  // symbols of a block that are written, and that are read
constexpr uint32_t kBitsMaxPrefix = 16;   // zero bits in front of a code; more is a bad code
constexpr uint32_t kBitsBlockMax = 368;   // 64 x 46 bits

// length of ue(k): 2n - 1, n = 32 - clz(k + 1)
__device__ __forceinline__ uint32_t ue_len(uint32_t k) { return 63u - 2u * (uint32_t)__builtin_clz(k + 1u); }
// the value's index m (0 -> 0, 1 -> 1, -1 -> 2, 2 -> 3, ...; -32768 -> 65536) and back, as int16 bits
__device__ __forceinline__ uint32_t value_code(int16_t v) {
    return v > 0 ? 2u * (uint32_t)v - 1u : 2u * (uint32_t)(-(int32_t)v);
}
__device__ __forceinline__ int16_t code_value(uint32_t m) {
    return (int16_t)(uint16_t)((m & 1u) ? (m + 1u) >> 1 : 0u - (m >> 1));
}

// f(value code m, clamped run r) for symbols [rel, rel + cnt) of the stream behind `rsy`
// (format W; a load at or past the descriptor's end reads 0), four loads in flight.  The
// whole wave calls it: cnt is per lane.
template <int W, typename F>
__device__ __forceinline__ void for_block_symbols(__amdgpu_buffer_rsrc_t rsy, uint32_t rel, uint32_t cnt, F &&f) {
    for (uint32_t i = 0; __builtin_amdgcn_ballot_w64(i < cnt); i += 4u) {
        uint32_t s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = 0u;
            if (i + j < cnt) {
                if constexpr (W == 4) s[j] = __builtin_amdgcn_raw_buffer_load_b32(rsy, (rel + i + j) * 4u, 0, 0);
                else s[j] = __builtin_amdgcn_raw_buffer_load_b16(rsy, (rel + i + j) * 2u, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < cnt) {
                const uint32_t r = sym_run<W>(s[j]);
                f(value_code(sym_value<W>(s[j])), r < 64u ? r : 64u);
            }
        }
    }
}

// ---- decode: one wave per 64-block tile, 32 blocks at a time, as rebuild_half.  The bit
// walk is serial inside a block, so lane i < 32 walks block h + i from LDS: the half's bytes
// come in as coalesced dword loads in chunks of whole blocks that fit kBitsStage (a smooth or
// noisy half is one chunk; a dense one takes several; a block that claims more than the
// stage is cut there, beyond the 528 B that 64 symbols of two 33-bit codes can span), and
// each value lands at zigzag[pos] of its row in the zeroed natural-order half tile (pitch
// kDecPitch: a value past position 63 goes to the row's padding, so placement is branch-free).
// No load leaves the chunk: whole dwords inside it go through a descriptor that ends on its
// last whole dword, and the up to three bytes in front of the first and after the last one
// are byte loads.  Every chunk's LDS work follows a vmcnt(0) (store-data hazard: the
// previous half's stores); no store is issued inside the half.
constexpr int kBitsStage = 2560;  // bytes; 10 dword loads per lane
constexpr int kBitsLds = kHalf * kDecPitch + kBitsStage;
static_assert(kBitsStage % 256 == 0 && kBitsStage - 3 >= 2 * 33 * 64 / 8, "whole load rounds; any block's useful bytes fit");

// bytes: the stream; offv: lane b holds offsets[64t + b] (lanes >= nb: the tile's end); oend:
// the tile's end.  Blocks [h, he) of the tile -> rows at lt + i * kDecPitch (the pitch is
// returned); the stage is the kBitsStage bytes behind the half tile.  A source of decode_tiles
// (tile_decode_core.h), whose per-lane block lengths it does not need.  END: the walk of a
// block stops once its position has reached END; positions only increase, so every value at a
// zigzag position below END is what the full walk (END = 64, every full-size decoder) places
// there, and the rows hold nothing a caller may rely on at or beyond it (decode_scaled.hip).
template <uint32_t END = 64u>
__device__ __forceinline__ int bits_rebuild_half(const uint8_t *__restrict__ bytes, uint32_t offv, uint32_t oend,
                                                 uint32_t /* cnt_lane */, int h, int he, int lane, char *lt,
                                                 const uint8_t (*zz)[64]) {
    uint8_t *lst = reinterpret_cast<uint8_t *>(lt + kHalf * kDecPitch);
    const int n = he - h;
    const uint32_t my_off = (uint32_t)__shfl((int)offv, (lane + h) & 63);
    const uint32_t nx_off = (uint32_t)__shfl((int)offv, (lane + h + 1) & 63);
    const uint32_t my_end = lane + h + 1 < 64 ? nx_off : oend;
    char *row = lt + (lane & 31) * kDecPitch;
    for (int s = 0; s < n;) {
        const uint32_t c0 = __builtin_amdgcn_readlane(offv, h + s);
        const unsigned long long addr = (unsigned long long)bytes + c0;
        const uint32_t pad = (uint32_t)(addr & 3ull), room = (uint32_t)kBitsStage - pad;
        // the chunk: blocks [s, e) end inside the stage (the first block always belongs)
        const uint64_t over = __builtin_amdgcn_ballot_w64(lane >= s && (lane >= n || my_end - c0 > room));
        int e = over ? (int)__builtin_ctzll(over) : n;
        uint32_t clen = off_at(offv, oend, h + e) - c0;
        if (e == s) e = s + 1, clen = room;
        const uint32_t left = oend >= c0 ? oend - c0 : 0u;  // never past the tile
        clen = clen < left ? clen : left;
        clen = clen < room ? clen : room;
        const uint32_t end = pad + clen, lo4 = pad ? 4u : 0u, hi4 = end & ~3u;
        char *base = reinterpret_cast<char *>(addr - pad);
        const __amdgpu_buffer_rsrc_t rdw = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)hi4, kRsrcFlags);
        const __amdgpu_buffer_rsrc_t rby = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)end, kRsrcFlags);
        uint32_t v[kBitsStage / 256];
#pragma unroll
        for (int j = 0; j < kBitsStage / 256; ++j) {
            const uint32_t d = (uint32_t)(j * 64 + lane) * 4u;
            v[j] = (uint32_t)j * 256u < end && d >= lo4 ? __builtin_amdgcn_raw_buffer_load_b32(rdw, d, 0, 0) : 0u;
        }
        // the bytes in front of the first whole dword (lanes 0..3) and after the last (4..7)
        const uint32_t edge = lane < 4 ? pad + (uint32_t)lane : (hi4 > lo4 ? hi4 : lo4) + (uint32_t)(lane - 4);
        const bool has_edge = lane < 8 && edge < end && (lane >= 4 || edge < lo4);
        const uint32_t eb = has_edge ? __builtin_amdgcn_raw_buffer_load_b8(rby, edge, 0, 0) : 0u;
        // vmcnt(0): these loads, and the previous half's stores before any LDS read (store-data hazard)
        retire_stores();
#pragma unroll
        for (int j = 0; j < kBitsStage / 256; ++j)
            if ((uint32_t)j * 256u < end) reinterpret_cast<uint32_t *>(lst)[j * 64 + lane] = v[j];
        if (has_edge) lst[edge] = (uint8_t)eb;
        if (s == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k < 4 || lane < 32) reinterpret_cast<u4r *>(lt)[k * 64 + lane] = u4r{0u, 0u, 0u, 0u};
        }
        wave_sync_lds();
        if (lane >= s && lane < e) {
            // the block's bytes, inside the chunk for any offsets
            const uint32_t start = my_off - c0;
            const uint32_t want = my_end >= my_off ? my_end - my_off : 0u;
            const uint32_t len = start <= clen ? (want < clen - start ? want : clen - start) : 0u;
            uint32_t bp = pad + start;
            const uint32_t bend = bp + len;
            uint64_t win = 0ull;  // the next `have` bits, from bit 63 down; zeros below them
            uint32_t have = 0u, pos = 0u;
            // k of the next code; false: a bad code (prefix too long, or bits past the block's end)
            auto get = [&](uint32_t &k) {
                while (have <= 56u && bp < bend) {
                    win |= (uint64_t)lst[bp++] << (56u - have);
                    have += 8u;
                }
                const uint32_t z = win ? (uint32_t)__builtin_clzll(win) : 64u;
                const uint32_t bits = 2u * z + 1u;
                if (z > kBitsMaxPrefix || bits > have) return false;
                k = (uint32_t)(win >> (64u - bits)) - 1u;
                win <<= bits;
                have -= bits;
                return true;
            };
            for (uint32_t i = 0; i < kBitsMaxSymbols && pos < END; ++i) {
                uint32_t r, m;
                if (!get(r) || !get(m)) break;
                pos += r;
                const uint32_t at = pos < 64u ? 2u * (*zz)[pos] : 128u;  // 128: the padding
                *reinterpret_cast<int16_t *>(row + at) = code_value(m);
                pos += 1u;
            }
        }
        wave_sync_lds();  // the walk is done before the next chunk overwrites the stage
        s = e;
    }
    return kDecPitch;
}

}  // namespace dctq
