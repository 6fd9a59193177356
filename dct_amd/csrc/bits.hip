// dct_amd/csrc/bits.hip -- dctq_bits_pack and dctq_bits_decode: the run-length symbols of
// the encoder as the bit-packed stream "bits v1" (bits_core.h), and back to
// coefficients.
//
//   dctq_bits_pack  : count (lane-per-block byte lengths, wave-scanned per 64-block tile),
//                     the tile scan and fix-up of the symbol offsets (rle.hip), then emit.
//   dctq_bits_decode: the decoders' tile loop (tile_decode_core.h) over bits_rebuild_half,
//                     rows out as 1 KiB stores.
//
// A block's bits are serial, so both directions work lane-per-block; what the wave shares
// is the memory side.  Emit: lane b packs block b into an LDS copy of the tile's bytes (the
// tile's bytes are contiguous in the stream), which leaves as coalesced dword stores; the
// first and last dword of a tile can be shared with its neighbours, so the bytes of the tile
// in them are byte stores.  A tile whose bytes exceed the stage (dense content at the
// finest quantizers) stores its bytes from the lanes directly.
#include "bits_core.h"
#include "scan_core.h"
#include "tile_decode_core.h"

namespace dctq {

constexpr int kBitsWaves = 4;
constexpr int kBitsThreads = 64 * kBitsWaves;
constexpr int kBitsGridMult = 64;       // as the symbol decoders: about one tile per wave on large inputs
constexpr int kPackStage = 8192;        // bytes of a tile the emit stages per wave (128 B per block)
constexpr int kPackRound = 8;           // dwords per lane and store round

// The tile's symbols behind one descriptor: a lane reads inside the tile for any offsets.
template <int W>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_symbols(const void *symbols, uint32_t s0, uint32_t send) {
    const unsigned long long nbytes = (unsigned long long)(send - s0) * W;
    return __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(reinterpret_cast<const char *>(symbols)) + (unsigned long long)s0 * W, (short)0,
        (int)(send >= s0 ? (nbytes < 0x7FFFFFFFull ? nbytes : 0x7FFFFFFFull) : 0ull), kRsrcFlags);
}

// lane b < nb: block 64t + b's first symbol from the tile's, and its count (at most 64, inside the tile)
struct TileSymbols {
    uint32_t s0, rel, cnt;
};
__device__ __forceinline__ TileSymbols tile_symbol_ranges(const uint32_t *__restrict__ sym_offsets, long long b0,
                                                          int nb, int lane) {
    const uint32_t soff = sym_offsets[b0 + (lane < nb ? lane : nb)];
    const uint32_t snext = sym_offsets[b0 + (lane < nb ? lane + 1 : nb)];
    TileSymbols r;
    r.s0 = __builtin_amdgcn_readfirstlane(soff);
    const uint32_t c = snext >= soff ? snext - soff : 0u;
    r.rel = soff - r.s0;
    r.cnt = lane < nb && soff >= r.s0 ? (c < kBitsMaxSymbols ? c : kBitsMaxSymbols) : 0u;
    return r;
}

// ---- count: offsets[b] = bytes of the tile's blocks before b; tiles[t] = the tile's bytes
template <int W>
__global__ __launch_bounds__(kBitsThreads) void bits_count_kernel(const void *__restrict__ symbols,
                                                                  const uint32_t *__restrict__ sym_offsets,
                                                                  long long nblk, uint32_t *__restrict__ offsets,
                                                                  uint32_t *__restrict__ tiles, long long ntiles) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * kBitsWaves;
    for (long long t = (long long)blockIdx.x * kBitsWaves + wv; t < ntiles; t += stride) {
        const long long b0 = t * 64;
        const int nb = tile_blocks(t, nblk);
        const TileSymbols ts = tile_symbol_ranges(sym_offsets, b0, nb, lane);
        const uint32_t send = sym_offsets[b0 + nb];
        const __amdgpu_buffer_rsrc_t rsy = tile_symbols<W>(symbols, ts.s0, send);
        uint32_t bits = 0;
        for_block_symbols<W>(rsy, ts.rel, ts.cnt, [&](uint32_t m, uint32_t r) { bits += ue_len(r) + ue_len(m); });
        const uint32_t nbytes = (bits + 7u) >> 3;
        const uint32_t inc = wave_inclusive_scan(nbytes);
        if (lane < nb) offsets[b0 + lane] = inc - nbytes;
        if (lane == 63) tiles[t] = inc;
    }
}

// Lane-per-block: the block's symbols as bytes, put(i, byte) for byte i of the block.
template <int W, typename P>
__device__ __forceinline__ void pack_block(__amdgpu_buffer_rsrc_t rsy, const TileSymbols &ts, P &&put) {
    uint64_t acc = 0;  // the low nbit bits: not yet written
    uint32_t nbit = 0, at = 0;
    for_block_symbols<W>(rsy, ts.rel, ts.cnt, [&](uint32_t m, uint32_t r) {
        // x = k + 1 in a field of ue_len(k) bits is ue(k); 7 + 13 + 33 bits at most
        acc = (((acc << ue_len(r)) | (r + 1u)) << ue_len(m)) | (m + 1u);
        nbit += ue_len(r) + ue_len(m);
        while (nbit >= 8u) {
            nbit -= 8u;
            put(at++, (uint32_t)(acc >> nbit) & 0xFFu);
        }
    });
    if (nbit) put(at, (uint32_t)(acc << (8u - nbit)) & 0xFFu);
}

// ---- emit: bytes[offsets[b] .. offsets[b+1]) of every block; nothing at or past `capacity`
template <int W>
__global__ __launch_bounds__(kBitsThreads) void bits_emit_kernel(const void *__restrict__ symbols,
                                                                 const uint32_t *__restrict__ sym_offsets,
                                                                 long long nblk, const uint32_t *__restrict__ offsets,
                                                                 uint8_t *__restrict__ bytes, long long ntiles,
                                                                 unsigned long long capacity) {
    __shared__ uint32_t stage[kBitsWaves][kPackStage / 4];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * kBitsWaves;
    uint8_t *ls = reinterpret_cast<uint8_t *>(stage[wv]);
    for (long long t = (long long)blockIdx.x * kBitsWaves + wv; t < ntiles; t += stride) {
        const long long b0 = t * 64;
        const int nb = tile_blocks(t, nblk);
        const TileSymbols ts = tile_symbol_ranges(sym_offsets, b0, nb, lane);
        const uint32_t send = sym_offsets[b0 + nb];
        const __amdgpu_buffer_rsrc_t rsy = tile_symbols<W>(symbols, ts.s0, send);
        const uint32_t boff = offsets[b0 + (lane < nb ? lane : nb)];
        const uint32_t t0 = __builtin_amdgcn_readfirstlane(boff);
        const uint32_t tbytes = __builtin_amdgcn_readfirstlane(offsets[b0 + nb]) - t0;
        const uint32_t pad = t0 & 3u;  // bytes is 4-byte aligned: the tile is staged from its first dword
        if (capacity <= t0) continue;
        const unsigned long long room = capacity - t0;
        const uint32_t tlen = (uint32_t)(room < tbytes ? room : tbytes);  // the tile's bytes below capacity
        if (pad + tbytes > (uint32_t)kPackStage) {
            // dense tile: every lane stores its block's bytes itself
            const __amdgpu_buffer_rsrc_t rby = __builtin_amdgcn_make_buffer_rsrc(bytes + t0, (short)0, (int)tlen, kRsrcFlags);
            const uint32_t rel = boff - t0;
            pack_block<W>(rsy, ts, [&](uint32_t i, uint32_t byte) {
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)byte, rby, rel + i, 0, 0);
            });
            continue;
        }
        // LDS byte i is byte i of the stream from the dword that holds the tile's first byte
        const uint32_t rel = pad + boff - t0;
        pack_block<W>(rsy, ts, [&](uint32_t i, uint32_t byte) {
            if (rel + i < (uint32_t)kPackStage) ls[rel + i] = (uint8_t)byte;
        });
        wave_sync_lds();
        // whole dwords [lo4, hi4) as dwords; the bytes before and after them, which share
        // their dword with the neighbour tile (or are cut by capacity), as bytes
        const uint32_t end = pad + tlen, lo4 = pad ? 4u : 0u, hi4 = end & ~3u;
        uint8_t *base = bytes + (t0 - pad);
        const __amdgpu_buffer_rsrc_t rdw = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)hi4, kRsrcFlags);
        const __amdgpu_buffer_rsrc_t rby = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)end, kRsrcFlags);
        const uint32_t edge = lane < 4 ? pad + (uint32_t)lane : (hi4 > lo4 ? hi4 : lo4) + (uint32_t)(lane - 4);
        const bool has_edge = lane < 8 && edge < end && (lane >= 4 || edge < lo4);
        // vmcnt(0) before every round's LDS reads: the stores of the round (or tile) before (store-data hazard)
        retire_stores();
        const uint32_t eb = has_edge ? ls[edge] : 0u;
        for (uint32_t d0 = 0; d0 * 4u < hi4; d0 += 64u * kPackRound) {
            retire_stores();
            uint32_t v[kPackRound];
#pragma unroll
            for (int j = 0; j < kPackRound; ++j) v[j] = stage[wv][d0 + j * 64 + lane];
#pragma unroll
            for (int j = 0; j < kPackRound; ++j) {
                const uint32_t d = (d0 + j * 64 + lane) * 4u;
                if (d >= lo4) __builtin_amdgcn_raw_buffer_store_b32(v[j], rdw, d, 0, 0);  // past hi4: dropped
            }
        }
        if (has_edge) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)eb, rby, edge, 0, 0);
        wave_sync_lds();  // the stage is read out before the next tile packs into it
    }
}

// ---- decode to coefficients: source = the packed bytes (bits_rebuild_half), sink = int16 rows
// as 1 KiB stores; the loop, the sink and the hazard rule: tile_decode_core.h
__global__ __launch_bounds__(kBitsThreads) void bits_to_coef(const uint8_t *__restrict__ bytes,
                                                             const uint32_t *__restrict__ offsets, long long nblk,
                                                             int16_t *__restrict__ coef, long long ntiles) {
    decode_tiles<long long, kBitsWaves, kBitsLds>(
        offsets, nblk, ntiles,
        [&](auto... half) __attribute__((always_inline)) { return bits_rebuild_half(bytes, half...); },
        [&](auto... half) __attribute__((always_inline)) { coef_rows_out<true>(coef, half...); });
}

hipError_t launch_bits_pack(const void *symbols, int symbol_bytes, const uint32_t *sym_offsets, long long nblk,
                            uint32_t *offsets, uint8_t *bytes, unsigned long long capacity, void *ws,
                            hipStream_t stream, int num_cus) {
    const long long ntiles = (nblk + 63) / 64;
    uint32_t *tiles = (uint32_t *)ws;
    hipError_t e = with_bools(
        [&](auto w2) {
            return launch_persistent<bits_count_kernel<(decltype(w2)::value ? 2 : 4)>, kBitsThreads, kBitsWaves,
                                     kBitsGridMult>((uint64_t)ntiles, num_cus, stream, symbols, sym_offsets, nblk,
                                                    offsets, tiles, ntiles);
        },
        symbol_bytes == 2);
    if (e != hipSuccess) return e;
    if ((e = launch_rle_scan(ws, ntiles, stream)) != hipSuccess) return e;
    if ((e = launch_rle_fixup(offsets, nblk, ws, ntiles, 0, offsets + nblk, stream)) != hipSuccess) return e;
    if (!bytes || !capacity) return hipSuccess;
    return with_bools(
        [&](auto w2) {
            return launch_persistent<bits_emit_kernel<(decltype(w2)::value ? 2 : 4)>, kBitsThreads, kBitsWaves,
                                     kBitsGridMult>((uint64_t)ntiles, num_cus, stream, symbols, sym_offsets, nblk,
                                                    (const uint32_t *)offsets, bytes, ntiles, capacity);
        },
        symbol_bytes == 2);
}

hipError_t launch_bits_decode(const uint8_t *bytes, const uint32_t *offsets, long long nblk, int16_t *coef,
                              hipStream_t stream, int num_cus) {
    const long long ntiles = (nblk + 63) / 64;
    return launch_persistent<bits_to_coef, kBitsThreads, kBitsWaves, kBitsGridMult>((uint64_t)ntiles, num_cus, stream,
                                                                                  bytes, offsets, nblk, coef, ntiles);
}

}  // namespace dctq
