// dct_amd/csrc/decode_symbols.hip -- dctq_decode_symbols_planes: run-length symbols ->
// u8 pixels, for every block of up to 4 planes in ONE launch and with no coefficient in
// memory.  Bit for bit dctq_rle_decode (or dctq_rle_decode16) followed by
// dctq_decode_planes, because it is both kernels' code: source = rle_decode_kernel's
// (symbols_source over rebuild_half, pitch 144 B on every path), sink = decode8's inverse and
// pixel stores (pixel_rows_out, decode_core.h), in the decoders' one tile loop
// (tile_decode_core.h, which also states the store-data hazard rule).
//
// S + 4 B in + 64 B out per block (S = the block's symbols; + 4 B of var_num, adaptive
// plans) against S + 4 + 128 + 128 + 64 B of the two launches.
#include "decode_core.h"
#include "tile_decode_core.h"

namespace dctq {

// The grid (launch_persistent): up to 64 x the resident workgroups, as decode8: about one tile per wave.
constexpr int kSymGridMult = 64;
// 4.5 KiB half tile + 960 B of lane-path symbols per wave; 4 waves/SIMD (the inverse's registers) need 87 KiB per CU
constexpr int kSymLds = dec_lds_bytes(kDecPitch);

template <int W, bool ADAPTIVE, bool INV32>
__global__ __launch_bounds__(kThreadsP, 4) void symbols_to_pixels(SymbolSet ss, const void *__restrict__ symbols,
                                                                  const uint32_t *__restrict__ offsets,
                                                                  const DevTables *__restrict__ dev) {
    const uint32_t nblk = ss.blk_first[kMaxPlanes];
    decode_tiles<uint32_t, kWavesP, kSymLds>(
        offsets, nblk, (nblk + 63u) >> 6,
        [&](auto... half) __attribute__((always_inline)) { return symbols_source<W, kDecPitch>(symbols, half...); },
        [&](auto... half) __attribute__((always_inline)) { pixel_rows_out<ADAPTIVE, INV32>(ss, dev, half...); });
}

hipError_t launch_decode_symbols(const SymbolSet &ss, const void *symbols, int symbol_bytes, const uint32_t *offsets,
                                 const DevTables *dev, int adaptive, bool inv_f32, hipStream_t stream, int num_cus) {
    const uint64_t ntiles = ((uint64_t)ss.blk_first[kMaxPlanes] + 63) / 64;
    return with_bools(
        [&](auto w2) {
            return with_inverse(
                [&](auto a, auto f32) {
                    return launch_persistent<symbols_to_pixels<(decltype(w2)::value ? 2 : 4), a, f32>, kThreadsP,
                                             kWavesP, kSymGridMult>(ntiles, num_cus, stream, ss, symbols, offsets, dev);
                },
                adaptive != 0, inv_f32);
        },
        symbol_bytes == 2);
}

}  // namespace dctq
