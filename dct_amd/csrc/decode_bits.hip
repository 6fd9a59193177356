// dct_amd/csrc/decode_bits.hip -- dctq_decode_bits_planes: the bit-packed stream "bits v1"
// -> u8 pixels, for every block of up to 4 planes in ONE launch and with no coefficient in
// memory.  Bit for bit dctq_bits_decode followed by dctq_decode_planes, because it is both
// kernels' code: source = bits_to_coef's bit walk (bits_rebuild_half, bits_core.h), sink =
// decode8's inverse and pixel stores (pixel_rows_out, decode_core.h), in the decoders' one
// tile loop (tile_decode_core.h, which also states the store-data hazard rule) --
// symbols_to_pixels (decode_symbols.hip) with the packed bytes in the symbols' place.
//
// P + 4 B in + 64 B out per block (P = the block's packed bytes; + 4 B of var_num, adaptive
// plans) against P + 4 + 128 + 128 + 64 B of the two launches.
#include "bits_core.h"
#include "decode_core.h"
#include "tile_decode_core.h"

namespace dctq {

constexpr int kBitsPixGridMult = 64;  // as symbols_to_pixels: about one tile per wave

template <bool ADAPTIVE, bool INV32>
__global__ __launch_bounds__(kThreadsP, 4) void bits_to_pixels(SymbolSet ss, const uint8_t *__restrict__ bytes,
                                                               const uint32_t *__restrict__ offsets,
                                                               const DevTables *__restrict__ dev) {
    const uint32_t nblk = ss.blk_first[kMaxPlanes];
    decode_tiles<uint32_t, kWavesP, kBitsLds>(
        offsets, nblk, (nblk + 63u) >> 6,
        [&](auto... half) __attribute__((always_inline)) { return bits_rebuild_half(bytes, half...); },
        [&](auto... half) __attribute__((always_inline)) { pixel_rows_out<ADAPTIVE, INV32>(ss, dev, half...); });
}

hipError_t launch_decode_bits(const SymbolSet &ss, const uint8_t *bytes, const uint32_t *offsets, const DevTables *dev,
                              int adaptive, bool inv_f32, hipStream_t stream, int num_cus) {
    const uint64_t ntiles = ((uint64_t)ss.blk_first[kMaxPlanes] + 63) / 64;
    return with_inverse(
        [&](auto a, auto f32) {
            return launch_persistent<bits_to_pixels<a, f32>, kThreadsP, kWavesP, kBitsPixGridMult>(
                ntiles, num_cus, stream, ss, bytes, offsets, dev);
        },
        adaptive != 0, inv_f32);
}

}  // namespace dctq
