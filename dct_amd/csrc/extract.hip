// dct_amd/csrc/extract.hip -- dctq_bits_window_offsets and dctq_bits_window_gather: a window of
// a "bits v1" stream as a stream of its own, without decoding.  Nothing in
// bits v1 couples one block to another, so the window's stream is the sub-sequence of the
// stored stream's blocks, in the numbering of the window's own picture (plane by plane, then
// frames, block rows, block columns; tools/extract_ref.py states it in plain numpy).
//
//   offsets: one wave per 64-block tile of the DESTINATION numbering.  Lane d finds its stored
//            block (plane select chain, fdiv by the window's width and rows), takes its length
//            from two entries of `offsets` (exact, mod 2^32: no 368 clamp) and gathers its
//            var_num; the wave scan gives the tile-local offsets and the tile total; then the
//            tile scan and fix-up of rle.hip, as bits.hip and frame.hip use them.
//   gather:  one wave per run (window_core.h).  A run's source bytes [offsets[s0], offsets[s0 +
//            nb)) are contiguous and so is its destination from win_offsets[d0], so a run is one
//            byte copy at independent source and destination alignment.  Whole destination-
//            aligned dwords leave as coalesced dword stores, each assembled (v_alignbyte) from
//            the two aligned source dwords that hold its bytes, kGatherRounds of them in flight
//            per lane.  The up to three bytes before the first whole destination dword and
//            after the last one are byte stores: the neighbouring runs are other waves' work,
//            and no two waves store to one dword.  An aligned source dword that is not wholly
//            inside the run (at most one at each end) is never loaded: the destination dword
//            that needs it is assembled from byte loads by a lane of its own.  So nothing
//            outside [offsets[s0], offsets[s0 + nb)) is read and nothing outside
//            [win_offsets[d0], min(win_offsets[d0 + nb], capacity)) is written, for any offsets.
//            Addresses are 64-bit pointers plus unsigned byte offsets: an offset with bit 31 set
//            is ordinary.
//
// No LDS is used by either kernel, so the store-data hazard of DESIGN.md 3.1 (tile_decode_core.h)
// does not arise: no LDS read follows a store.
#include "scan_core.h"
#include "window_core.h"

namespace dctq {

constexpr int kExtractWaves = 4;
constexpr int kExtractThreads = 64 * kExtractWaves;
constexpr int kExtractGridMult = 64;  // as the bits kernels: about one tile or run per wave on large inputs
constexpr int kGatherRounds = 4;      // destination dwords per lane and round: 4 or 8 loads in flight

// The destination numbering: each plane's first block in the window's own concatenated
// numbering; first[n..] = the window's blocks (< 2^26).
struct WindowBlocks {
    uint32_t first[kMaxPlanes + 1];
};

// Field `get(i)` of plane k (k may differ by lane): a select chain, no indexed kernel-argument loads.
template <typename G>
__device__ __forceinline__ uint32_t of_plane(int k, G &&get) {
    uint32_t v = get(0);
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) v = k == i ? get(i) : v;
    return v;
}
template <typename G>
__device__ __forceinline__ FastDiv div_of_plane(int k, G &&get) {
    FastDiv f;
    f.d = of_plane(k, [&](int i) { return get(i).d; });
    f.m = of_plane(k, [&](int i) { return get(i).m; });
    f.s = of_plane(k, [&](int i) { return get(i).s; });
    return f;
}

// ---- offsets: win_offsets[d] = bytes of the tile's blocks before d; tiles[t] = the tile's bytes
template <bool VAR>
__global__ __launch_bounds__(kExtractThreads) void window_lengths_kernel(WindowSet ws, WindowBlocks wb,
                                                                         const uint32_t *__restrict__ offsets,
                                                                         uint32_t *__restrict__ win_offsets,
                                                                         int32_t *__restrict__ win_var,
                                                                         uint32_t *__restrict__ tiles, uint32_t ntiles) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nblk = wb.first[kMaxPlanes];
    const uint32_t stride = gridDim.x * kExtractWaves;
    for (uint32_t t = blockIdx.x * kExtractWaves + wv; t < ntiles; t += stride) {
        const uint32_t d = t * 64u + (uint32_t)lane;
        const bool valid = d < nblk;
        const uint32_t dd = valid ? d : nblk - 1u;  // past the end: the last block, computed and not stored
        // destination block dd -> plane k, window row q (over the window's frames), column x
        int k = 0;
#pragma unroll
        for (int i = 1; i < kMaxPlanes; ++i) k += dd >= wb.first[i] ? 1 : 0;
        const uint32_t dk = dd - of_plane(k, [&](int i) { return wb.first[i]; });
        const uint32_t wbw = of_plane(k, [&](int i) { return (uint32_t)ws.pl[i].bw; });
        const uint32_t rows = of_plane(k, [&](int i) { return ws.win[i].rows; });
        const uint32_t q = fdiv(dk, div_of_plane(k, [&](int i) { return ws.pl[i].div_bw; })), x = dk - q * wbw;
        const uint32_t f = fdiv(q, div_of_plane(k, [&](int i) { return ws.win[i].div_rows; })), y = q - f * rows;
        // behind the window's first block by f frames, y rows and x blocks of the STORED plane
        const uint32_t rel = f * of_plane(k, [&](int i) { return ws.win[i].nblk_frame; }) +
                             y * of_plane(k, [&](int i) { return ws.win[i].bw; }) + x;
        const uint32_t s = of_plane(k, [&](int i) { return ws.win[i].first; }) + rel;
        uint32_t len = offsets[s + 1u] - offsets[s];
        len = valid ? len : 0u;
        if constexpr (VAR) {
            const int32_t vn = var_of(ws, (uint32_t)k)[of_plane(k, [&](int i) { return ws.win[i].var_first; }) + rel];
            if (valid) win_var[d] = vn;
        }
        const uint32_t inc = wave_inclusive_scan(len);
        if (valid) win_offsets[d] = inc - len;
        if (lane == 63) tiles[t] = inc;
    }
}

// ---- gather: win_bytes[win_offsets[d] .. win_offsets[d + 1]) of every block; nothing at or past `capacity`
//
// One destination dword of a run whose aligned source dwords are whole inside the run:
// SHIFT false: source and destination agree mod 4, one load; true: two loads and v_alignbyte.
template <bool SHIFT>
__device__ __forceinline__ void gather_dwords(const uint32_t *__restrict__ sw, uint32_t *__restrict__ dw, uint32_t lo,
                                              uint32_t hi, uint32_t sh, int lane) {
    for (uint32_t i0 = lo; i0 < hi; i0 += 64u * kGatherRounds) {
        uint32_t w0[kGatherRounds], w1[kGatherRounds];
#pragma unroll
        for (int j = 0; j < kGatherRounds; ++j) {
            const uint32_t i = i0 + 64u * j + (uint32_t)lane;
            const uint32_t ii = i < hi ? i : lo;  // past the end: a dword of the run, loaded and not stored
            w0[j] = sw[ii];
            if constexpr (SHIFT) w1[j] = sw[(unsigned long long)ii + 1ull];
        }
#pragma unroll
        for (int j = 0; j < kGatherRounds; ++j) {
            const uint32_t i = i0 + 64u * j + (uint32_t)lane;
            if (i < hi) dw[i] = SHIFT ? __builtin_amdgcn_alignbyte(w1[j], w0[j], sh) : w0[j];
        }
    }
}

__global__ __launch_bounds__(kExtractThreads) void window_gather_kernel(WindowSet ws, WindowBlocks wb,
                                                                        const uint8_t *__restrict__ bytes,
                                                                        const uint32_t *__restrict__ offsets,
                                                                        const uint32_t *__restrict__ win_offsets,
                                                                        uint8_t *__restrict__ win_bytes,
                                                                        unsigned long long capacity) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for_window_runs<kExtractWaves>(
        ws, offsets, lane, wv,
        [&](int k, uint32_t q, uint32_t, uint32_t, uint32_t j, uint32_t, int nb, uint32_t offv, uint32_t oend) {
            // the run's first block in the window's own numbering, its source and destination ranges
            const uint32_t d0 = of_plane(k, [&](int i) { return wb.first[i]; }) + q * (uint32_t)ws.pl[k].bw + 64u * j;
            const uint32_t a = __builtin_amdgcn_readfirstlane(offv), e = __builtin_amdgcn_readfirstlane(oend);
            const uint32_t D = __builtin_amdgcn_readfirstlane(win_offsets[d0]);
            const uint32_t Dend = __builtin_amdgcn_readfirstlane(win_offsets[d0 + (uint32_t)nb]);
            const uint32_t slen = e >= a ? e - a : 0u;  // bytes that may be read
            uint32_t len = Dend >= D ? Dend - D : 0u;   // bytes that may be written, ...
            len = len < slen ? len : slen;
            if (capacity <= D) return;
            const unsigned long long room = capacity - D;  // ... below capacity
            len = room < len ? (uint32_t)room : len;
            const uint8_t *src = bytes + (unsigned long long)a;
            uint8_t *dst = win_bytes + (unsigned long long)D;
            // [0, head) bytes, [head, head + 4 nd) whole destination dwords, then `tail` bytes
            const uint32_t lead = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & 3u;
            const uint32_t head = lead < len ? lead : len;
            const uint32_t nd = (len - head) >> 2, tail = (len - head) & 3u;
            // destination dword i holds source bytes [head + 4 i, head + 4 i + 4): bytes sh .. sh + 3
            // of aligned source dwords i and i + 1 counted from sw, which starts at byte head - sh
            const uint32_t sh = (uint32_t)(uintptr_t)(src + head) & 3u;
            const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - sh);
            uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
            // dwords [lo, hi): both source dwords lie in [0, slen) of the run.  Dword 0 does not when
            // sw starts before the run; at the end, dword i needs bytes below head - sh + 4 i + need
            const uint32_t lo = head < sh ? 1u : 0u, need = sh ? 8u : 4u;
            const long long most = ((long long)slen - (long long)need - (long long)head + (long long)sh) >> 2;  // floor
            uint32_t hi = most < 0 ? 0u : (most + 1 < (long long)nd ? (uint32_t)(most + 1) : nd);
            hi = hi < lo ? lo : hi;
            if (sh) gather_dwords<true>(sw, dw, lo, hi, sh, lane);
            else gather_dwords<false>(sw, dw, lo, hi, sh, lane);
            // the dwords left out (at most dword 0 and the last one), each from four byte loads
            // inside the run by one lane; the head and tail bytes by lanes of their own
            if (lane >= 8 && lane < 12) {
                const uint32_t i = lane == 8 ? 0u : hi + (uint32_t)(lane - 9);
                if (lane == 8 ? (lo != 0u && nd != 0u) : i < nd) {
                    const uint8_t *s = src + head + 4ull * i;
                    dw[i] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
                }
            } else if (lane < 3) {
                if ((uint32_t)lane < head) dst[lane] = src[lane];
            } else if (lane >= 4 && lane < 7) {
                const unsigned long long at = (unsigned long long)head + 4ull * nd + (unsigned long long)(lane - 4);
                if ((uint32_t)(lane - 4) < tail) dst[at] = src[at];
            }
        });
}

hipError_t launch_bits_window_offsets(const WindowSet &ws, const uint32_t *offsets, uint32_t *win_offsets,
                                      int32_t *win_var, void *wsp, hipStream_t stream, int num_cus) {
    WindowBlocks wb;
    uint32_t next = 0;
    for (int k = 0; k <= kMaxPlanes; ++k) {
        wb.first[k] = next;
        if (k < ws.n) next += (uint32_t)ws.pl[k].nblk;
    }
    const uint32_t nblk = wb.first[kMaxPlanes], ntiles = (nblk + 63u) / 64u;
    hipError_t e = with_bools(
        [&](auto var) {
            return launch_persistent<window_lengths_kernel<decltype(var)::value>, kExtractThreads, kExtractWaves,
                                     kExtractGridMult>((uint64_t)ntiles, num_cus, stream, ws, wb, offsets, win_offsets,
                                                       win_var, (uint32_t *)wsp, ntiles);
        },
        win_var != nullptr);
    if (e != hipSuccess) return e;
    if ((e = launch_rle_scan(wsp, ntiles, stream)) != hipSuccess) return e;
    return launch_rle_fixup(win_offsets, nblk, wsp, ntiles, 0, win_offsets + nblk, stream);
}

hipError_t launch_bits_window_gather(const WindowSet &ws, const uint8_t *bytes, const uint32_t *offsets,
                                     const uint32_t *win_offsets, uint8_t *win_bytes, unsigned long long capacity,
                                     hipStream_t stream, int num_cus) {
    WindowBlocks wb;
    uint32_t next = 0;
    for (int k = 0; k <= kMaxPlanes; ++k) {
        wb.first[k] = next;
        if (k < ws.n) next += (uint32_t)ws.pl[k].nblk;
    }
    return launch_persistent<window_gather_kernel, kExtractThreads, kExtractWaves, kExtractGridMult>(
        (uint64_t)ws.run_first[kMaxPlanes], num_cus, stream, ws, wb, bytes, offsets, win_offsets, win_bytes, capacity);
}

}  // namespace dctq
