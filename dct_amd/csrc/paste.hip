// dct_amd/csrc/paste.hip -- dctq_bits_paste_offsets and dctq_bits_paste_copy: a window of a
// "bits v1" stream replaced by another stream's blocks, without decoding.
// Nothing in bits v1 couples one block to another, so the stream of an edited picture is the
// stored stream with the window's blocks swapped for the patch's: block s of the result is the
// patch's block d when s lies in its plane's window (d: the block's number in the window's own
// picture, the numbering dctq_bits_window_offsets produces) and block s of the base otherwise
// (tools/paste_ref.py states it in plain numpy).  The inverse direction of extract.hip.
//
//   offsets: one wave per 64-block tile of the DESTINATION numbering, which is the stored one.
//            Lane s finds its plane (select chain), its frame, row and column (fdiv by the stored
//            plane's blocks per frame and per row), tests them against the window, and takes its
//            length from two entries of the base's or the patch's offsets (exact, mod 2^32: no
//            368 clamp) and its var_num from the matching array; the wave scan gives the
//            tile-local offsets and the tile total; then the tile scan and fix-up of rle.hip.
//   copy:    one wave per 64-block destination tile, whose bytes [out_offsets[t0], out_offsets[t0
//            + nb)) are contiguous.  Each lane computes its source (base or patch) and source
//            block; a ballot of "the source changes, or the source block is not the previous
//            lane's plus one" splits the tile into segments that are contiguous in source and
//            destination, and the wave copies them one after another (a wave-uniform loop of at
//            most 64 rounds; a tile outside every window is one segment).  A segment is the byte
//            copy of extract.hip's gather, in this file's own text: whole destination-aligned
//            dwords, each assembled (v_alignbyte) from the two aligned source dwords that hold
//            its bytes; the up to three bytes before the first and after the last whole dword as
//            byte stores, because the neighbouring tiles are other waves' work; an aligned source
//            dword that is not wholly inside the segment is never loaded.  So nothing outside a
//            segment's source bytes is read and nothing outside [out_offsets[t0],
//            min(out_offsets[t0 + nb], capacity)) is written, for any offsets.  Addresses are
//            64-bit pointers plus unsigned byte offsets: an offset with bit 31 set is ordinary.
//
// No LDS memory is used by either kernel (the neighbour lane's source comes through a lane
// shuffle), so the store-data hazard of DESIGN.md 3.1 does not arise.
#include "scan_core.h"

namespace dctq {

constexpr int kPasteWaves = 4;
constexpr int kPasteThreads = 64 * kPasteWaves;
constexpr int kPasteGridMult = 64;  // as extract.hip: about one tile per wave on large inputs
constexpr int kPasteRounds = 4;     // destination dwords per lane and round: 4 or 8 loads in flight

// Stored plane k and its window, in blocks.
struct PastePlane {
    uint32_t first;            // the stored plane's first block in the concatenated stored numbering
    uint32_t patch_first;      // the window's first block in the patch's concatenated numbering
    uint32_t bw, nblk_frame;   // the stored plane's blocks per row and per frame
    FastDiv div_bw, div_frame;
    uint32_t f0, y0, x0;       // the window's first frame, block row and block column
    uint32_t wf, wh, ww;       // the window's frames, block rows and block columns
};
struct PasteSet {
    PastePlane pl[kMaxPlanes];
    const int32_t *var[kMaxPlanes];     // the base's var_num per stored plane, or unused
    const int32_t *pvar[kMaxPlanes];    // the patch's var_num per plane, or unused
    uint32_t nblk;                      // stored blocks in all (< 2^26)
    int n;
};

// Field `get(i)` of plane k (k may differ by lane): a select chain, no indexed kernel-argument loads.
template <typename G>
__device__ __forceinline__ auto paste_pick(int k, G &&get) {
    auto v = get(0);
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) v = k == i ? get(i) : v;
    return v;
}
template <typename G>
__device__ __forceinline__ FastDiv paste_pick_div(int k, G &&get) {
    FastDiv f;
    f.d = paste_pick(k, [&](int i) { return get(i).d; });
    f.m = paste_pick(k, [&](int i) { return get(i).m; });
    f.s = paste_pick(k, [&](int i) { return get(i).s; });
    return f;
}

// Where destination (= stored) block s comes from.
struct PasteFrom {
    int k;          // its plane
    uint32_t sk;    // its number inside the stored plane
    bool patch;     // inside the plane's window
    uint32_t d;     // then: its number in the patch's concatenated numbering
};
__device__ __forceinline__ PasteFrom paste_from(const PasteSet &ps, uint32_t s) {
    PasteFrom r;
    r.k = 0;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) r.k += (i < ps.n && s >= ps.pl[i].first) ? 1 : 0;
    const int k = r.k;
    r.sk = s - paste_pick(k, [&](int i) { return ps.pl[i].first; });
    const uint32_t per = paste_pick(k, [&](int i) { return ps.pl[i].nblk_frame; });
    const uint32_t bw = paste_pick(k, [&](int i) { return ps.pl[i].bw; });
    const uint32_t f = fdiv(r.sk, paste_pick_div(k, [&](int i) { return ps.pl[i].div_frame; })), in_frame = r.sk - f * per;
    const uint32_t y = fdiv(in_frame, paste_pick_div(k, [&](int i) { return ps.pl[i].div_bw; })), x = in_frame - y * bw;
    // unsigned: a coordinate before the window's first wraps to a large number
    const uint32_t wf = f - paste_pick(k, [&](int i) { return ps.pl[i].f0; });
    const uint32_t wy = y - paste_pick(k, [&](int i) { return ps.pl[i].y0; });
    const uint32_t wx = x - paste_pick(k, [&](int i) { return ps.pl[i].x0; });
    const uint32_t wh = paste_pick(k, [&](int i) { return ps.pl[i].wh; });
    const uint32_t ww = paste_pick(k, [&](int i) { return ps.pl[i].ww; });
    r.patch = wf < paste_pick(k, [&](int i) { return ps.pl[i].wf; }) && wy < wh && wx < ww;
    r.d = paste_pick(k, [&](int i) { return ps.pl[i].patch_first; }) + (wf * wh + wy) * ww + wx;
    return r;
}
__device__ __forceinline__ const int32_t *paste_var(const int32_t *const (&v)[kMaxPlanes], int k) {
    const int32_t *p = v[0];
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) p = k == i ? v[i] : p;
    return p;
}

// ---- offsets: out_offsets[s] = bytes of the tile's blocks before s; tiles[t] = the tile's bytes
template <bool VAR>
__global__ __launch_bounds__(kPasteThreads) void paste_lengths_kernel(PasteSet ps, const uint32_t *__restrict__ offsets,
                                                                        const uint32_t *__restrict__ patch_offsets,
                                                                        uint32_t *__restrict__ out_offsets,
                                                                        int32_t *__restrict__ out_var,
                                                                        uint32_t *__restrict__ tiles, uint32_t ntiles) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nblk = ps.nblk;
    const uint32_t stride = gridDim.x * kPasteWaves;
    for (uint32_t t = blockIdx.x * kPasteWaves + wv; t < ntiles; t += stride) {
        const uint32_t s = t * 64u + (uint32_t)lane;
        const bool valid = s < nblk;
        const uint32_t ss = valid ? s : nblk - 1u;  // past the end: the last block, computed and not stored
        const PasteFrom from = paste_from(ps, ss);
        const uint32_t *src = from.patch ? patch_offsets : offsets;
        const uint32_t at = from.patch ? from.d : ss;
        uint32_t len = src[at + 1u] - src[at];
        len = valid ? len : 0u;
        if constexpr (VAR) {
            const int32_t *vp = from.patch ? paste_var(ps.pvar, from.k) : paste_var(ps.var, from.k);
            const uint32_t vi =
                from.patch ? from.d - paste_pick(from.k, [&](int i) { return ps.pl[i].patch_first; }) : from.sk;
            const int32_t vn = vp[vi];
            if (valid) out_var[s] = vn;
        }
        const uint32_t inc = wave_inclusive_scan(len);
        if (valid) out_offsets[s] = inc - len;
        if (lane == 63) tiles[t] = inc;
    }
}

// ---- copy: out_bytes[out_offsets[s] .. out_offsets[s + 1]) of every block; nothing at or past `capacity`
//
// One destination dword of a segment whose aligned source dwords are whole inside the segment:
// SHIFT false: source and destination agree mod 4, one load; true: two loads and v_alignbyte.
template <bool SHIFT>
__device__ __forceinline__ void paste_dwords(const uint32_t *__restrict__ sw, uint32_t *__restrict__ dw, uint32_t lo,
                                             uint32_t hi, uint32_t sh, int lane) {
    for (uint32_t i0 = lo; i0 < hi; i0 += 64u * kPasteRounds) {
        uint32_t w0[kPasteRounds], w1[kPasteRounds];
#pragma unroll
        for (int j = 0; j < kPasteRounds; ++j) {
            const uint32_t i = i0 + 64u * j + (uint32_t)lane;
            const uint32_t ii = i < hi ? i : lo;  // past the end: a dword of the segment, loaded and not stored
            w0[j] = sw[ii];
            if constexpr (SHIFT) w1[j] = sw[(unsigned long long)ii + 1ull];
        }
#pragma unroll
        for (int j = 0; j < kPasteRounds; ++j) {
            const uint32_t i = i0 + 64u * j + (uint32_t)lane;
            if (i < hi) dw[i] = SHIFT ? __builtin_amdgcn_alignbyte(w1[j], w0[j], sh) : w0[j];
        }
    }
}

// One segment: source bytes [a, e) of `from` to out_bytes from D, as far as Dend and capacity
// allow.  Every argument but lane is wave-uniform.
__device__ __forceinline__ void paste_segment(const uint8_t *__restrict__ from, uint32_t a, uint32_t e,
                                              uint8_t *__restrict__ out_bytes, uint32_t D, uint32_t Dend,
                                              unsigned long long capacity, int lane) {
    const uint32_t slen = e >= a ? e - a : 0u;  // bytes that may be read
    uint32_t len = Dend >= D ? Dend - D : 0u;   // bytes that may be written, ...
    len = len < slen ? len : slen;
    if (capacity <= D) return;
    const unsigned long long room = capacity - D;  // ... below capacity
    len = room < len ? (uint32_t)room : len;
    const uint8_t *src = from + (unsigned long long)a;
    uint8_t *dst = out_bytes + (unsigned long long)D;
    // [0, head) bytes, [head, head + 4 nd) whole destination dwords, then `tail` bytes
    const uint32_t lead = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & 3u;
    const uint32_t head = lead < len ? lead : len;
    const uint32_t nd = (len - head) >> 2, tail = (len - head) & 3u;
    // destination dword i holds source bytes [head + 4 i, head + 4 i + 4): bytes sh .. sh + 3
    // of aligned source dwords i and i + 1 counted from sw, which starts at byte head - sh
    const uint32_t sh = (uint32_t)(uintptr_t)(src + head) & 3u;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - sh);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    // dwords [lo, hi): both source dwords lie in [0, slen) of the segment.  Dword 0 does not when
    // sw starts before the segment; at the end, dword i needs bytes below head - sh + 4 i + need
    const uint32_t lo = head < sh ? 1u : 0u, need = sh ? 8u : 4u;
    const long long most = ((long long)slen - (long long)need - (long long)head + (long long)sh) >> 2;  // floor
    uint32_t hi = most < 0 ? 0u : (most + 1 < (long long)nd ? (uint32_t)(most + 1) : nd);
    hi = hi < lo ? lo : hi;
    if (sh) paste_dwords<true>(sw, dw, lo, hi, sh, lane);
    else paste_dwords<false>(sw, dw, lo, hi, sh, lane);
    // the dwords left out (at most dword 0 and the last one), each from four byte loads inside
    // the segment by one lane; the head and tail bytes by lanes of their own
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
}

__global__ __launch_bounds__(kPasteThreads) void paste_copy_kernel(PasteSet ps, const uint8_t *__restrict__ bytes,
                                                                     const uint32_t *__restrict__ offsets,
                                                                     const uint8_t *__restrict__ patch_bytes,
                                                                     const uint32_t *__restrict__ patch_offsets,
                                                                     const uint32_t *__restrict__ out_offsets,
                                                                     uint8_t *__restrict__ out_bytes,
                                                                     unsigned long long capacity, uint32_t ntiles) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nblk = ps.nblk;
    const uint32_t stride = gridDim.x * kPasteWaves;
    for (uint32_t t = blockIdx.x * kPasteWaves + wv; t < ntiles; t += stride) {
        const uint32_t t0 = t * 64u;
        const int nb = nblk - t0 < 64u ? (int)(nblk - t0) : 64;  // >= 1
        const bool valid = lane < nb;
        const uint32_t ss = t0 + (uint32_t)(valid ? lane : nb - 1);  // past the end: the tile's last block
        const PasteFrom from = paste_from(ps, ss);
        const uint32_t *src = from.patch ? patch_offsets : offsets;
        const uint32_t at = from.patch ? from.d : ss;
        const uint32_t a = src[at], e = src[at + 1u];
        const uint32_t D = out_offsets[ss], Dn = out_offsets[ss + 1u];
        // a segment starts where the source changes or its block is not the previous lane's + 1:
        // one key per (source, block), both below 2^26, so keys of different sources are far apart
        const uint32_t key = from.patch ? (from.d | 0x80000000u) : ss;
        const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
        unsigned long long heads = __ballot(valid && (lane == 0 || key != prev + 1u));
        // the tile's own bytes: no segment may write outside them, whatever out_offsets holds
        const uint32_t T0 = __builtin_amdgcn_readfirstlane(D), T1 = __builtin_amdgcn_readlane(Dn, nb - 1);
        while (heads) {
            const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(heads));
            heads &= heads - 1ull;
            const int j = __builtin_amdgcn_readfirstlane(heads ? __builtin_ctzll(heads) : nb);  // lanes [i, j)
            const uint32_t sa = __builtin_amdgcn_readlane(a, i), se = __builtin_amdgcn_readlane(e, j - 1);
            const uint32_t sD = __builtin_amdgcn_readlane(D, i);
            uint32_t sDend = __builtin_amdgcn_readlane(Dn, j - 1);
            const bool patch = (__builtin_amdgcn_readlane(key, i) >> 31) != 0u;
            if (sD < T0 || sD > T1) continue;
            sDend = sDend < T1 ? sDend : T1;
            paste_segment(patch ? patch_bytes : bytes, sa, se, out_bytes, sD, sDend, capacity, lane);
        }
    }
}

// ws: the windows through the window decoder's own host check (ws.pl[k]: the window's own picture,
// ws.win[k]: its place in the stored plane); first[k]: each stored plane's first block, first[n..]
// the stored blocks in all.
static PasteSet paste_set(const WindowSet &ws, const uint32_t *first) {
    PasteSet ps = {};
    ps.n = ws.n;
    ps.nblk = first[kMaxPlanes];
    uint32_t next = 0;
    for (int k = 0; k < kMaxPlanes; ++k) {
        const int c = k < ws.n ? k : ws.n - 1;  // unused planes: copies of the last one, never selected
        const WindowPlane &w = ws.win[c];
        PastePlane &p = ps.pl[k];
        p.first = first[c];
        p.patch_first = next;
        p.bw = w.bw;
        p.nblk_frame = w.nblk_frame;
        p.div_bw = make_fastdiv(w.bw);
        p.div_frame = make_fastdiv(w.nblk_frame);
        p.f0 = w.var_first / w.nblk_frame;
        p.y0 = w.var_first % w.nblk_frame / w.bw;
        p.x0 = w.var_first % w.bw;
        p.wf = (uint32_t)(ws.pl[c].nblk / ws.pl[c].nblk_frame);
        p.wh = w.rows;
        p.ww = (uint32_t)ws.pl[c].bw;
        ps.var[k] = ws.var[c];
        if (k < ws.n) next += (uint32_t)ws.pl[k].nblk;
    }
    return ps;
}

hipError_t launch_bits_paste_offsets(const WindowSet &ws, const uint32_t *first, const uint32_t *offsets,
                                     const uint32_t *patch_offsets, const int32_t *const *patch_var,
                                     uint32_t *out_offsets, int32_t *out_var, void *wsp, hipStream_t stream,
                                     int num_cus) {
    PasteSet ps = paste_set(ws, first);
    for (int k = 0; k < kMaxPlanes; ++k) ps.pvar[k] = patch_var ? patch_var[k < ws.n ? k : ws.n - 1] : nullptr;
    const uint32_t nblk = ps.nblk, ntiles = (nblk + 63u) / 64u;
    hipError_t e = with_bools(
        [&](auto var) {
            return launch_persistent<paste_lengths_kernel<decltype(var)::value>, kPasteThreads, kPasteWaves,
                                     kPasteGridMult>((uint64_t)ntiles, num_cus, stream, ps, offsets, patch_offsets,
                                                     out_offsets, out_var, (uint32_t *)wsp, ntiles);
        },
        out_var != nullptr);
    if (e != hipSuccess) return e;
    if ((e = launch_rle_scan(wsp, ntiles, stream)) != hipSuccess) return e;
    return launch_rle_fixup(out_offsets, nblk, wsp, ntiles, 0, out_offsets + nblk, stream);
}

hipError_t launch_bits_paste_copy(const WindowSet &ws, const uint32_t *first, const uint8_t *bytes,
                                  const uint32_t *offsets, const uint8_t *patch_bytes, const uint32_t *patch_offsets,
                                  const uint32_t *out_offsets, uint8_t *out_bytes, unsigned long long capacity,
                                  hipStream_t stream, int num_cus) {
    const PasteSet ps = paste_set(ws, first);
    const uint32_t ntiles = (ps.nblk + 63u) / 64u;
    return launch_persistent<paste_copy_kernel, kPasteThreads, kPasteWaves, kPasteGridMult>(
        (uint64_t)ntiles, num_cus, stream, ps, bytes, offsets, patch_bytes, patch_offsets, out_offsets, out_bytes,
        capacity, ntiles);
}

}  // namespace dctq
