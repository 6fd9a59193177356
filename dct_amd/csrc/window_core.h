// dct_amd/csrc/window_core.h -- the run loop of the scaled window decoder (decode_scaled.hip):
// which stored blocks a wave takes from a WindowSet, and where they sit in the window's own
// picture.  It is the loop bits_window_to_pixels (decode_window.hip) spells out in its body;
// that kernel keeps its own text, because calling this function there changed its machine
// code (tools/isa_digest.py --diff), and a kernel that is not being changed keeps its code.
//
// A run (tools/window_ref.py states the mapping in plain Python): up to 64 consecutive stored
// blocks of one block row of one frame of one plane, inside that plane's window.  A window wb
// blocks wide has ceil(wb / 64) runs per block row; runs are numbered over window rows, then
// frames, then planes, and never straddle any of them.  Consecutive stored blocks are
// contiguous in the payload, so a run is to the bit source what a tile is: lanes hold
// offsets[s0 + min(lane, nb)], oend = offsets[s0 + nb], and nothing outside [offsets[s0], oend)
// is read.  A window narrower than 64 blocks leaves lanes idle; rows are not packed into one
// wave, which would break that contiguity.
#pragma once
#include "dctq_internal.h"

namespace dctq {

// Plane of run r (wave-uniform; a select chain over prefixes that stay in SGPRs).
__device__ __forceinline__ int plane_of_run(const WindowSet &ws, uint32_t r) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < kMaxPlanes; ++i) k += r >= ws.run_first[i] ? 1 : 0;
    return k;
}

// One wave (wv of WAVES in the workgroup) per run, grid-stride over the runs of ws:
//     body(k, q, f, y, j, rel, nb, offv, oend)
// once per run: plane k; window row q = f * rows + y over the window's frames, frame f and block
// row y of the WINDOW; run j of that row, so the run's first block is block q * bw + 64 j of the
// window's own picture ws.pl[k], in its block column 64 j; rel: that block's
// distance from the window's first block in the STORED plane's numbering (ws.win[k].first and
// .var_first); nb blocks; offv / oend as off_at (rle_decode_core.h).
template <int WAVES, typename Body>
__device__ __forceinline__ void for_window_runs(const WindowSet &ws, const uint32_t *__restrict__ offsets, int lane,
                                                int wv, Body &&body) {
    const uint32_t nruns = ws.run_first[kMaxPlanes];
    const uint32_t stride = gridDim.x * WAVES;
    for (uint32_t t = blockIdx.x * WAVES + wv; t < nruns; t += stride) {
        // run t -> plane k, window row q (over the window's frames), run j of that row
        const int k = plane_of_run(ws, t);
        uint32_t rf = 0u;
#pragma unroll
        for (int i = 1; i < kMaxPlanes; ++i) rf = k == i ? ws.run_first[i] : rf;
        const PlaneArgs &p = ws.pl[k];
        const WindowPlane &w = ws.win[k];
        const uint32_t rp = t - rf;
        const uint32_t q = fdiv(rp, w.div_runs), j = rp - q * w.runs_row;
        const uint32_t f = fdiv(q, w.div_rows), y = q - f * w.rows;
        // the run's first block: behind the window's first by f frames, y rows and 64 j blocks
        // of the STORED plane
        const uint32_t rel = f * w.nblk_frame + y * w.bw + 64u * j;
        const uint32_t s0 = w.first + rel;
        const uint32_t left = (uint32_t)p.bw - 64u * j;
        const int nb = left < 64u ? (int)left : 64;
        const uint32_t offv = offsets[s0 + (uint32_t)(lane < nb ? lane : nb)];  // lanes >= nb: the end of the run
        const uint32_t oend = offsets[s0 + (uint32_t)nb];
        body(k, q, f, y, j, rel, nb, offv, oend);
    }
}

}  // namespace dctq
