// dct_amd/csrc/api.hip -- the batched C-ABI of include/dct_amd.h.
//
// Host side of the hot path: the error string, argument validation and the entry
// points that launch the kernels on the caller's stream.  The plans and their tables
// are plan_tables.hip's, the rand() isolation isolation.hip's.
#include <string>

#include "dct_amd.h"
#include "dctq_internal.h"
#include "plan.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace dctq {
int fail(int code, const char *what, hipError_t e) {
    g_err = what;
    if (e != hipSuccess) {
        g_err += ": ";
        g_err += hipGetErrorString(e);
    }
    return code;
}
}  // namespace dctq
using dctq::fail;

// The small checks that several entry points share, each with its one wording.
static bool misaligned(const void *p, uintptr_t n) { return ((uintptr_t)p) % n != 0; }

static int check_workspace(const void *workspace) {
    if (!workspace) return fail(DCTQ_EINVAL, "workspace is NULL");
    if (misaligned(workspace, 4)) return fail(DCTQ_EINVAL, "workspace must be 4-byte aligned");
    return DCTQ_OK;
}

static int check_nplanes(int nplanes) {
    if (nplanes < 1 || nplanes > dctq::kMaxPlanes) return fail(DCTQ_EINVAL, "nplanes must be in [1, 4]");
    return DCTQ_OK;
}

static int check_symbol_bytes(int symbol_bytes) {
    if (symbol_bytes != 2 && symbol_bytes != 4) return fail(DCTQ_EINVAL, "symbol_bytes must be 2 or 4");
    return DCTQ_OK;
}

// what the three *_workspace_bytes exports of the offset scans answer: a count below 1 asks for one block's
static size_t scan_workspace_bytes(long long nblocks) { return dctq::rle_workspace_bytes(nblocks < 1 ? 1 : nblocks); }

int dctq::plane_args(const dctq_plane *s, dctq::PlaneArgs *a) {
    if (!s || !s->pixels) return fail(DCTQ_EINVAL, "plane/pixels is NULL");
    if (s->width <= 0 || s->height <= 0 || s->width % 8 || s->height % 8)
        return fail(DCTQ_EINVAL, "width and height must be positive multiples of 8");
    if (s->stride < s->width || s->stride % 8) return fail(DCTQ_EINVAL, "stride must be >= width and a multiple of 8");
    if (misaligned(s->pixels, 8) || s->frame_stride % 8) return fail(DCTQ_EINVAL, "pixels/frame_stride must be 8-byte aligned");
    if (s->nframes < 1) return fail(DCTQ_EINVAL, "nframes must be >= 1");
    if (s->nframes > 1 && s->frame_stride < s->stride * (long long)s->height)
        return fail(DCTQ_EINVAL, "frame_stride smaller than one frame");
    const long long bw = s->width / 8, bh = s->height / 8, per = bw * bh, tot = per * s->nframes;
    if (tot >= (1ll << 31) - 256) return fail(DCTQ_EINVAL, "more than 2^31 blocks in one call");
    a->src = s->pixels;
    a->stride = s->stride;
    a->frame_stride = s->frame_stride;
    a->bw = (int)bw;
    a->nblk_frame = (int)per;
    a->nblk = (int)tot;
    a->div_bw = dctq::make_fastdiv((uint32_t)bw);
    a->div_frame = dctq::make_fastdiv((uint32_t)per);
    const long long span = (s->nframes - 1) * s->frame_stride + (s->height - 1) * s->stride + s->width;
    a->span = span < 0xFFFFFFFFll ? (uint32_t)span : 0u;
    return DCTQ_OK;
}

// A plan's tables live on the device that was current at its creation.
int dctq::check_plan(const dctq_plan *plan) {
    if (!plan) return fail(DCTQ_EINVAL, "plan is NULL");
    int dev = -1;
    HIPCHK(hipGetDevice(&dev), "hipGetDevice");
    if (dev != plan->device) return fail(DCTQ_EINVAL, "plan was created on another device than the current one");
    return DCTQ_OK;
}

// first[k] = global index of plane k's first batch of `per` blocks; first[n..] = their total
// (< 4 * 2^26 for per >= 32)
static void plane_batches(const dctq::PlaneArgs *pl, int nplanes, int per, uint32_t (&first)[dctq::kMaxPlanes + 1]) {
    uint32_t next = 0;
    for (int k = 0; k <= dctq::kMaxPlanes; ++k) {
        first[k] = next;
        if (k < nplanes) next += (uint32_t)((pl[k].nblk + per - 1) / per);
    }
}

// blk_first[k] = plane k's first block in the concatenated numbering; blk_first[n] = their
// total, which must stay below `limit`
static int number_blocks(const dctq::PlaneArgs *pl, int n, uint32_t (&blk_first)[dctq::kMaxPlanes + 1], long long limit,
                         const char *too_many) {
    long long blocks = 0;
    for (int k = 0; k < n; ++k) {
        blk_first[k] = (uint32_t)blocks;
        blocks += pl[k].nblk;
        if (blocks >= limit) return fail(DCTQ_EINVAL, too_many);
    }
    blk_first[n] = (uint32_t)blocks;
    return DCTQ_OK;
}
static int number_blocks(dctq::EncodeSet *es, long long limit, const char *too_many) {
    return number_blocks(es->ps.pl, es->ps.n, es->blk_first, limit, too_many);
}

int dctq::plane_inputs(const dctq_plane *planes, int nplanes, dctq::PlaneSet *ps_out) {
    if (!planes) return fail(DCTQ_EINVAL, "planes is NULL");
    if (int rc = check_nplanes(nplanes)) return rc;
    dctq::PlaneSet &ps = *ps_out;
    ps = {};
    ps.n = nplanes;
    for (int k = 0; k < nplanes; ++k)
        if (int rc = dctq::plane_args(&planes[k], &ps.pl[k])) return rc;
    plane_batches(ps.pl, nplanes, 64, ps.first);
    return DCTQ_OK;
}

int dctq::plane_set(const dctq_plane *planes, int nplanes, int16_t *const *coef, int32_t *const *var_num,
                    dctq::PlaneSet *ps_out) {
    if (!planes || !coef) return fail(DCTQ_EINVAL, "planes/coef is NULL");
    if (int rc = dctq::plane_inputs(planes, nplanes, ps_out)) return rc;
    dctq::PlaneSet &ps = *ps_out;
    for (int k = 0; k < nplanes; ++k) {
        if (!coef[k]) return fail(DCTQ_EINVAL, "coef[k] is NULL");
        if (misaligned(coef[k], 16)) return fail(DCTQ_EINVAL, "coef must be 16-byte aligned");
        if (var_num && !var_num[k]) return fail(DCTQ_EINVAL, "var_num given but var_num[k] is NULL");
        ps.coef[k] = coef[k];
        ps.var[k] = var_num ? var_num[k] : nullptr;
    }
    return DCTQ_OK;
}

extern "C" {

int dctq_forward_quant_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                              int32_t *const *var_num, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryForwardQuantPlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    dctq::PlaneSet ps;
    int rc = dctq::plane_set(planes, nplanes, coef, var_num, &ps);
    if (rc) return rc;
    HIPCHK(dctq::launch_fdct8_quant(ps, plan->dev, plan->adaptive, plan->fallbacks, (hipStream_t)stream,
                                    plan->num_cus),
           "fdct8_quant_v3 launch");
    return DCTQ_OK;
}

int dctq_round_trip_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                           int32_t *const *var_num, float *const *recon, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRoundTripPlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!recon) return fail(DCTQ_EINVAL, "recon is NULL");
    dctq::RoundTripSet rt = {};
    int rc = dctq::plane_set(planes, nplanes, coef, var_num, &rt.ps);
    if (rc) return rc;
    for (int k = 0; k < nplanes; ++k) {
        if (!recon[k] || misaligned(recon[k], 16)) return fail(DCTQ_EINVAL, "recon[k] NULL or not 16-byte aligned");
        rt.recon[k] = recon[k];
    }
    HIPCHK(dctq::launch_roundtrip(rt, plan->dev, plan->adaptive, plan->inv_f32 != 0, plan->fallbacks,
                                  (hipStream_t)stream, plan->num_cus),
           "roundtrip launch");
    return DCTQ_OK;
}

size_t dctq_encode_workspace_bytes(long long total_blocks) {
    return dctq::encode_workspace_bytes((total_blocks < 1 ? 1 : total_blocks) / 64 + dctq::kMaxPlanes + 1);
}

int dctq_plan_symbol_bytes(const dctq_plan *plan) { return plan ? plan->symbol_bytes : DCTQ_EINVAL; }

int dctq_abi_version(void) { return DCTQ_ABI_VERSION; }

static int encode_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                         uint32_t *offsets, void *symbols, long long symbols_capacity, void *workspace, void *stream,
                         int symbol_bytes) {
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!offsets || !workspace) return fail(DCTQ_EINVAL, "offsets/workspace is NULL");
    if (symbols_capacity < 0) return fail(DCTQ_EINVAL, "symbols_capacity < 0");
    if (misaligned(symbols, 4)) return fail(DCTQ_EINVAL, "symbols must be 4-byte aligned");
    if (int rc = check_workspace(workspace)) return rc;
    if (symbol_bytes == 2 && plan->symbol_bytes != 2)
        return fail(DCTQ_EINVAL, "the plan's quantized coefficients can exceed 511: 2-byte symbols cannot hold them "
                                 "(dctq_plan_symbol_bytes == 4; use dctq_encode_planes)");
    dctq::EncodeSet es = {};
    int rc = dctq::plane_set(planes, nplanes, coef, nullptr, &es.ps);
    if (rc) return rc;
    if ((rc = number_blocks(&es, 1ll << 26, "more than 2^26 - 1 blocks in one encode"))) return rc;
    HIPCHK(dctq::launch_encode(es, plan->dev, plan->adaptive, offsets, symbols, symbol_bytes,
                               symbols ? (unsigned long long)symbols_capacity : 0ull, workspace, (hipStream_t)stream,
                               plan->num_cus),
           "encode launch");
    return DCTQ_OK;
}

int dctq_encode_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                       uint32_t *offsets, uint32_t *symbols, long long symbols_capacity, void *workspace,
                       void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryEncodePlanes);
    return encode_planes(plan, planes, nplanes, coef, offsets, symbols, symbols_capacity, workspace, stream, 4);
}

int dctq_encode_planes16(const dctq_plan *plan, const dctq_plane *planes, int nplanes, int16_t *const *coef,
                         uint32_t *offsets, uint16_t *symbols, long long symbols_capacity, void *workspace,
                         void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryEncodePlanes16);
    return encode_planes(plan, planes, nplanes, coef, offsets, symbols, symbols_capacity, workspace, stream, 2);
}

int dctq_forward_quant(const dctq_plan *plan, const dctq_plane *src, int16_t *coef, int32_t *var_num, void *stream) {
    if (!src) return fail(DCTQ_EINVAL, "plane is NULL");
    return dctq_forward_quant_planes(plan, src, 1, &coef, var_num ? &var_num : nullptr, stream);
}

int dctq_forward_float(const dctq_plan *plan, const dctq_plane *src, float *coef, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryForwardFloat);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!coef) return fail(DCTQ_EINVAL, "coef is NULL");
    if (misaligned(coef, 16)) return fail(DCTQ_EINVAL, "coef must be 16-byte aligned");
    dctq::PlaneArgs a;
    int rc = dctq::plane_args(src, &a);
    if (rc) return rc;
    HIPCHK(dctq::launch_fdct8_float_pair(a, plan->dev, coef, (hipStream_t)stream, plan->num_cus),
           "fdct8_float_pair launch");
    return DCTQ_OK;
}

int dctq_inverse(const dctq_plan *plan, const int16_t *coef, const int32_t *var_num, long long nblocks, float *recon,
                 void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryInverse);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!coef || !recon) return fail(DCTQ_EINVAL, "coef/recon is NULL");
    if (plan->adaptive && !var_num) return fail(DCTQ_EINVAL, "adaptive inverse needs var_num");
    if (nblocks < 0 || nblocks >= (1ll << 40)) return fail(DCTQ_EINVAL, "bad nblocks");
    if (misaligned(coef, 16) || misaligned(recon, 16)) return fail(DCTQ_EINVAL, "coef/recon must be 16-byte aligned");
    if (nblocks == 0) return DCTQ_OK;
    HIPCHK(dctq::launch_idct8_pair(plan->dev, plan->adaptive, coef, var_num, nblocks, recon, (hipStream_t)stream,
                                   plan->num_cus),
           "idct8_pair launch");
    return DCTQ_OK;
}

// The destination planes of a decoder: pl[k] from dst[k], var[k] = var_num[k] for an adaptive plan (else NULL).
// input(k): the caller's own checks of plane k's input, between the plane's and its var_num's.
extern "C++" template <typename F>
static int decoder_planes(const dctq_plan *plan, const int32_t *const *var_num, const dctq_plane *dst, int nplanes,
                          dctq::PlaneArgs *pl, const int32_t **var, F &&input) {
    if (int rc = check_nplanes(nplanes)) return rc;
    if (plan->adaptive && !var_num) return fail(DCTQ_EINVAL, "adaptive decode needs var_num");
    for (int k = 0; k < nplanes; ++k) {
        if (int rc = dctq::plane_args(&dst[k], &pl[k])) return rc;
        if (int rc = input(k)) return rc;
        if (plan->adaptive && !var_num[k]) return fail(DCTQ_EINVAL, "adaptive decode needs every var_num[k]");
        var[k] = plan->adaptive ? var_num[k] : nullptr;
    }
    return DCTQ_OK;
}

int dctq_decode_planes(const dctq_plan *plan, const int16_t *const *coef, const int32_t *const *var_num,
                       const dctq_plane *dst, int nplanes, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryDecodePlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!coef || !dst) return fail(DCTQ_EINVAL, "coef/dst is NULL");
    dctq::DecodeSet ds = {};
    ds.n = nplanes;
    const auto coef_of_plane = [&](int k) {
        if (!coef[k]) return fail(DCTQ_EINVAL, "coef[k] is NULL");
        if (misaligned(coef[k], 16)) return fail(DCTQ_EINVAL, "coef must be 16-byte aligned");
        ds.coef[k] = coef[k];
        return (int)DCTQ_OK;
    };
    if (int rc = decoder_planes(plan, var_num, dst, nplanes, ds.pl, ds.var, coef_of_plane)) return rc;
    plane_batches(ds.pl, nplanes, 32, ds.first);
    HIPCHK(dctq::launch_decode(ds, plan->dev, plan->adaptive, plan->inv_f32 != 0, (hipStream_t)stream, plan->num_cus),
           "decode launch");
    return DCTQ_OK;
}

// The fused decoders' planes: decoder_planes and the concatenated block numbering.
static int symbol_set(const dctq_plan *plan, const int32_t *const *var_num, const dctq_plane *dst, int nplanes,
                      dctq::SymbolSet *out) {
    dctq::SymbolSet &ss = *out;
    ss = {};
    ss.n = nplanes;
    if (int rc = decoder_planes(plan, var_num, dst, nplanes, ss.pl, ss.var, [](int) { return (int)DCTQ_OK; })) return rc;
    if (int rc = number_blocks(ss.pl, nplanes, ss.blk_first, 1ll << 26, "more than 2^26 - 1 blocks in one decode"))
        return rc;
    for (int k = nplanes + 1; k <= dctq::kMaxPlanes; ++k) ss.blk_first[k] = ss.blk_first[nplanes];
    return DCTQ_OK;
}

int dctq_decode_symbols_planes(const dctq_plan *plan, const void *symbols, int symbol_bytes, const uint32_t *offsets,
                               const int32_t *const *var_num, const dctq_plane *dst, int nplanes, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryDecodeSymbolsPlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!symbols || !offsets || !dst) return fail(DCTQ_EINVAL, "symbols/offsets/dst is NULL");
    if (int rc = check_symbol_bytes(symbol_bytes)) return rc;
    if (misaligned(symbols, 4) || misaligned(offsets, 4)) return fail(DCTQ_EINVAL, "symbols/offsets must be 4-byte aligned");
    dctq::SymbolSet ss;
    if (int rc = symbol_set(plan, var_num, dst, nplanes, &ss)) return rc;
    HIPCHK(dctq::launch_decode_symbols(ss, symbols, symbol_bytes, offsets, plan->dev, plan->adaptive,
                                       plan->inv_f32 != 0, (hipStream_t)stream, plan->num_cus),
           "decode_symbols launch");
    return DCTQ_OK;
}

int dctq_decode_bits_planes(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                            const int32_t *const *var_num, const dctq_plane *dst, int nplanes, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryDecodeBitsPlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!bytes || !offsets || !dst) return fail(DCTQ_EINVAL, "bytes/offsets/dst is NULL");
    if (misaligned(offsets, 4)) return fail(DCTQ_EINVAL, "offsets must be 4-byte aligned");
    dctq::SymbolSet ss;
    if (int rc = symbol_set(plan, var_num, dst, nplanes, &ss)) return rc;
    HIPCHK(dctq::launch_decode_bits(ss, bytes, offsets, plan->dev, plan->adaptive, plan->inv_f32 != 0,
                                    (hipStream_t)stream, plan->num_cus),
           "decode_bits launch");
    return DCTQ_OK;
}

// plane_args for the reduced picture of the scaled window decoder: n = 8 / scale pixels a block
// side, so everything plane_args asks in units of 8 is asked in units of n, and the block
// counts are the window's.
static int scaled_plane_args(const dctq_plane *s, int n, dctq::PlaneArgs *a) {
    if (!s || !s->pixels) return fail(DCTQ_EINVAL, "plane/pixels is NULL");
    if (s->width <= 0 || s->height <= 0 || s->width % n || s->height % n)
        return fail(DCTQ_EINVAL, "scaled: dst width and height must be positive multiples of 8 / scale");
    if (s->stride < s->width || s->stride % n)
        return fail(DCTQ_EINVAL, "scaled: dst stride must be >= width and a multiple of 8 / scale");
    if (misaligned(s->pixels, (uintptr_t)n) || s->frame_stride % n)
        return fail(DCTQ_EINVAL, "scaled: dst pixels/frame_stride must be aligned to 8 / scale bytes");
    if (s->nframes < 1) return fail(DCTQ_EINVAL, "nframes must be >= 1");
    if (s->nframes > 1 && s->frame_stride < s->stride * (long long)s->height)
        return fail(DCTQ_EINVAL, "frame_stride smaller than one frame");
    const long long bw = s->width / n, bh = s->height / n, per = bw * bh, tot = per * s->nframes;
    if (tot >= (1ll << 31) - 256) return fail(DCTQ_EINVAL, "more than 2^31 blocks in one call");
    a->src = s->pixels;
    a->stride = s->stride;
    a->frame_stride = s->frame_stride;
    a->bw = (int)bw;
    a->nblk_frame = (int)per;
    a->nblk = (int)tot;
    a->div_bw = dctq::make_fastdiv((uint32_t)bw);
    a->div_frame = dctq::make_fastdiv((uint32_t)per);
    const long long span = (s->nframes - 1) * s->frame_stride + (s->height - 1) * s->stride + s->width;
    a->span = span < 0xFFFFFFFFll ? (uint32_t)span : 0u;
    return DCTQ_OK;
}

// The window decoders' planes: dst[k] placed in the stored plane win[k] describes, the stored
// planes' concatenated block numbering and the run numbering (tools/window_ref.py).  log2_scale
// 0: dst[k] is the window's own picture; 1..3: its reduction by 2, 4 or 8, so the window's
// extent is dst[k]'s width and height times that.  Needs no plan and no device, so every
// refusal of the geometry comes before either is looked at.
static int window_set(const dctq_window *win, const dctq_plane *dst, int nplanes, int log2_scale,
                      dctq::WindowSet *out) {
    if (!win || !dst) return fail(DCTQ_EINVAL, "win/dst is NULL");
    if (int rc = check_nplanes(nplanes)) return rc;
    dctq::WindowSet &ws = *out;
    ws = {};
    ws.n = nplanes;
    long long blocks = 0, runs = 0;
    for (int k = 0; k < nplanes; ++k) {
        const dctq_window &w = win[k];
        if (w.width <= 0 || w.height <= 0 || w.width % 8 || w.height % 8)
            return fail(DCTQ_EINVAL, "window: the stored width and height must be positive multiples of 8");
        if (w.nframes < 1) return fail(DCTQ_EINVAL, "window: the stored nframes must be >= 1");
        if (w.x0 < 0 || w.y0 < 0 || w.x0 % 8 || w.y0 % 8)
            return fail(DCTQ_EINVAL, "window: x0 and y0 must be non-negative multiples of 8");
        if (w.frame0 < 0) return fail(DCTQ_EINVAL, "window: frame0 must be >= 0");
        dctq::PlaneArgs &p = ws.pl[k];
        if (int rc = log2_scale ? scaled_plane_args(&dst[k], 8 >> log2_scale, &p) : dctq::plane_args(&dst[k], &p))
            return rc;
        const long long ww = (long long)dst[k].width << log2_scale, wh = (long long)dst[k].height << log2_scale;
        if (w.x0 + ww > w.width || w.y0 + wh > w.height)
            return fail(DCTQ_EINVAL, "window: the region leaves the stored plane");
        if ((long long)w.frame0 + dst[k].nframes > w.nframes)
            return fail(DCTQ_EINVAL, "window: the frame range leaves the stored frames");
        const long long sbw = w.width / 8, sper = sbw * (w.height / 8);
        if (blocks + sper * w.nframes >= 1ll << 26) return fail(DCTQ_EINVAL, "more than 2^26 - 1 blocks in one decode");
        dctq::WindowPlane &wp = ws.win[k];
        wp.var_first = (uint32_t)(w.frame0 * sper + (w.y0 / 8) * sbw + w.x0 / 8);
        wp.first = (uint32_t)blocks + wp.var_first;
        wp.bw = (uint32_t)sbw;
        wp.nblk_frame = (uint32_t)sper;
        wp.rows = (uint32_t)(p.nblk_frame / p.bw);
        wp.runs_row = (uint32_t)((p.bw + 63) / 64);
        wp.div_runs = dctq::make_fastdiv(wp.runs_row);
        wp.div_rows = dctq::make_fastdiv(wp.rows);
        ws.run_first[k] = (uint32_t)runs;
        blocks += sper * w.nframes;
        runs += (long long)wp.runs_row * wp.rows * dst[k].nframes;  // at most the window's blocks: < 2^26
    }
    for (int k = nplanes; k <= dctq::kMaxPlanes; ++k) ws.run_first[k] = (uint32_t)runs;
    return DCTQ_OK;
}

// What the window decoders check after the geometry: the plan (and its device), the stream's
// pointers, and var_num where the plan is adaptive (into ws->var).
static int window_source(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                         const int32_t *const *var_num, int nplanes, dctq::WindowSet *ws) {
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!bytes || !offsets) return fail(DCTQ_EINVAL, "bytes/offsets is NULL");
    if (misaligned(offsets, 4)) return fail(DCTQ_EINVAL, "offsets must be 4-byte aligned");
    if (plan->adaptive && !var_num) return fail(DCTQ_EINVAL, "adaptive decode needs var_num");
    for (int k = 0; k < nplanes; ++k) {
        if (plan->adaptive && !var_num[k]) return fail(DCTQ_EINVAL, "adaptive decode needs every var_num[k]");
        ws->var[k] = plan->adaptive ? var_num[k] : nullptr;
    }
    return DCTQ_OK;
}

int dctq_decode_bits_window_planes(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                                   const int32_t *const *var_num, const dctq_window *win, const dctq_plane *dst,
                                   int nplanes, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryDecodeBitsWindowPlanes);
    dctq::WindowSet ws;
    if (int rc = window_set(win, dst, nplanes, 0, &ws)) return rc;
    if (int rc = window_source(plan, bytes, offsets, var_num, nplanes, &ws)) return rc;
    HIPCHK(dctq::launch_decode_bits_window(ws, bytes, offsets, plan->dev, plan->adaptive, plan->inv_f32 != 0,
                                           (hipStream_t)stream, plan->num_cus),
           "decode_bits_window launch");
    return DCTQ_OK;
}

int dctq_decode_bits_window_scaled_planes(const dctq_plan *plan, const uint8_t *bytes, const uint32_t *offsets,
                                          const int32_t *const *var_num, const dctq_window *win,
                                          const dctq_plane *dst, int nplanes, int log2_scale, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryDecodeBitsWindowScaledPlanes);
    if (log2_scale < 1 || log2_scale > 3) return fail(DCTQ_EINVAL, "scaled: log2_scale must be 1, 2 or 3");
    dctq::WindowSet ws;
    if (int rc = window_set(win, dst, nplanes, log2_scale, &ws)) return rc;
    if (int rc = window_source(plan, bytes, offsets, var_num, nplanes, &ws)) return rc;
    HIPCHK(dctq::launch_decode_bits_window_scaled(ws, bytes, offsets, plan->dev, plan->adaptive, log2_scale,
                                                  (hipStream_t)stream, plan->num_cus),
           "decode_bits_window_scaled launch");
    return DCTQ_OK;
}

// The stream extraction's windows: window_set over planes that stand for the extents (a window's
// own picture as a dense plane that is never touched), so the geometry is the window decoder's
// check and not a copy of it.
static int extent_window_set(const dctq_window *win, const dctq_extent *ext, int nplanes, dctq::WindowSet *ws) {
    alignas(8) static const uint8_t no_pixels[8] = {};
    if (!win || !ext) return fail(DCTQ_EINVAL, "win/ext is NULL");
    if (int rc = check_nplanes(nplanes)) return rc;
    dctq_plane dst[dctq::kMaxPlanes];
    for (int k = 0; k < nplanes; ++k)
        dst[k] = {no_pixels, ext[k].width, (long long)ext[k].width * ext[k].height, ext[k].width, ext[k].height,
                  ext[k].nframes};
    return window_set(win, dst, nplanes, 0, ws);
}

static int device_cus();

size_t dctq_bits_window_workspace_bytes(long long window_blocks) { return scan_workspace_bytes(window_blocks); }

int dctq_bits_window_offsets(const uint32_t *offsets, const int32_t *const *var_num, const dctq_window *win,
                             const dctq_extent *ext, int nplanes, uint32_t *win_offsets, int32_t *win_var_num,
                             void *workspace, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBitsWindowOffsets);
    dctq::WindowSet ws;
    if (int rc = extent_window_set(win, ext, nplanes, &ws)) return rc;
    if (!offsets || !win_offsets) return fail(DCTQ_EINVAL, "offsets/win_offsets is NULL");
    if (misaligned(offsets, 4) || misaligned(win_offsets, 4))
        return fail(DCTQ_EINVAL, "offsets and win_offsets must be 4-byte aligned");
    if (var_num) {
        if (!win_var_num || misaligned(win_var_num, 4))
            return fail(DCTQ_EINVAL, "var_num given but win_var_num is NULL or not 4-byte aligned");
        for (int k = 0; k < nplanes; ++k) {
            if (!var_num[k] || misaligned(var_num[k], 4))
                return fail(DCTQ_EINVAL, "var_num given but var_num[k] is NULL or not 4-byte aligned");
            ws.var[k] = var_num[k];
        }
    }
    if (int rc = check_workspace(workspace)) return rc;
    HIPCHK(dctq::launch_bits_window_offsets(ws, offsets, win_offsets, var_num ? win_var_num : nullptr, workspace,
                                            (hipStream_t)stream, device_cus()),
           "bits_window_offsets launch");
    return DCTQ_OK;
}

int dctq_bits_window_gather(const uint8_t *bytes, const uint32_t *offsets, const dctq_window *win,
                            const dctq_extent *ext, int nplanes, const uint32_t *win_offsets, uint8_t *win_bytes,
                            size_t capacity, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBitsWindowGather);
    dctq::WindowSet ws;
    if (int rc = extent_window_set(win, ext, nplanes, &ws)) return rc;
    if (!bytes || !offsets || !win_offsets || !win_bytes)
        return fail(DCTQ_EINVAL, "bytes/offsets/win_offsets/win_bytes is NULL");
    if (misaligned(offsets, 4) || misaligned(win_offsets, 4))
        return fail(DCTQ_EINVAL, "offsets and win_offsets must be 4-byte aligned");
    if (!capacity) return DCTQ_OK;
    HIPCHK(dctq::launch_bits_window_gather(ws, bytes, offsets, win_offsets, win_bytes, (unsigned long long)capacity,
                                           (hipStream_t)stream, device_cus()),
           "bits_window_gather launch");
    return DCTQ_OK;
}

// The stream paste's geometry: the extraction's windows, plus each stored plane's first block
// (first[k]; first[nplanes..] the stored blocks in all, < 2^26 after window_set).
static int paste_window_set(const dctq_window *win, const dctq_extent *ext, int nplanes, dctq::WindowSet *ws,
                            uint32_t *first) {
    if (int rc = extent_window_set(win, ext, nplanes, ws)) return rc;
    uint32_t next = 0;
    for (int k = 0; k <= dctq::kMaxPlanes; ++k) {
        first[k] = next;
        if (k < nplanes) next += (uint32_t)((long long)(win[k].width / 8) * (win[k].height / 8) * win[k].nframes);
    }
    return DCTQ_OK;
}

size_t dctq_bits_paste_workspace_bytes(long long stored_blocks) { return scan_workspace_bytes(stored_blocks); }

int dctq_bits_paste_offsets(const uint32_t *offsets, const int32_t *const *var_num, const uint32_t *patch_offsets,
                            const int32_t *const *patch_var_num, size_t payload_bytes, size_t patch_payload_bytes,
                            const dctq_window *win, const dctq_extent *ext, int nplanes, uint32_t *out_offsets,
                            int32_t *out_var_num, void *workspace, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBitsPasteOffsets);
    dctq::WindowSet ws;
    uint32_t first[dctq::kMaxPlanes + 1];
    if (int rc = paste_window_set(win, ext, nplanes, &ws, first)) return rc;
    // the result holds at most both payloads, and its offsets are 32-bit
    if ((unsigned long long)payload_bytes >= (1ull << 32) || (unsigned long long)patch_payload_bytes >= (1ull << 32) ||
        (unsigned long long)payload_bytes + (unsigned long long)patch_payload_bytes >= (1ull << 32))
        return fail(DCTQ_EINVAL, "paste: payload_bytes + patch_payload_bytes must stay below 2^32");
    if (!offsets || !patch_offsets || !out_offsets) return fail(DCTQ_EINVAL, "offsets/patch_offsets/out_offsets is NULL");
    if (misaligned(offsets, 4) || misaligned(patch_offsets, 4) || misaligned(out_offsets, 4))
        return fail(DCTQ_EINVAL, "offsets, patch_offsets and out_offsets must be 4-byte aligned");
    if (!var_num != !patch_var_num) return fail(DCTQ_EINVAL, "paste: var_num and patch_var_num are both given or both NULL");
    if (var_num) {
        if (!out_var_num || misaligned(out_var_num, 4))
            return fail(DCTQ_EINVAL, "var_num given but out_var_num is NULL or not 4-byte aligned");
        for (int k = 0; k < nplanes; ++k) {
            if (!var_num[k] || misaligned(var_num[k], 4) || !patch_var_num[k] || misaligned(patch_var_num[k], 4))
                return fail(DCTQ_EINVAL, "var_num given but var_num[k] or patch_var_num[k] is NULL or not 4-byte aligned");
            ws.var[k] = var_num[k];
        }
    }
    if (int rc = check_workspace(workspace)) return rc;
    HIPCHK(dctq::launch_bits_paste_offsets(ws, first, offsets, patch_offsets, var_num ? patch_var_num : nullptr,
                                           out_offsets, var_num ? out_var_num : nullptr, workspace,
                                           (hipStream_t)stream, device_cus()),
           "bits_paste_offsets launch");
    return DCTQ_OK;
}

int dctq_bits_paste_copy(const uint8_t *bytes, const uint32_t *offsets, const uint8_t *patch_bytes,
                         const uint32_t *patch_offsets, const dctq_window *win, const dctq_extent *ext, int nplanes,
                         const uint32_t *out_offsets, uint8_t *out_bytes, size_t capacity, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBitsPasteCopy);
    dctq::WindowSet ws;
    uint32_t first[dctq::kMaxPlanes + 1];
    if (int rc = paste_window_set(win, ext, nplanes, &ws, first)) return rc;
    if (!bytes || !offsets || !patch_bytes || !patch_offsets || !out_offsets || !out_bytes)
        return fail(DCTQ_EINVAL, "bytes/offsets/patch_bytes/patch_offsets/out_offsets/out_bytes is NULL");
    if (misaligned(offsets, 4) || misaligned(patch_offsets, 4) || misaligned(out_offsets, 4))
        return fail(DCTQ_EINVAL, "offsets, patch_offsets and out_offsets must be 4-byte aligned");
    if (!capacity) return DCTQ_OK;
    HIPCHK(dctq::launch_bits_paste_copy(ws, first, bytes, offsets, patch_bytes, patch_offsets, out_offsets, out_bytes,
                                        (unsigned long long)capacity, (hipStream_t)stream, device_cus()),
           "bits_paste_copy launch");
    return DCTQ_OK;
}

int dctq_synth(uint64_t seed, int kind, const dctq_plane *dst, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntrySynth);
    if (!dst || !dst->pixels) return fail(DCTQ_EINVAL, "dst is NULL");
    if (dst->width <= 0 || dst->height <= 0 || dst->width % 4 || dst->stride < dst->width || dst->stride % 4 ||
        dst->nframes < 1 || misaligned(dst->pixels, 4))
        return fail(DCTQ_EINVAL, "bad synth plane geometry");
    HIPCHK(dctq::launch_synth(seed, kind, (uint8_t *)dst->pixels, dst->stride, dst->frame_stride, dst->width,
                              dst->height, dst->nframes, (hipStream_t)stream),
           "synth launch");
    return DCTQ_OK;
}

static int device_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return 256;
    return n;
}

static int rle_args(const void *a, const void *b, long long nblocks) {
    if (!a || !b) return fail(DCTQ_EINVAL, "NULL pointer");
    if (nblocks < 1 || nblocks >= (1ll << 26)) return fail(DCTQ_EINVAL, "nblocks must be in [1, 2^26)");
    return DCTQ_OK;
}

size_t dctq_rle_workspace_bytes(long long nblocks) { return scan_workspace_bytes(nblocks); }

int dctq_rle_count(const int16_t *coef, long long nblocks, uint32_t *offsets, void *workspace, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRleCount);
    if (int rc = rle_args(coef, offsets, nblocks)) return rc;
    if (int rc = check_workspace(workspace)) return rc;
    HIPCHK(dctq::launch_rle_count(coef, nblocks, offsets, workspace, (hipStream_t)stream, device_cus()),
           "rle_count launch");
    return DCTQ_OK;
}

int dctq_rle_emit(const int16_t *coef, long long nblocks, const uint32_t *offsets, uint32_t *symbols, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRleEmit);
    if (int rc = rle_args(coef, offsets, nblocks)) return rc;
    if (!symbols) return fail(DCTQ_EINVAL, "symbols is NULL");
    HIPCHK(dctq::launch_rle_emit(coef, nblocks, offsets, symbols, 4, ~0ull, (hipStream_t)stream, device_cus()),
           "rle_emit launch");
    return DCTQ_OK;
}

int dctq_rle_decode(const uint32_t *symbols, const uint32_t *offsets, long long nblocks, int16_t *coef,
                    void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRleDecode);
    if (int rc = rle_args(symbols, offsets, nblocks)) return rc;
    if (!coef) return fail(DCTQ_EINVAL, "coef is NULL");
    HIPCHK(dctq::launch_rle_decode(symbols, 4, offsets, nblocks, coef, (hipStream_t)stream, device_cus()),
           "rle_decode launch");
    return DCTQ_OK;
}

int dctq_rle_decode16(const uint16_t *symbols, const uint32_t *offsets, long long nblocks, int16_t *coef,
                      void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRleDecode16);
    if (int rc = rle_args(symbols, offsets, nblocks)) return rc;
    if (!coef) return fail(DCTQ_EINVAL, "coef is NULL");
    if (misaligned(symbols, 4)) return fail(DCTQ_EINVAL, "symbols must be 4-byte aligned");
    HIPCHK(dctq::launch_rle_decode(symbols, 2, offsets, nblocks, coef, (hipStream_t)stream, device_cus()),
           "rle_decode16 launch");
    return DCTQ_OK;
}

size_t dctq_bits_workspace_bytes(long long nblocks) { return scan_workspace_bytes(nblocks); }

int dctq_bits_pack(const void *symbols, int symbol_bytes, const uint32_t *sym_offsets, long long nblocks,
                   uint32_t *offsets, uint8_t *bytes, long long bytes_capacity, void *workspace, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBitsPack);
    if (int rc = rle_args(symbols, sym_offsets, nblocks)) return rc;
    if (!offsets || !workspace) return fail(DCTQ_EINVAL, "offsets/workspace is NULL");
    if (int rc = check_symbol_bytes(symbol_bytes)) return rc;
    // offsets are 32-bit and a block takes up to 368 B
    if (368 * nblocks >= (1ll << 32)) return fail(DCTQ_EINVAL, "368 * nblocks must stay below 2^32");
    if (bytes_capacity < 0) return fail(DCTQ_EINVAL, "bytes_capacity < 0");
    if (misaligned(symbols, 4) || misaligned(sym_offsets, 4) || misaligned(offsets, 4) || misaligned(bytes, 4))
        return fail(DCTQ_EINVAL, "symbols/sym_offsets/offsets/bytes must be 4-byte aligned");
    if (int rc = check_workspace(workspace)) return rc;
    HIPCHK(dctq::launch_bits_pack(symbols, symbol_bytes, sym_offsets, nblocks, offsets, bytes,
                                  bytes ? (unsigned long long)bytes_capacity : 0ull, workspace, (hipStream_t)stream,
                                  device_cus()),
           "bits_pack launch");
    return DCTQ_OK;
}

int dctq_bits_decode(const uint8_t *bytes, const uint32_t *offsets, long long nblocks, int16_t *coef, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBitsDecode);
    if (int rc = rle_args(bytes, offsets, nblocks)) return rc;
    if (!coef) return fail(DCTQ_EINVAL, "coef is NULL");
    if (misaligned(offsets, 4) || misaligned(coef, 16)) return fail(DCTQ_EINVAL, "offsets must be 4-byte, coef 16-byte aligned");
    HIPCHK(dctq::launch_bits_decode(bytes, offsets, nblocks, coef, (hipStream_t)stream, device_cus()),
           "bits_decode launch");
    return DCTQ_OK;
}

// the arguments the two frame entry points share: 1 <= nblocks <= 11 671 106 (368 * nblocks < 2^32, as dctq_bits_pack)
static int frame_args(const void *offsets, const void *lengths, int length_bytes, long long nblocks) {
    if (!offsets || !lengths) return fail(DCTQ_EINVAL, "offsets/lengths is NULL");
    if (length_bytes != 1 && length_bytes != 2) return fail(DCTQ_EINVAL, "length_bytes must be 1 or 2");
    if (nblocks < 1 || 368 * nblocks >= (1ll << 32)) return fail(DCTQ_EINVAL, "nblocks must be in [1, 11671106]");
    if (misaligned(offsets, 4) || misaligned(lengths, 4))
        return fail(DCTQ_EINVAL, "offsets and lengths must be 4-byte aligned");
    return DCTQ_OK;
}

int dctq_block_lengths(const uint32_t *offsets, long long nblocks, int length_bytes, void *lengths,
                       uint32_t *max_length, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBlockLengths);
    if (int rc = frame_args(offsets, lengths, length_bytes, nblocks)) return rc;
    if (!max_length || misaligned(max_length, 4)) return fail(DCTQ_EINVAL, "max_length is NULL or not 4-byte aligned");
    HIPCHK(dctq::launch_block_lengths(offsets, nblocks, length_bytes, lengths, max_length, (hipStream_t)stream,
                                      device_cus()),
           "block_lengths launch");
    return DCTQ_OK;
}

size_t dctq_block_offsets_workspace_bytes(long long nblocks) { return scan_workspace_bytes(nblocks); }

int dctq_block_offsets(const void *lengths, int length_bytes, long long nblocks, uint32_t *offsets, void *workspace,
                       void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryBlockOffsets);
    if (int rc = frame_args(offsets, lengths, length_bytes, nblocks)) return rc;
    if (int rc = check_workspace(workspace)) return rc;
    HIPCHK(dctq::launch_block_offsets(lengths, length_bytes, nblocks, offsets, workspace, (hipStream_t)stream,
                                      device_cus()),
           "block_offsets launch");
    return DCTQ_OK;
}

int dctq_huffman_bits(const int16_t *coef, long long nblocks, uint32_t *bits, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryHuffmanBits);
    if (!coef || !bits) return fail(DCTQ_EINVAL, "coef/bits is NULL");
    if (nblocks < 0) return fail(DCTQ_EINVAL, "nblocks < 0");
    if (misaligned(coef, 16) || misaligned(bits, 4)) return fail(DCTQ_EINVAL, "coef must be 16-byte, bits 4-byte aligned");
    if (nblocks == 0) return DCTQ_OK;
    HIPCHK(dctq::launch_huffman_bits(coef, nblocks, bits, (hipStream_t)stream, device_cus()), "huffman_bits launch");
    return DCTQ_OK;
}

int dctq_huffman_bits_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, uint32_t *bits,
                             void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryHuffmanBitsPlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!bits || misaligned(bits, 4)) return fail(DCTQ_EINVAL, "bits is NULL or not 4-byte aligned");
    // pixel planes only: the coefficients stay on chip (es.ps.coef stays NULL)
    dctq::EncodeSet es = {};
    int rc = dctq::plane_inputs(planes, nplanes, &es.ps);
    if (rc) return rc;
    if ((rc = number_blocks(&es, 1ll << 31, "2^31 blocks or more in one launch"))) return rc;
    HIPCHK(dctq::launch_huffman_from_pixels(es, plan->dev, plan->adaptive, bits, (hipStream_t)stream, plan->num_cus),
           "huffman_from_pixels launch");
    return DCTQ_OK;
}

int dctq_distortion_planes(const dctq_plan *plan, const dctq_plane *planes, int nplanes, uint32_t *sse,
                           void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryDistortionPlanes);
    if (int rc = dctq::check_plan(plan)) return rc;
    if (!sse || misaligned(sse, 4)) return fail(DCTQ_EINVAL, "sse is NULL or not 4-byte aligned");
    // pixel planes only: no coefficient, var_num or picture buffer (es.ps.coef / var stay NULL)
    dctq::EncodeSet es = {};
    int rc = dctq::plane_inputs(planes, nplanes, &es.ps);
    if (rc) return rc;
    if ((rc = number_blocks(&es, 1ll << 26, "more than 2^26 - 1 blocks in one launch"))) return rc;
    HIPCHK(dctq::launch_distortion(es, plan->dev, plan->adaptive, plan->inv_f32 != 0, sse, (hipStream_t)stream,
                                   plan->num_cus),
           "distortion launch");
    return DCTQ_OK;
}

// A source stack's own geometry: a stride that covers a row of row_bytes and, for more than one frame, a
// frame_stride that covers a frame; with `sizes`, width, height and nframes >= 1 first.  `what` names the stack.
static int stack_geometry(const char *what, bool sizes, int width, int height, int nframes, long long row_bytes,
                          long long stride, long long frame_stride) {
    const auto refuse = [&](const char *rule) { return fail(DCTQ_EINVAL, (std::string(what) + rule).c_str()); };
    if (sizes && (width < 1 || height < 1 || nframes < 1)) return refuse("width, height and nframes must be >= 1");
    if (stride < row_bytes) return refuse("stride smaller than one row");
    if (nframes > 1 && frame_stride < stride * (long long)height) return refuse("frame_stride smaller than one frame");
    return DCTQ_OK;
}

// The patch grid of ColorArgs or a PadPlane: per_row x rows patches a frame in raster order over nframes frames,
// fewer than 2^31 of them or the refusal `too_many`.
extern "C++" template <typename Args>
static int patch_grid(Args &a, long long per_row, long long rows, long long nframes, const char *too_many) {
    const long long per_frame = per_row * rows;
    if (per_frame * nframes >= (1ll << 31)) return fail(DCTQ_EINVAL, too_many);
    a.npatch = (uint32_t)(per_frame * nframes);
    a.per_row = (uint32_t)per_row;
    a.per_frame = (uint32_t)per_frame;
    a.div_row = dctq::make_fastdiv(a.per_row);
    a.div_frame = dctq::make_fastdiv(a.per_frame);
    return DCTQ_OK;
}

// The colour kernels' arguments from an RGB stack and its three planes, everything checked: *pixel_step and
// *s420 select the kernel.  The aligned entry points want the stack at dword alignment and of the Y plane's
// size.  any_size (the padding ones): the stack is the true W x H picture at any alignment, the planes are
// its extension to whole blocks, and *aligned says that it needs neither padding nor unaligned access, so
// that out->c describes the same call to the aligned kernels.
static int color_args(const dctq_rgb *rgb, const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr,
                      bool any_size, dctq::ColorPadArgs *out, int *pixel_step, bool *s420, bool *aligned) {
    if (!rgb || !rgb->pixels) return fail(DCTQ_EINVAL, "rgb/pixels is NULL");
    const int step = rgb->pixel_step;
    if (step != 1 && step != 3 && step != 4) return fail(DCTQ_EINVAL, "pixel_step must be 1, 3 or 4");
    const long long cs = rgb->channel_stride;
    const bool planar_dwords = step != 1 || cs % 4 == 0;
    if (step == 1 ? (cs == 0 || (!any_size && !planar_dwords)) : (cs != 1 && cs != -1))
        return fail(DCTQ_EINVAL, any_size ? "channel_stride must be +1 or -1 (interleaved) or non-zero (planar)"
                                          : "channel_stride must be +1 or -1 (interleaved) or a non-zero multiple of 4 "
                                            "(planar)");
    // the lowest byte of pixel (0,0): its B byte when the order is B, G, R
    uint8_t *first = (uint8_t *)rgb->pixels - (step != 1 && cs == -1 ? 2 : 0);
    const bool dwords = !misaligned(first, 4) && rgb->stride % 4 == 0 && rgb->frame_stride % 4 == 0;
    if (!any_size && !dwords)
        return fail(DCTQ_EINVAL, "rgb: the lowest byte of pixel (0,0) must be 4-byte aligned, stride and frame_stride "
                                 "multiples of 4");
    // sizes: only where they are the stack's own; otherwise they are the Y plane's, checked below
    if (int rc = stack_geometry("rgb: ", any_size, rgb->width, rgb->height, rgb->nframes, (long long)rgb->width * step,
                                rgb->stride, rgb->frame_stride))
        return rc;
    dctq::PlaneArgs py, pb, pr;
    if (int rc = dctq::plane_args(y, &py)) return rc;
    if (int rc = dctq::plane_args(cb, &pb)) return rc;
    if (int rc = dctq::plane_args(cr, &pr)) return rc;
    if (cb->width != cr->width || cb->height != cr->height) return fail(DCTQ_EINVAL, "Cb and Cr differ in size");
    const bool full = cb->width == y->width && cb->height == y->height;
    const bool half = 2ll * cb->width == y->width && 2ll * cb->height == y->height;
    if (!full && !half)
        return fail(DCTQ_EINVAL, "chroma must be luma's size (4:4:4) or exactly half of it in both directions (4:2:0)");
    const bool whole = rgb->width == y->width && rgb->height == y->height;
    const long long m = half ? 16 : 8;
    if (!any_size) {
        if (!whole) return fail(DCTQ_EINVAL, "the RGB stack and the Y plane differ in width or height");
    } else if (y->width != (rgb->width + m - 1) / m * m || y->height != (rgb->height + m - 1) / m * m) {
        return fail(DCTQ_EINVAL, "the Y plane is not the RGB stack's size rounded up to whole blocks (8, or 16 in 4:2:0)");
    }
    if (rgb->nframes != y->nframes || cb->nframes != y->nframes || cr->nframes != y->nframes)
        return fail(DCTQ_EINVAL, "the RGB stack and the planes differ in nframes");
    if (step == 1 && (cs < 0 ? -cs : cs) < rgb->width) return fail(DCTQ_EINVAL, "rgb: channel_stride smaller than one row");
    *out = {};
    dctq::ColorArgs &a = out->c;
    if (int rc = patch_grid(a, y->width / 8, y->height / (half ? 2 : 1), y->nframes, "2^31 patches or more in one call"))
        return rc;
    a.rgb = first;
    a.rgb_stride = rgb->stride;
    a.rgb_frame_stride = rgb->frame_stride;
    a.channel_stride = cs;
    a.swap = step != 1 && cs == -1;
    a.y = const_cast<uint8_t *>(y->pixels), a.y_stride = y->stride, a.y_frame_stride = y->frame_stride;
    a.cb = const_cast<uint8_t *>(cb->pixels), a.cb_stride = cb->stride, a.cb_frame_stride = cb->frame_stride;
    a.cr = const_cast<uint8_t *>(cr->pixels), a.cr_stride = cr->stride, a.cr_frame_stride = cr->frame_stride;
    out->width = (uint32_t)rgb->width;
    out->height = (uint32_t)rgb->height;
    *pixel_step = step;
    *s420 = half;
    *aligned = whole && dwords && planar_dwords;
    return DCTQ_OK;
}

// The four colour entry points: to_rgb is the direction, any_size as in color_args.
static int color_planes(bool to_rgb, bool any_size, const dctq_rgb *rgb, const dctq_plane *y, const dctq_plane *cb,
                        const dctq_plane *cr, void *stream) {
    dctq::ColorPadArgs a;
    int step;
    bool s420, aligned;
    if (int rc = color_args(rgb, y, cb, cr, any_size, &a, &step, &s420, &aligned)) return rc;
    if (aligned)  // always, for the aligned entry points; for the others the same bytes from the same kernels
        HIPCHK((to_rgb ? dctq::launch_ycc_to_rgb : dctq::launch_rgb_to_ycc)(a.c, step, s420, (hipStream_t)stream,
                                                                           device_cus()),
               to_rgb ? "ycc_to_rgb launch" : "rgb_to_ycc launch");
    else
        HIPCHK((to_rgb ? dctq::launch_ycc_to_rgb_crop : dctq::launch_rgb_to_ycc_pad)(a, step, s420, (hipStream_t)stream,
                                                                                    device_cus()),
               to_rgb ? "ycc_to_rgb_crop launch" : "rgb_to_ycc_pad launch");
    return DCTQ_OK;
}

int dctq_rgb_to_ycbcr_planes(const dctq_rgb *src, const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr,
                             void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRgbToYcbcrPlanes);
    return color_planes(false, false, src, y, cb, cr, stream);
}

int dctq_ycbcr_to_rgb_planes(const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr, const dctq_rgb *dst,
                             void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryYcbcrToRgbPlanes);
    return color_planes(true, false, dst, y, cb, cr, stream);
}

int dctq_rgb_to_ycbcr_pad_planes(const dctq_rgb *src, const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr,
                                 void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryRgbToYcbcrPadPlanes);
    return color_planes(false, true, src, y, cb, cr, stream);
}

int dctq_ycbcr_to_rgb_crop_planes(const dctq_plane *y, const dctq_plane *cb, const dctq_plane *cr, const dctq_rgb *dst,
                                  void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryYcbcrToRgbCropPlanes);
    return color_planes(true, true, dst, y, cb, cr, stream);
}

int dctq_pad_planes(const dctq_plane *src, const dctq_plane *dst, int nplanes, void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntryPadPlanes);
    if (!src || !dst) return fail(DCTQ_EINVAL, "src/dst is NULL");
    if (int rc = check_nplanes(nplanes)) return rc;
    dctq::PadSet ps = {};
    ps.n = nplanes;
    for (int k = 0; k < nplanes; ++k) {
        const dctq_plane &s = src[k], &d = dst[k];
        dctq::PlaneArgs pd;
        if (int rc = dctq::plane_args(&d, &pd)) return rc;
        if (!s.pixels) return fail(DCTQ_EINVAL, "src: pixels is NULL");
        if (int rc = stack_geometry("src: ", true, s.width, s.height, s.nframes, s.width, s.stride, s.frame_stride))
            return rc;
        if (d.width != (s.width + 7) / 8 * 8 || d.height != (s.height + 7) / 8 * 8 || d.nframes != s.nframes)
            return fail(DCTQ_EINVAL, "dst must be src's size rounded up to multiples of 8, with its nframes");
        for (int j = 0; j < nplanes; ++j)
            if (src[j].pixels == d.pixels) return fail(DCTQ_EINVAL, "src == dst: padding in place is not supported");
        dctq::PadPlane &p = ps.pl[k];
        if (int rc = patch_grid(p, d.width / 8, d.height, d.nframes, "2^31 patches or more in one plane")) return rc;
        p.src = s.pixels, p.src_stride = s.stride, p.src_frame_stride = s.frame_stride;
        p.dst = const_cast<uint8_t *>(d.pixels), p.dst_stride = d.stride, p.dst_frame_stride = d.frame_stride;
        p.width = (uint32_t)s.width, p.height = (uint32_t)s.height;
    }
    HIPCHK(dctq::launch_pad_planes(ps, (hipStream_t)stream, device_cus()), "pad_planes launch");
    return DCTQ_OK;
}

int dctq_device_count(int *count) {
    DCTQ_ENTRY;
    HIPCHK(hipGetDeviceCount(count), "hipGetDeviceCount");
    return DCTQ_OK;
}
int dctq_set_device(int device) {
    DCTQ_ENTRY;
    HIPCHK(hipSetDevice(device), "hipSetDevice");
    return DCTQ_OK;
}
int dctq_malloc(void **ptr, size_t bytes) {
    DCTQ_ENTRY;
    HIPCHK(hipMalloc(ptr, bytes), "hipMalloc");
    return DCTQ_OK;
}
int dctq_free(void *ptr) {
    DCTQ_ENTRY;
    HIPCHK(hipFree(ptr), "hipFree");
    return DCTQ_OK;
}
int dctq_memcpy_htod(void *dst, const void *src, size_t bytes) {
    DCTQ_ENTRY;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
    return DCTQ_OK;
}
int dctq_memcpy_dtoh(void *dst, const void *src, size_t bytes) {
    DCTQ_ENTRY;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    return DCTQ_OK;
}
int dctq_synchronize(void *stream) {
    DCTQ_LAUNCH(stream, dctq::kEntrySynchronize);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    return DCTQ_OK;
}

const char *dctq_error_string(int code) {
    if (code == DCTQ_OK) return "ok";
    if (!g_err.empty()) return g_err.c_str();
    switch (code) {
    case DCTQ_EINVAL: return "invalid argument";
    case DCTQ_EHIP: return "HIP runtime error";
    case DCTQ_ENOMEM: return "out of device memory";
    case DCTQ_ENODEV: return "no gfx950 device";
    default: return "unknown error";
    }
}

}  // extern "C"
