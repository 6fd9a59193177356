// dct_amd/csrc/plan_tables.hip -- a plan's tables and their error bounds, and the plan
// entry points of include/dct_amd.h.
//
// D of src/dct.c:17-30 and Q of src/quantization.c:51-99 come from the reference's own
// expressions (host_tables.h), so the exact tie path sees bit-identical constants; the
// fast path's scale and guard tables from the proven bound in fdct8_bound.h; the fp32
// inverse's admission from idct8_bound.h.  Compiled with -ffp-contract=off, so host
// arithmetic is the reference's.
#include <math.h>
#include <string.h>

#include "dct_amd.h"
#include "dctq_diag.h"
#include "dctq_internal.h"
#include "fdct8_bound.h"
#include "host_tables.h"
#include "idct8_bound.h"
#include "plan.h"

using dctq::fail;

namespace dctq {
FastDiv make_fastdiv(uint32_t d) {
    uint32_t s = 0;
    while ((1ull << s) < d) ++s;
    const uint64_t m = ((1ull << 32) * ((1ull << s) - d)) / d + 1;
    return FastDiv{d, (uint32_t)m, s};
}

// Guard band of the fast path (DESIGN.md "Exactness").  With Y~ the fp32
// butterfly output (|Y~ - Y| <= kErrY), w~ = fl32(S_i S_j / Q) and
// f~ = fl(Y~ w~ - r) for r = rint(Y~ w~), the reference's quotient V = fl(ref / M)
// satisfies |V - (r + f~)| <= B below; hence |f~| <= 0.5 - B  =>  round(V) == r.
void fill_fast_tables(const double *q, int adaptive, FastTables *t) {
    const double u = 0x1p-24;
    // scale-factor representation: fl32(w) (0.5u) and its product (0.5u); adaptive
    // plans also the kernel's 1/(2-nv) = v_rcp_f32(fl32(2-nv)) (0.5u + 2u, fdct8_core.h)
    const double rel = adaptive ? 4.5 * u + 0x1p-48 : u + 0x1p-48;
    for (int c = 0; c < 64; ++c) {
        const int i = c >> 3, j = c & 7;
        const double w = kAanScale[i] * kAanScale[j] / q[c];
        const float wf = (float)w;
        const double wt = (double)wf;
        const double B = 0x1p-25                        /* rounding of f~ */
                         + kErrY[c] * wt * (1.0 + 4.0 * u) /* butterfly error, scaled */
                         + kMaxY[c] * w * rel           /* scale-factor representation */
                         + 1e-9 / q[c]                  /* reference's own fp64 error (< 1e-11) */
                         + (kMaxY[c] * w + 1.0) * 0x1p-52; /* reference's division rounding */
        double thr = (0.5 - B) * (1.0 - 0x1p-20);
        float tf = (float)thr;
        if ((double)tf > thr) tf = nextafterf(tf, 0.0f);
        t->w[c] = wf;
        t->thr[c] = tf;
        const double tt = (double)tf * (double)tf;  // exact
        float t2 = (float)tt;
        if ((double)t2 > tt) t2 = nextafterf(t2, 0.0f);
        t->thr2[c] = t2;
    }
    for (int p = 0; p < 64; ++p) {
        const int c = (((p >> 1) & 7) << 3) + ((p >> 4) << 1) + (p & 1);
        t->ws[p] = t->w[c];
        t->t2s[p] = t->thr2[c];
    }
}
}  // namespace dctq

// Quantized DC of a constant block, exactly as the reference computes it:
// temp[k][0] = sum_l x * D[0][l] (the same for every row k, l ascending), then
// out = sum_k D[0][k] * temp[k][0], q = (int) round(out / Q[0]).  This file is
// compiled with -ffp-contract=off, so host arithmetic is the reference's.
void dctq::dc_const_table(const double *d, const double *q, int16_t *tab) {
    for (int v = 0; v < 256; ++v) {
        const double x = (double)v - 128.0;
        double t = 0.0;
        for (int l = 0; l < 8; ++l) t += x * d[l];
        double out = 0.0;
        for (int k = 0; k < 8; ++k) out += d[k] * t;
        tab[v] = (int16_t)(int)round(out / q[0]);
    }
}

// The fused round trip's fp32 inverse is admitted for a non-adaptive plan when the
// rigorous bound of tools/inv_bound.py (idct8_bound.h) keeps |recon - reference|
// within kInvTol (5e-5, half of north_star's 1e-4) for every block of u8 pixels, i.e.
// every coefficient block inside the plan's forward range (NOT every int16 block a
// decoder may be handed: outside the range the same bound, evaluated at the block's own
// magnitudes, grows linearly -- tools/inv_bound.py block_error, include/dct_amd.h):
// |c_uv| <= 128 L1(D_u) L1(D_v) for centred pixels, so |q_uv| <= round(c_max / Q)
// and |x_uv| <= B_uv = |q|max * (1/Q) * S_u S_v (the reference's 1/Q dequantisation,
// src/quantization.c:139,144); per output pixel the bound is G.B (1 + u) + u (128 + |L|.B)
// (the final + 128 rounding) + 1e-9 (the reference's own fp64 error).
static_assert(kInvTol == kInvTolDiag, "plan.h's copy of the fp32 inverse's admission tolerance");
// |q_k|max of every coefficient for u8 input: |c_uv| <= 128 L1(D_u) L1(D_v) for centred
// pixels, so |q_uv| <= round(c_max / Q_uv).
static void max_quantized(const dctq::DevTables &t, double (&qmax)[64]) {
    double l1[8];
    for (int r = 0; r < 8; ++r) {
        l1[r] = 0.0;
        for (int c = 0; c < 8; ++c) l1[r] += fabs(t.dct[r * 8 + c]);
    }
    for (int k = 0; k < 64; ++k) {
        const double cmax = 128.0 * l1[k >> 3] * l1[k & 7] * (1.0 + 1e-12);
        qmax[k] = floor(cmax / t.quant[k] + 0.5 + 1e-9);
    }
}

double dctq::inverse_f32_bound(const dctq::DevTables &t) {
    const double u = 1.0 / 16777216.0;
    double qmax[64], B[64];
    max_quantized(t, qmax);
    for (int k = 0; k < 64; ++k) B[k] = qmax[k] * t.dequant[k] * t.s2[k] * (1.0 + 1e-12);
    double worst = 0.0;
    for (int p = 0; p < 64; ++p) {
        double g = 0.0, a = 0.0;
        for (int k = 0; k < 64; ++k) {
            g += kInvErrG[p][k] * B[k];
            a += kInvAbsL[p][k] * B[k];
        }
        const double e = g * (1.0 + u) + u * (128.0 + a) + 1e-9;
        worst = e > worst ? e : worst;
    }
    return worst;
}

int dctq::max_abs_quantized(const dctq::DevTables &t) {
    double qmax[64];
    max_quantized(t, qmax);
    int m = 0;
    for (int k = 0; k < 64; ++k) m = (int)qmax[k] > m ? (int)qmax[k] : m;
    return m;
}

static int build_plan(const double *q, int quality, int adaptive, dctq_plan **out) {
    if (!out) return fail(DCTQ_EINVAL, "plan pointer is NULL");
    for (int c = 0; c < 64; ++c)
        if (!(q[c] >= 1.0 && q[c] <= 65535.0)) return fail(DCTQ_EINVAL, "quant_matrix entries must lie in [1, 65535]");
    int dev = 0, arch_ok = 0;
    HIPCHK(hipGetDevice(&dev), "hipGetDevice");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
    arch_ok = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    if (!arch_ok) return fail(DCTQ_ENODEV, "libdct_amd is built for gfx950 (MI355X) only");
    dctq_plan *p = new dctq_plan();
    p->quality = quality;
    p->adaptive = adaptive ? 1 : 0;
    p->device = dev;
    p->num_cus = prop.multiProcessorCount;
    p->variant = 2;  // the product kernels; dctq_diag_* entry points (libdct_amd_diag.so) can force another
    p->fallbacks = nullptr;
    dctq_host::dct_matrix(8, p->host.dct);
    for (int c = 0; c < 64; ++c) {
        const double s2 = kAanScale[c >> 3] * kAanScale[c & 7];
        p->host.quant[c] = q[c];
        p->host.dequant[c] = 1.0 / q[c];
        p->host.s2[c] = s2;
        p->host.iscale[c] = p->host.dequant[c] * s2;
        p->host.qscale[c] = q[c] * s2;
    }
    dctq::fill_fast_tables(q, p->adaptive, &p->fast);
    dctq::dc_const_table(p->host.dct, p->host.quant, p->host.dc_const);
    for (int k = 0; k < 8; ++k) p->host.s1[k] = kAanScale[k];
    for (int c = 0; c < 64; ++c) p->host.iscale32[c] = (float)p->host.iscale[c];
    p->inv_bound = dctq::inverse_f32_bound(p->host);
    p->inv_f32 = !p->adaptive && p->inv_bound <= kInvTol;
    p->symbol_bytes = dctq::max_abs_quantized(p->host) <= 511 ? 2 : 4;
    p->host.fast = p->fast;
    hipError_t e = hipMalloc(&p->dev, sizeof(dctq::DevTables));
    if (e != hipSuccess) {
        delete p;
        return fail(DCTQ_ENOMEM, "hipMalloc(plan tables)", e);
    }
    e = hipMemcpy(p->dev, &p->host, sizeof(dctq::DevTables), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p->dev);
        delete p;
        return fail(DCTQ_EHIP, "hipMemcpy(plan tables)", e);
    }
    *out = p;
    return DCTQ_OK;
}

extern "C" {

int dctq_plan_create(int quality, int adaptive, dctq_plan **plan) {
    DCTQ_ENTRY;
    double q[64];
    quality = dctq_host::clamp_quality(quality);
    dctq_host::quant_matrix(8, quality, q);
    return build_plan(q, quality, adaptive, plan);
}

int dctq_plan_from_context(const QuantContext *qctx, dctq_plan **plan) {
    DCTQ_ENTRY;
    if (!qctx || qctx->block_size != 8 || !qctx->quant_matrix) return fail(DCTQ_EINVAL, "QuantContext must be 8x8");
    double q[64];
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) q[i * 8 + j] = qctx->quant_matrix[i][j];
    return build_plan(q, qctx->quality, qctx->adaptive, plan);
}

void dctq_plan_destroy(dctq_plan *plan) {
    DCTQ_ENTRY;
    if (!plan) return;
    (void)hipFree(plan->dev);
    delete plan;
}

int dctq_plan_set_fallback_counter(dctq_plan *plan, unsigned long long *counter) {
    DCTQ_ENTRY;
    if (!plan) return fail(DCTQ_EINVAL, "plan is NULL");
    plan->fallbacks = counter;
    return DCTQ_OK;
}

}  // extern "C"
