/*
 * host/frame_scaled.c -- a plain C99 host of the reduced-size decoder of the batched C-ABI
 * (include/dct_amd.h, dctq_decode_bits_window_scaled_planes): generates a synthetic Y/Cb/Cr
 * 4:2:0 frame on the device, encodes and packs the three planes ("bits v1"), and decodes a
 * window of each plane (everything but the first block column; in the luma, but the first
 * block row too) at 1 / 2^LOG2S size into buffers that were filled with a sentinel, each
 * picture at the minimum alignment: n = 8 >> LOG2S bytes into its buffer, with row padding of
 * 3 n bytes.  The yardstick is the header's definition, restated below in plain C on the
 * coefficients dctq_bits_decode gives for the same bytes, with the table quant_init builds.
 * Prints
 *   scaled_equal=1 padding_intact=1 abi_version=6
 * and exits non-zero if either flag is 0.
 *
 *   frame_scaled WIDTH HEIGHT QUALITY ADAPTIVE SEED KIND LOG2S
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dct_amd.h"
#include "quantization.h"

#define CHK(x)                                                                  \
    do {                                                                        \
        int rc_ = (x);                                                          \
        if (rc_) {                                                              \
            fprintf(stderr, "%s: %s\n", #x, dctq_error_string(rc_));            \
            return 1;                                                           \
        }                                                                       \
    } while (0)

#define SENTINEL 0xA5

static const double D1[1][1] = {{1.0}};
static const double D2[2][2] = {{0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bcdp-1}, {0x1.6a09e667f3bcdp-1, -0x1.6a09e667f3bcdp-1}};
static const double D4[4][4] = {{0.5, 0.5, 0.5, 0.5},
                                {0x1.4e7ae9144f0fcp-1, 0x1.1517a7bdb3896p-2, -0x1.1517a7bdb3896p-2, -0x1.4e7ae9144f0fcp-1},
                                {0.5, -0.5, -0.5, 0.5},
                                {0x1.1517a7bdb3896p-2, -0x1.4e7ae9144f0fcp-1, 0x1.4e7ae9144f0fcp-1, -0x1.1517a7bdb3896p-2}};

static double dn(int n, int u, int i) { return n == 4 ? D4[u][i] : n == 2 ? D2[u][i] : D1[u][i]; }

/* the n x n pixels of one block, by the definition of include/dct_amd.h */
static void block_pixels(const int16_t *q, double **Q, int n, int adaptive, int32_t var_num, uint8_t out[4][4]) {
    double x[4][4], temp[4][4];
    const double sc = 2.0 - fmin(1.0, fmax(0.1, ((double)var_num / 4096.0) / 1000.0));
    for (int u = 0; u < n; ++u)
        for (int v = 0; v < n; ++v) {
            const double c = (double)q[8 * u + v];
            if (!adaptive) x[u][v] = c * (1.0 / Q[u][v]);
            else x[u][v] = (u | v) ? (c * Q[u][v]) * sc : c * Q[u][v];
        }
    for (int u = 0; u < n; ++u)
        for (int j = 0; j < n; ++j) {
            double s = x[u][0] * dn(n, 0, j);
            for (int v = 1; v < n; ++v) s = s + x[u][v] * dn(n, v, j);
            temp[u][j] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = dn(n, 0, i) * temp[0][j];
            for (int u = 1; u < n; ++u) s = s + dn(n, u, i) * temp[u][j];
            const double r = s * (n / 8.0) + 128.0;
            out[i][j] = (uint8_t)rint(fmin(fmax(r, 0.0), 255.0));
        }
}

int main(int argc, char **argv) {
    if (argc < 8) {
        fprintf(stderr, "usage: %s W H QUALITY ADAPTIVE SEED KIND LOG2S\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[1]), h = atoi(argv[2]), q = atoi(argv[3]), ad = atoi(argv[4]);
    const uint64_t seed = strtoull(argv[5], NULL, 10);
    const int kind = atoi(argv[6]), log2s = atoi(argv[7]);
    if (w < 32 || h < 32 || w % 16 || h % 16 || log2s < 1 || log2s > 3) {
        fprintf(stderr, "W and H must be multiples of 16 and >= 32, LOG2S 1, 2 or 3\n");
        return 2;
    }
    const int n = 8 >> log2s;
    const int pw[3] = {w, w / 2, w / 2}, ph[3] = {h, h / 2, h / 2};
    const int x0[3] = {8, 8, 8}, y0[3] = {8, 0, 0};
    long long nb[3], first[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        nb[k] = (long long)(pw[k] / 8) * (ph[k] / 8);
        first[k + 1] = first[k] + nb[k];
    }
    const long long nblk = first[3], cap = 64 * nblk;

    void *px[3], *coef, *var, *off, *sym, *ws, *boff, *bws, *bytes, *back, *out[3];
    dctq_plane src[3], dst[3];
    dctq_window win[3];
    uint8_t *hout[3];
    size_t osize[3];
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_malloc(&px[k], (size_t)pw[k] * ph[k]));
        src[k].pixels = (const uint8_t *)px[k];
        src[k].stride = pw[k];
        src[k].frame_stride = (long long)pw[k] * ph[k];
        src[k].width = pw[k];
        src[k].height = ph[k];
        src[k].nframes = 1;
        CHK(dctq_synth(seed + (uint64_t)k, kind, &src[k], NULL));
        win[k].width = pw[k];
        win[k].height = ph[k];
        win[k].nframes = 1;
        win[k].x0 = x0[k];
        win[k].y0 = y0[k];
        win[k].frame0 = 0;
        dst[k].width = (pw[k] - x0[k]) >> log2s;
        dst[k].height = (ph[k] - y0[k]) >> log2s;
        dst[k].nframes = 1;
        dst[k].stride = dst[k].width + 3 * n;
        dst[k].frame_stride = dst[k].stride * dst[k].height;
        osize[k] = (size_t)n + (size_t)dst[k].frame_stride + 32;
        hout[k] = malloc(osize[k]);
        if (!hout[k]) return 1;
        memset(hout[k], SENTINEL, osize[k]);
        CHK(dctq_malloc(&out[k], osize[k]));
        CHK(dctq_memcpy_htod(out[k], hout[k], osize[k]));
        dst[k].pixels = (const uint8_t *)out[k] + n;
    }
    CHK(dctq_malloc(&coef, (size_t)nblk * 128));
    CHK(dctq_malloc(&back, (size_t)nblk * 128));
    CHK(dctq_malloc(&var, (size_t)nblk * 4));
    CHK(dctq_malloc(&off, (size_t)(nblk + 1) * 4));
    CHK(dctq_malloc(&boff, (size_t)(nblk + 1) * 4));
    CHK(dctq_malloc(&sym, (size_t)cap * 4));
    CHK(dctq_malloc(&ws, dctq_encode_workspace_bytes(nblk)));
    CHK(dctq_malloc(&bws, dctq_bits_workspace_bytes(nblk)));
    dctq_plan *plan;
    CHK(dctq_plan_create(q, ad, &plan));

    int16_t *cp[3];
    int32_t *vw[3];
    const int32_t *vn[3];
    for (int k = 0; k < 3; ++k) {
        cp[k] = (int16_t *)coef + 64 * first[k];
        vw[k] = (int32_t *)var + first[k];
        vn[k] = vw[k];
    }
    CHK(dctq_forward_quant_planes(plan, src, 3, cp, vw, NULL));
    CHK(dctq_encode_planes(plan, src, 3, cp, (uint32_t *)off, (uint32_t *)sym, cap, ws, NULL));
    uint32_t bytes_total = 0;
    CHK(dctq_bits_pack(sym, 4, (const uint32_t *)off, nblk, (uint32_t *)boff, NULL, 0, bws, NULL));
    CHK(dctq_synchronize(NULL));
    CHK(dctq_memcpy_dtoh(&bytes_total, (const uint32_t *)boff + nblk, 4));
    CHK(dctq_malloc(&bytes, (size_t)bytes_total + 4));
    CHK(dctq_bits_pack(sym, 4, (const uint32_t *)off, nblk, (uint32_t *)boff, (uint8_t *)bytes, (long long)bytes_total,
                       bws, NULL));

    CHK(dctq_decode_bits_window_scaled_planes(plan, (const uint8_t *)bytes, (const uint32_t *)boff, ad ? vn : NULL, win,
                                              dst, 3, log2s, NULL));
    CHK(dctq_bits_decode((const uint8_t *)bytes, (const uint32_t *)boff, nblk, (int16_t *)back, NULL));
    CHK(dctq_synchronize(NULL));

    int16_t *hcoef = malloc((size_t)nblk * 128);
    int32_t *hvar = malloc((size_t)nblk * 4);
    if (!hcoef || !hvar) return 1;
    CHK(dctq_memcpy_dtoh(hcoef, back, (size_t)nblk * 128));
    CHK(dctq_memcpy_dtoh(hvar, var, (size_t)nblk * 4));
    QuantContext *ctx = quant_init(8, q, ad);
    if (!ctx) return 1;

    int equal = 1, intact = 1;
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_memcpy_dtoh(hout[k], out[k], osize[k]));
        uint8_t *own = calloc(osize[k], 1);
        if (!own) return 1;
        const int bw = pw[k] / 8;
        for (int by = y0[k] / 8; by < ph[k] / 8; ++by)
            for (int bx = x0[k] / 8; bx < bw; ++bx) {
                const long long b = first[k] + (long long)by * bw + bx;
                uint8_t pix[4][4];
                block_pixels(hcoef + 64 * b, ctx->quant_matrix, n, ad, hvar[b], pix);
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) {
                        const size_t at = (size_t)n + (size_t)((by - y0[k] / 8) * n + i) * (size_t)dst[k].stride +
                                          (size_t)((bx - x0[k] / 8) * n + j);
                        equal &= hout[k][at] == pix[i][j];
                        own[at] = 1;
                    }
            }
        for (size_t i = 0; i < osize[k]; ++i)
            if (!own[i]) intact &= hout[k][i] == SENTINEL;
        free(own);
    }
    printf("scaled_equal=%d padding_intact=%d abi_version=%d\n", equal, intact, dctq_abi_version());

    quant_free(ctx);
    dctq_plan_destroy(plan);
    for (int k = 0; k < 3; ++k) {
        dctq_free(px[k]);
        dctq_free(out[k]);
        free(hout[k]);
    }
    free(hcoef);
    free(hvar);
    dctq_free(coef);
    dctq_free(back);
    dctq_free(var);
    dctq_free(off);
    dctq_free(boff);
    dctq_free(sym);
    dctq_free(ws);
    dctq_free(bws);
    dctq_free(bytes);
    return equal && intact ? 0 : 1;
}
