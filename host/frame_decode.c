/*
 * host/frame_decode.c -- a plain C99 host of the decoder chain of the batched
 * C-ABI (include/dct_amd.h), symbols -> pixels in three calls: generates a
 * synthetic frame on the device, encodes it (dctq_encode_planes16 where the plan
 * admits 2-byte symbols, dctq_encode_planes otherwise), then decodes the symbols
 * (dctq_rle_decode16 / dctq_rle_decode) and the coefficients
 * (dctq_decode_planes) into a u8 plane with padded rows, copies that plane back
 * (one byte per pixel, not 256 per block) and prints
 *   abi_version     dctq_abi_version()
 *   pixels_fnv1a    64-bit FNV-1a of the decoded WIDTH x HEIGHT bytes, row by row
 *   padding_intact  1 if no byte of the row padding was written
 *   psnr_u8         PSNR of the decoded against the original pixels
 *                   (tests/test_entropy.c:376-393 formula)
 * An adaptive plan's decoder needs each block's var_num as side information; it
 * comes from dctq_forward_quant here.
 *
 *   frame_decode WIDTH HEIGHT QUALITY ADAPTIVE SEED [KIND]
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dct_amd.h"

#define CHK(x)                                                                  \
    do {                                                                        \
        int rc_ = (x);                                                          \
        if (rc_) {                                                              \
            fprintf(stderr, "%s: %s\n", #x, dctq_error_string(rc_));            \
            return 1;                                                           \
        }                                                                       \
    } while (0)

#define SENTINEL 0xA5

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s W H QUALITY ADAPTIVE SEED [KIND]\n", argv[0]);
        return 2;
    }
    int w = atoi(argv[1]), h = atoi(argv[2]), q = atoi(argv[3]), ad = atoi(argv[4]);
    uint64_t seed = strtoull(argv[5], NULL, 10);
    int kind = argc > 6 ? atoi(argv[6]) : 0;
    if (w < 8 || h < 8 || w % 8 || h % 8) {
        fprintf(stderr, "W and H must be positive multiples of 8\n");
        return 2;
    }
    const long long nblk = (long long)(w / 8) * (h / 8);
    const long long cap = 64 * nblk;
    const long long stride = (long long)w + 64;  /* 64 bytes of padding after every row */
    const size_t padded = (size_t)stride * h;

    void *px, *coef, *var, *off, *sym, *ws, *coef2, *out;
    CHK(dctq_malloc(&px, (size_t)w * h));
    CHK(dctq_malloc(&coef, (size_t)nblk * 128));
    CHK(dctq_malloc(&var, (size_t)nblk * 4));
    CHK(dctq_malloc(&off, (size_t)(nblk + 1) * 4));
    CHK(dctq_malloc(&sym, (size_t)cap * 4));
    CHK(dctq_malloc(&ws, dctq_encode_workspace_bytes(nblk)));
    CHK(dctq_malloc(&coef2, (size_t)nblk * 128));
    CHK(dctq_malloc(&out, padded));
    dctq_plane pl = {NULL, 0, 0, 0, 0, 1};
    pl.pixels = (const uint8_t *)px;
    pl.stride = w;
    pl.frame_stride = (long long)w * h;
    pl.width = w;
    pl.height = h;
    CHK(dctq_synth(seed, kind, &pl, NULL));
    dctq_plan *plan;
    CHK(dctq_plan_create(q, ad, &plan));

    /* encoder side: symbols (+ var_num, the adaptive decoder's side information) */
    int16_t *cp = (int16_t *)coef;
    if (ad) CHK(dctq_forward_quant(plan, &pl, cp, (int32_t *)var, NULL));
    const int symbytes = dctq_plan_symbol_bytes(plan);
    if (symbytes == 2)
        CHK(dctq_encode_planes16(plan, &pl, 1, &cp, (uint32_t *)off, (uint16_t *)sym, cap, ws, NULL));
    else
        CHK(dctq_encode_planes(plan, &pl, 1, &cp, (uint32_t *)off, (uint32_t *)sym, cap, ws, NULL));

    /* decoder side: symbols -> coefficients -> pixels, into a plane with padded rows */
    uint8_t *hout = malloc(padded);
    uint8_t *hpx = malloc((size_t)w * h);
    if (!hout || !hpx) return 1;
    memset(hout, SENTINEL, padded);
    CHK(dctq_memcpy_htod(out, hout, padded));
    if (symbytes == 2)
        CHK(dctq_rle_decode16((const uint16_t *)sym, (const uint32_t *)off, nblk, (int16_t *)coef2, NULL));
    else
        CHK(dctq_rle_decode((const uint32_t *)sym, (const uint32_t *)off, nblk, (int16_t *)coef2, NULL));
    dctq_plane dst = {NULL, 0, 0, 0, 0, 1};
    dst.pixels = (const uint8_t *)out;
    dst.stride = stride;
    dst.frame_stride = (long long)padded;
    dst.width = w;
    dst.height = h;
    const int16_t *c2 = (const int16_t *)coef2;
    const int32_t *vn = (const int32_t *)var;
    CHK(dctq_decode_planes(plan, &c2, ad ? &vn : NULL, &dst, 1, NULL));
    CHK(dctq_synchronize(NULL));
    CHK(dctq_memcpy_dtoh(hout, out, padded));
    CHK(dctq_memcpy_dtoh(hpx, px, (size_t)w * h));

    uint64_t fnv = 1469598103934665603ULL;
    int intact = 1;
    double se = 0.0;
    for (int y = 0; y < h; ++y) {
        const uint8_t *row = hout + (size_t)y * (size_t)stride;
        for (int x = 0; x < w; ++x) {
            fnv = (fnv ^ row[x]) * 1099511628211ULL;
            double d = (double)hpx[(size_t)y * w + x] - (double)row[x];
            se += d * d;
        }
        for (long long x = w; x < stride; ++x) intact &= row[x] == SENTINEL;
    }
    const double mse = se / ((double)w * h);
    printf("abi_version:%d\n", dctq_abi_version());
    printf("pixels_fnv1a:%016llx\n", (unsigned long long)fnv);
    printf("padding_intact:%d\n", intact);
    if (mse > 0.0)
        printf("psnr_u8:%.4f\n", 10.0 * log10(255.0 * 255.0 / mse));
    else
        printf("psnr_u8:inf\n");

    dctq_plan_destroy(plan);
    dctq_free(px);
    dctq_free(coef);
    dctq_free(var);
    dctq_free(off);
    dctq_free(sym);
    dctq_free(ws);
    dctq_free(coef2);
    dctq_free(out);
    free(hout);
    free(hpx);
    return 0;
}
