/*
 * host/frame_rgb.c -- a plain C99 host of the whole device path from a picture to bytes
 * and back, over the batched C-ABI only (include/dct_amd.h):
 *   1. an interleaved RGB frame stack (three dctq_synth planes of different seeds,
 *      interleaved on the host) is uploaded;
 *   2. dctq_rgb_to_ycbcr_planes makes its Y, Cb, Cr planes (4:2:0);
 *   3. dctq_encode_planes + dctq_bits_pack make the packed stream;
 *   4. dctq_decode_bits_planes decodes it into planes;
 *   5. dctq_ycbcr_to_rgb_planes writes the decoded picture into an RGB buffer with padded
 *      rows and a gap between frames, filled with a sentinel beforehand
 * -- and prints key:value lines:
 *   abi_version      dctq_abi_version()
 *   ycc_equal        1 if the planes of step 2 equal the formulas of include/dct_amd.h,
 *                    restated below, applied to the picture on the host
 *   rgb_equal        1 if the picture of step 5 equals the inverse formulas applied to the
 *                    decoded planes of step 4
 *   padding_intact   1 if step 5 wrote no byte outside width x height of a frame
 *   bytes_total      bytes of the packed stream
 *   bytes_per_pixel  bytes_total / (W * H * FRAMES)
 * It exits non-zero if any of the three flags is 0.
 *
 *   frame_rgb WIDTH HEIGHT FRAMES [QUALITY ADAPTIVE SEED KIND]
 */
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
#define PAD 20   /* bytes of padding after every RGB row (a multiple of 4) */
#define GAP 128  /* bytes between RGB frames */

static int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

/* floor(v / 2^16) for any int: >> of a negative int is implementation-defined in C99 */
static int shr16(int v) { return v >= 0 ? v >> 16 : -((-v + 65535) >> 16); }

static void ycc_of(const uint8_t *p, int *y, int *cb, int *cr) {
    const int r = p[0], g = p[1], b = p[2];
    *y = shr16(19595 * r + 38470 * g + 7471 * b + 32768);
    *cb = shr16(-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767);
    *cr = shr16(32768 * r - 27439 * g - 5329 * b + 8388608 + 32767);
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s W H FRAMES [QUALITY ADAPTIVE SEED KIND]\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[1]), h = atoi(argv[2]), nf = atoi(argv[3]);
    const int q = argc > 4 ? atoi(argv[4]) : 50, ad = argc > 5 ? atoi(argv[5]) : 0;
    const uint64_t seed = argc > 6 ? strtoull(argv[6], NULL, 10) : 1;
    const int kind = argc > 7 ? atoi(argv[7]) : 1;
    if (w < 16 || h < 16 || w % 16 || h % 16 || nf < 1) {
        fprintf(stderr, "W and H must be positive multiples of 16 (4:2:0 chroma in 8x8 blocks), FRAMES >= 1\n");
        return 2;
    }
    const int pw[3] = {w, w / 2, w / 2}, ph[3] = {h, h / 2, h / 2};
    long long nb[3], first[4] = {0, 0, 0, 0};
    size_t psize[3];
    for (int k = 0; k < 3; ++k) {
        nb[k] = (long long)(pw[k] / 8) * (ph[k] / 8) * nf;
        first[k + 1] = first[k] + nb[k];
        psize[k] = (size_t)pw[k] * ph[k] * nf;
    }
    const long long nblk = first[3], cap = 64 * nblk;
    const size_t npix = psize[0];

    /* 1. the picture: channel c is a synthetic plane of its own seed */
    void *chan, *rgb_in;
    uint8_t *hchan = malloc(npix), *hrgb = malloc(3 * npix);
    if (!hchan || !hrgb) return 1;
    CHK(dctq_malloc(&chan, npix));
    CHK(dctq_malloc(&rgb_in, 3 * npix));
    dctq_plane cpl;
    cpl.pixels = (const uint8_t *)chan;
    cpl.stride = w;
    cpl.frame_stride = (long long)w * h;
    cpl.width = w;
    cpl.height = h;
    cpl.nframes = nf;
    for (int c = 0; c < 3; ++c) {
        CHK(dctq_synth(seed + 1000u * (uint64_t)c, kind, &cpl, NULL));
        CHK(dctq_synchronize(NULL));
        CHK(dctq_memcpy_dtoh(hchan, chan, npix));
        for (size_t i = 0; i < npix; ++i) hrgb[3 * i + c] = hchan[i];
    }
    CHK(dctq_memcpy_htod(rgb_in, hrgb, 3 * npix));
    dctq_rgb src;
    src.pixels = rgb_in;
    src.stride = 3ll * w;
    src.frame_stride = 3ll * w * h;
    src.channel_stride = 1;
    src.pixel_step = 3;
    src.width = w;
    src.height = h;
    src.nframes = nf;

    /* 2. RGB -> Y, Cb, Cr (4:2:0) */
    void *pl[3], *dec[3];
    dctq_plane ycc[3], out[3];
    uint8_t *hpl[3], *hdec[3];
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_malloc(&pl[k], psize[k]));
        CHK(dctq_malloc(&dec[k], psize[k]));
        hpl[k] = malloc(psize[k]);
        hdec[k] = malloc(psize[k]);
        if (!hpl[k] || !hdec[k]) return 1;
        ycc[k].pixels = (const uint8_t *)pl[k];
        ycc[k].stride = pw[k];
        ycc[k].frame_stride = (long long)pw[k] * ph[k];
        ycc[k].width = pw[k];
        ycc[k].height = ph[k];
        ycc[k].nframes = nf;
        out[k] = ycc[k];
        out[k].pixels = (const uint8_t *)dec[k];
    }
    CHK(dctq_rgb_to_ycbcr_planes(&src, &ycc[0], &ycc[1], &ycc[2], NULL));

    /* 3. planes -> symbols -> packed bytes */
    void *coef, *var, *off, *sym, *ws, *boff, *bws, *bytes;
    CHK(dctq_malloc(&coef, (size_t)nblk * 128));
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
    if (ad) CHK(dctq_forward_quant_planes(plan, ycc, 3, cp, vw, NULL));
    CHK(dctq_encode_planes(plan, ycc, 3, cp, (uint32_t *)off, (uint32_t *)sym, cap, ws, NULL));
    uint32_t bytes_total = 0;
    CHK(dctq_bits_pack(sym, 4, (const uint32_t *)off, nblk, (uint32_t *)boff, NULL, 0, bws, NULL));
    CHK(dctq_synchronize(NULL));
    CHK(dctq_memcpy_dtoh(&bytes_total, (const uint32_t *)boff + nblk, 4));
    CHK(dctq_malloc(&bytes, ((size_t)bytes_total + 3) / 4 * 4 + 4));
    CHK(dctq_bits_pack(sym, 4, (const uint32_t *)off, nblk, (uint32_t *)boff, (uint8_t *)bytes,
                       (long long)bytes_total, bws, NULL));

    /* 4. packed bytes -> decoded planes */
    CHK(dctq_decode_bits_planes(plan, (const uint8_t *)bytes, (const uint32_t *)boff, ad ? vn : NULL, out, 3, NULL));

    /* 5. decoded planes -> RGB, rows and frames padded */
    const size_t ostride = 3 * (size_t)w + PAD, oframe = ostride * h + GAP, osize = oframe * nf;
    void *rgb_out;
    uint8_t *hout = malloc(osize);
    if (!hout) return 1;
    memset(hout, SENTINEL, osize);
    CHK(dctq_malloc(&rgb_out, osize));
    CHK(dctq_memcpy_htod(rgb_out, hout, osize));
    dctq_rgb dst = src;
    dst.pixels = rgb_out;
    dst.stride = (long long)ostride;
    dst.frame_stride = (long long)oframe;
    CHK(dctq_ycbcr_to_rgb_planes(&out[0], &out[1], &out[2], &dst, NULL));
    CHK(dctq_synchronize(NULL));
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_memcpy_dtoh(hpl[k], pl[k], psize[k]));
        CHK(dctq_memcpy_dtoh(hdec[k], dec[k], psize[k]));
    }
    CHK(dctq_memcpy_dtoh(hout, rgb_out, osize));

    int ycc_equal = 1, rgb_equal = 1, intact = 1;
    for (int f = 0; f < nf; ++f) {
        const uint8_t *fr = hrgb + (size_t)f * 3 * w * h;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                int yy, cb, cr;
                ycc_of(fr + 3 * ((size_t)y * w + x), &yy, &cb, &cr);
                ycc_equal &= hpl[0][((size_t)f * h + y) * w + x] == yy;
            }
        for (int y = 0; y < h / 2; ++y)
            for (int x = 0; x < w / 2; ++x) {
                int sb = 2, sr = 2;
                for (int j = 0; j < 4; ++j) {
                    int yy, cb, cr;
                    ycc_of(fr + 3 * ((size_t)(2 * y + j / 2) * w + 2 * x + j % 2), &yy, &cb, &cr);
                    sb += cb;
                    sr += cr;
                }
                const size_t at = ((size_t)f * (h / 2) + y) * (w / 2) + x;
                ycc_equal &= hpl[1][at] == sb >> 2 && hpl[2][at] == sr >> 2;
            }
        const uint8_t *of = hout + (size_t)f * oframe;
        for (int y = 0; y < h; ++y) {
            for (int x = 0; x < w; ++x) {
                const size_t at = ((size_t)f * (h / 2) + y / 2) * (w / 2) + x / 2;
                const int yy = hdec[0][((size_t)f * h + y) * w + x], cb = hdec[1][at] - 128, cr = hdec[2][at] - 128;
                const uint8_t *p = of + (size_t)y * ostride + 3 * (size_t)x;
                rgb_equal &= p[0] == clamp255(yy + shr16(91881 * cr + 32768));
                rgb_equal &= p[1] == clamp255(yy + shr16(-22554 * cb - 46802 * cr + 32768));
                rgb_equal &= p[2] == clamp255(yy + shr16(116130 * cb + 32768));
            }
            for (size_t x = 3 * (size_t)w; x < ostride; ++x) intact &= of[(size_t)y * ostride + x] == SENTINEL;
        }
        for (size_t i = ostride * h; i < oframe; ++i) intact &= of[i] == SENTINEL;
    }
    printf("abi_version:%d\n", dctq_abi_version());
    printf("ycc_equal:%d\n", ycc_equal);
    printf("rgb_equal:%d\n", rgb_equal);
    printf("padding_intact:%d\n", intact);
    printf("bytes_total:%u\n", (unsigned)bytes_total);
    printf("bytes_per_pixel:%.4f\n", (double)bytes_total / (double)npix);

    dctq_plan_destroy(plan);
    for (int k = 0; k < 3; ++k) {
        dctq_free(pl[k]);
        dctq_free(dec[k]);
        free(hpl[k]);
        free(hdec[k]);
    }
    free(hchan);
    free(hrgb);
    free(hout);
    dctq_free(chan);
    dctq_free(rgb_in);
    dctq_free(rgb_out);
    dctq_free(coef);
    dctq_free(var);
    dctq_free(off);
    dctq_free(boff);
    dctq_free(sym);
    dctq_free(ws);
    dctq_free(bws);
    dctq_free(bytes);
    return ycc_equal && rgb_equal && intact ? 0 : 1;
}
