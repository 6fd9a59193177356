/*
 * host/frame_rd.c -- a plain C99 host of the rate / distortion pair of the batched
 * C-ABI (include/dct_amd.h): both columns of the reference's per-block report
 * (tests/test_entropy.c:300-393) for a whole 4:2:0 frame stack in two launches, with
 * no coefficient or picture buffer.  Generates a synthetic stack (Y, Cb, Cr) on the
 * device, runs dctq_huffman_bits_planes and dctq_distortion_planes over it, then checks
 * the distortion the long way: dctq_forward_quant_planes + dctq_decode_planes into
 * pictures with padded rows, copied back, every block's squared error recomputed by the
 * host loop.  Prints
 *   blocks            blocks of the three planes (Y first; by frame, block row, column)
 *   bits_total        sum of the per-block Huffman sizes
 *   sse_total         sum of the per-block squared errors
 *   psnr_u8           10 log10(255^2 * 64 * blocks / sse_total) (inf for an exact stack)
 *   distortion_equal  1 only if every block's device value equals the host's
 *   abi_version       dctq_abi_version()
 *
 *   frame_rd WIDTH HEIGHT FRAMES QUALITY ADAPTIVE SEED [KIND]
 * Plane k of the stack is dctq_synth(SEED + 1000 k, KIND).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "dct_amd.h"

#define CHK(x)                                                                  \
    do {                                                                        \
        int rc_ = (x);                                                          \
        if (rc_) {                                                              \
            fprintf(stderr, "%s: %s\n", #x, dctq_error_string(rc_));            \
            return 1;                                                           \
        }                                                                       \
    } while (0)

#define NPLANES 3
#define PAD 64 /* bytes of padding after every decoded row */

int main(int argc, char **argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s W H FRAMES QUALITY ADAPTIVE SEED [KIND]\n", argv[0]);
        return 2;
    }
    int w = atoi(argv[1]), h = atoi(argv[2]), nf = atoi(argv[3]), q = atoi(argv[4]), ad = atoi(argv[5]);
    uint64_t seed = strtoull(argv[6], NULL, 10);
    int kind = argc > 7 ? atoi(argv[7]) : 0;
    if (w < 16 || h < 16 || w % 16 || h % 16 || nf < 1) {
        fprintf(stderr, "W and H must be positive multiples of 16 (4:2:0), FRAMES >= 1\n");
        return 2;
    }

    dctq_plane src[NPLANES], dst[NPLANES];
    void *px[NPLANES], *coef[NPLANES], *var[NPLANES], *pic[NPLANES];
    long long nblk[NPLANES], first[NPLANES + 1];
    first[0] = 0;
    for (int k = 0; k < NPLANES; ++k) {
        const int pw = k ? w / 2 : w, ph = k ? h / 2 : h;
        nblk[k] = (long long)(pw / 8) * (ph / 8) * nf;
        first[k + 1] = first[k] + nblk[k];
        CHK(dctq_malloc(&px[k], (size_t)pw * ph * nf));
        CHK(dctq_malloc(&coef[k], (size_t)nblk[k] * 128));
        CHK(dctq_malloc(&var[k], (size_t)nblk[k] * 4));
        CHK(dctq_malloc(&pic[k], (size_t)(pw + PAD) * ph * nf));
        src[k].pixels = (const uint8_t *)px[k];
        src[k].stride = pw;
        src[k].frame_stride = (long long)pw * ph;
        src[k].width = pw;
        src[k].height = ph;
        src[k].nframes = nf;
        dst[k] = src[k];
        dst[k].pixels = (const uint8_t *)pic[k];
        dst[k].stride = pw + PAD;
        dst[k].frame_stride = (long long)(pw + PAD) * ph;
        CHK(dctq_synth(seed + 1000u * (uint64_t)k, kind, &src[k], NULL));
    }
    const long long total = first[NPLANES];
    void *bits, *sse;
    CHK(dctq_malloc(&bits, (size_t)total * 4));
    CHK(dctq_malloc(&sse, (size_t)total * 4));
    dctq_plan *plan;
    CHK(dctq_plan_create(q, ad, &plan));

    /* the two launches: pixels in, 4 + 4 B per block out */
    CHK(dctq_huffman_bits_planes(plan, src, NPLANES, (uint32_t *)bits, NULL));
    CHK(dctq_distortion_planes(plan, src, NPLANES, (uint32_t *)sse, NULL));

    /* the composition the distortion is defined by, through coefficients and pictures */
    int16_t *cp[NPLANES];
    int32_t *vp[NPLANES];
    const int16_t *ccp[NPLANES];
    const int32_t *cvp[NPLANES];
    for (int k = 0; k < NPLANES; ++k) {
        ccp[k] = cp[k] = (int16_t *)coef[k];
        cvp[k] = vp[k] = (int32_t *)var[k];
    }
    CHK(dctq_forward_quant_planes(plan, src, NPLANES, cp, vp, NULL));
    CHK(dctq_decode_planes(plan, ccp, cvp, dst, NPLANES, NULL));
    CHK(dctq_synchronize(NULL));

    uint32_t *hbits = malloc((size_t)total * 4), *hsse = malloc((size_t)total * 4);
    if (!hbits || !hsse) return 1;
    CHK(dctq_memcpy_dtoh(hbits, bits, (size_t)total * 4));
    CHK(dctq_memcpy_dtoh(hsse, sse, (size_t)total * 4));

    int equal = 1;
    unsigned long long bits_total = 0, sse_total = 0;
    for (int k = 0; k < NPLANES; ++k) {
        const int pw = src[k].width, ph = src[k].height;
        const size_t ps = (size_t)dst[k].stride;
        uint8_t *hpx = malloc((size_t)pw * ph * nf), *hpic = malloc(ps * ph * nf);
        if (!hpx || !hpic) return 1;
        CHK(dctq_memcpy_dtoh(hpx, px[k], (size_t)pw * ph * nf));
        CHK(dctq_memcpy_dtoh(hpic, pic[k], ps * ph * nf));
        long long b = first[k];
        for (int f = 0; f < nf; ++f)
            for (int by = 0; by < ph / 8; ++by)
                for (int bx = 0; bx < pw / 8; ++bx, ++b) {
                    uint32_t se = 0;
                    for (int y = 0; y < 8; ++y)
                        for (int x = 0; x < 8; ++x) {
                            const size_t row = (size_t)f * ph + (size_t)by * 8 + y, col = (size_t)bx * 8 + x;
                            const int e = (int)hpx[row * pw + col] - (int)hpic[row * ps + col];
                            se += (uint32_t)(e * e);
                        }
                    equal &= se == hsse[b];
                    sse_total += hsse[b];
                    bits_total += hbits[b];
                }
        free(hpx);
        free(hpic);
    }

    printf("blocks:%lld\n", total);
    printf("bits_total:%llu\n", bits_total);
    printf("sse_total:%llu\n", sse_total);
    if (sse_total)
        printf("psnr_u8:%.4f\n", 10.0 * log10(255.0 * 255.0 * 64.0 * (double)total / (double)sse_total));
    else
        printf("psnr_u8:inf\n");
    printf("distortion_equal:%d\n", equal);
    printf("abi_version:%d\n", dctq_abi_version());

    dctq_plan_destroy(plan);
    for (int k = 0; k < NPLANES; ++k) {
        dctq_free(px[k]);
        dctq_free(coef[k]);
        dctq_free(var[k]);
        dctq_free(pic[k]);
    }
    dctq_free(bits);
    dctq_free(sse);
    free(hbits);
    free(hsse);
    return 0;
}
