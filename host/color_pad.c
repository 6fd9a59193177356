/*
 * host/color_pad.c -- a plain C99 host of the colour entry points for pictures of any size
 * (include/dct_amd.h): a 17 x 9 x 2 interleaved RGB stack that sits at an odd address inside a
 * sentinel-filled buffer, with padded rows and a gap between frames, goes through
 *   1. dctq_rgb_to_ycbcr_pad_planes into the Y, Cb, Cr planes of the picture extended to
 *      32 x 16 (4:2:0), and
 *   2. dctq_ycbcr_to_rgb_crop_planes from those planes into a second such buffer,
 * and prints key=value lines:
 *   abi_version      dctq_abi_version()
 *   ycc_equal        1 if the planes equal the formulas of include/dct_amd.h, restated below,
 *                    applied on the host to pixel(min(x, W - 1), min(y, H - 1))
 *   rgb_equal        1 if the picture of step 2 equals the inverse formulas applied to the planes
 *   padding_intact   1 if step 2 wrote no byte but those of the W x H pixels
 * It exits non-zero if any of the three flags is 0.
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

#define W 17
#define H 9
#define NF 2
#define EW 32 /* W and H rounded up to multiples of 16 */
#define EH 16
#define SENTINEL 0xA5
#define LEAD 13                    /* bytes in front of pixel (0,0): an odd address */
#define STRIDE (3 * W + 6)         /* 57: rows rotate through all four misalignments */
#define FRAME (STRIDE * H + 11)
#define SIZE (LEAD + FRAME * NF + 32)

static int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

/* floor(v / 2^16) for any int: >> of a negative int is implementation-defined in C99 */
static int shr16(int v) { return v >= 0 ? v >> 16 : -((-v + 65535) >> 16); }

static void ycc_of(const uint8_t *p, int *y, int *cb, int *cr) {
    const int r = p[0], g = p[1], b = p[2];
    *y = shr16(19595 * r + 38470 * g + 7471 * b + 32768);
    *cb = shr16(-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767);
    *cr = shr16(32768 * r - 27439 * g - 5329 * b + 8388608 + 32767);
}

/* pixel (x, y) of frame f of the extended picture */
static const uint8_t *pixel(const uint8_t *buf, int f, int x, int y) {
    if (x > W - 1) x = W - 1;
    if (y > H - 1) y = H - 1;
    return buf + LEAD + (size_t)f * FRAME + (size_t)y * STRIDE + 3 * (size_t)x;
}

int main(void) {
    static uint8_t hin[SIZE], hout[SIZE], hy[NF * EH * EW], hcb[NF * EH * EW / 4], hcr[NF * EH * EW / 4];
    uint32_t s = 12345u;
    for (size_t i = 0; i < SIZE; ++i) {
        s = s * 1664525u + 1013904223u;
        hin[i] = (uint8_t)(s >> 24);
    }
    memset(hout, SENTINEL, SIZE);

    void *din, *dout, *dpl[3];
    const size_t psize[3] = {sizeof hy, sizeof hcb, sizeof hcr};
    CHK(dctq_malloc(&din, SIZE));
    CHK(dctq_malloc(&dout, SIZE));
    CHK(dctq_memcpy_htod(din, hin, SIZE));
    CHK(dctq_memcpy_htod(dout, hout, SIZE));
    dctq_plane pl[3];
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_malloc(&dpl[k], psize[k]));
        pl[k].pixels = (const uint8_t *)dpl[k];
        pl[k].width = k ? EW / 2 : EW;
        pl[k].height = k ? EH / 2 : EH;
        pl[k].stride = pl[k].width;
        pl[k].frame_stride = (long long)pl[k].width * pl[k].height;
        pl[k].nframes = NF;
    }
    dctq_rgb rgb;
    rgb.pixels = (uint8_t *)din + LEAD;
    rgb.stride = STRIDE;
    rgb.frame_stride = FRAME;
    rgb.channel_stride = 1;
    rgb.pixel_step = 3;
    rgb.width = W;
    rgb.height = H;
    rgb.nframes = NF;

    CHK(dctq_rgb_to_ycbcr_pad_planes(&rgb, &pl[0], &pl[1], &pl[2], NULL));
    rgb.pixels = (uint8_t *)dout + LEAD;
    CHK(dctq_ycbcr_to_rgb_crop_planes(&pl[0], &pl[1], &pl[2], &rgb, NULL));
    CHK(dctq_synchronize(NULL));
    CHK(dctq_memcpy_dtoh(hy, dpl[0], sizeof hy));
    CHK(dctq_memcpy_dtoh(hcb, dpl[1], sizeof hcb));
    CHK(dctq_memcpy_dtoh(hcr, dpl[2], sizeof hcr));
    CHK(dctq_memcpy_dtoh(hout, dout, SIZE));

    int ycc_equal = 1, rgb_equal = 1, intact = 1;
    static uint8_t own[SIZE]; /* 1: a byte of one of the W x H pixels */
    for (int f = 0; f < NF; ++f) {
        for (int y = 0; y < EH; ++y)
            for (int x = 0; x < EW; ++x) {
                int yy, cb, cr;
                ycc_of(pixel(hin, f, x, y), &yy, &cb, &cr);
                ycc_equal &= hy[((size_t)f * EH + y) * EW + x] == yy;
            }
        for (int y = 0; y < EH / 2; ++y)
            for (int x = 0; x < EW / 2; ++x) {
                int sb = 2, sr = 2;
                for (int j = 0; j < 4; ++j) {
                    int yy, cb, cr;
                    ycc_of(pixel(hin, f, 2 * x + j % 2, 2 * y + j / 2), &yy, &cb, &cr);
                    sb += cb;
                    sr += cr;
                }
                const size_t at = ((size_t)f * (EH / 2) + y) * (EW / 2) + x;
                ycc_equal &= hcb[at] == sb >> 2 && hcr[at] == sr >> 2;
            }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t at = ((size_t)f * (EH / 2) + y / 2) * (EW / 2) + x / 2;
                const int yy = hy[((size_t)f * EH + y) * EW + x], cb = hcb[at] - 128, cr = hcr[at] - 128;
                const size_t o = (size_t)(pixel(hout, f, x, y) - hout);
                rgb_equal &= hout[o] == clamp255(yy + shr16(91881 * cr + 32768));
                rgb_equal &= hout[o + 1] == clamp255(yy + shr16(-22554 * cb - 46802 * cr + 32768));
                rgb_equal &= hout[o + 2] == clamp255(yy + shr16(116130 * cb + 32768));
                own[o] = own[o + 1] = own[o + 2] = 1;
            }
    }
    for (size_t i = 0; i < SIZE; ++i)
        if (!own[i]) intact &= hout[i] == SENTINEL;
    printf("abi_version=%d\n", dctq_abi_version());
    printf("ycc_equal=%d\n", ycc_equal);
    printf("rgb_equal=%d\n", rgb_equal);
    printf("padding_intact=%d\n", intact);

    for (int k = 0; k < 3; ++k) dctq_free(dpl[k]);
    dctq_free(din);
    dctq_free(dout);
    return ycc_equal && rgb_equal && intact ? 0 : 1;
}
