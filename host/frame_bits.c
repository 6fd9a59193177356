/*
 * host/frame_bits.c -- a plain C99 host of the bit-packed coefficient stream of the
 * batched C-ABI (include/dct_amd.h, format "bits v1"): generates a synthetic Y/Cb/Cr
 * 4:2:0 frame on the device, encodes the three planes in one call into the plan's most
 * compact symbols (dctq_encode_planes16, or dctq_encode_planes where the plan needs 4-byte
 * symbols), packs them (dctq_bits_pack: offsets first, then the bytes into a buffer of
 * exactly that size followed by guard bytes), and decodes twice into planes with padded
 * rows that were filled with a sentinel --
 *   A: dctq_decode_symbols_planes on the symbols;
 *   B: dctq_decode_bits_planes on the packed bytes
 * -- and prints key=value lines:
 *   abi_version     dctq_abi_version()
 *   symbol_bytes    the symbol format that was packed
 *   blocks          blocks of the three planes
 *   symbols_total   symbols of the stream
 *   bytes_total     bytes of the packed stream (offsets[blocks])
 *   fused_equal     1 if B's buffers equal A's byte for byte
 *   padding_intact  1 if B wrote no byte of the row padding
 *   guard_intact    1 if the packer wrote no byte past bytes_total
 *
 *   frame_bits WIDTH HEIGHT QUALITY ADAPTIVE SEED [KIND]
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
#define PAD 64   /* bytes of padding after every row */
#define GUARD 64 /* bytes after the packed stream */

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s W H QUALITY ADAPTIVE SEED [KIND]\n", argv[0]);
        return 2;
    }
    int w = atoi(argv[1]), h = atoi(argv[2]), q = atoi(argv[3]), ad = atoi(argv[4]);
    uint64_t seed = strtoull(argv[5], NULL, 10);
    int kind = argc > 6 ? atoi(argv[6]) : 0;
    if (w < 16 || h < 16 || w % 16 || h % 16) {
        fprintf(stderr, "W and H must be positive multiples of 16 (4:2:0 chroma in 8x8 blocks)\n");
        return 2;
    }
    const int pw[3] = {w, w / 2, w / 2}, ph[3] = {h, h / 2, h / 2};
    long long nb[3], first[4] = {0, 0, 0, 0};
    size_t padded[3];
    for (int k = 0; k < 3; ++k) {
        nb[k] = (long long)(pw[k] / 8) * (ph[k] / 8);
        first[k + 1] = first[k] + nb[k];
        padded[k] = (size_t)(pw[k] + PAD) * ph[k];
    }
    const long long nblk = first[3], cap = 64 * nblk;

    void *px[3], *outa[3], *outb[3], *coef, *var, *off, *sym, *ws, *boff, *bws, *bytes;
    dctq_plane src[3], da[3], db[3];
    uint8_t *ha[3], *hb[3];
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_malloc(&px[k], (size_t)pw[k] * ph[k]));
        CHK(dctq_malloc(&outa[k], padded[k]));
        CHK(dctq_malloc(&outb[k], padded[k]));
        ha[k] = malloc(padded[k]);
        hb[k] = malloc(padded[k]);
        if (!ha[k] || !hb[k]) return 1;
        src[k].pixels = (const uint8_t *)px[k];
        src[k].stride = pw[k];
        src[k].frame_stride = (long long)pw[k] * ph[k];
        src[k].width = pw[k];
        src[k].height = ph[k];
        src[k].nframes = 1;
        da[k] = src[k];
        da[k].pixels = (const uint8_t *)outa[k];
        da[k].stride = pw[k] + PAD;
        da[k].frame_stride = (long long)padded[k];
        db[k] = da[k];
        db[k].pixels = (const uint8_t *)outb[k];
        CHK(dctq_synth(seed + (uint64_t)k, kind, &src[k], NULL));
        memset(ha[k], SENTINEL, padded[k]);
        CHK(dctq_memcpy_htod(outa[k], ha[k], padded[k]));
        CHK(dctq_memcpy_htod(outb[k], ha[k], padded[k]));
    }
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
    if (ad) CHK(dctq_forward_quant_planes(plan, src, 3, cp, vw, NULL));

    const int symbytes = dctq_plan_symbol_bytes(plan);
    if (symbytes == 2)
        CHK(dctq_encode_planes16(plan, src, 3, cp, (uint32_t *)off, (uint16_t *)sym, cap, ws, NULL));
    else
        CHK(dctq_encode_planes(plan, src, 3, cp, (uint32_t *)off, (uint32_t *)sym, cap, ws, NULL));
    /* the offsets first: they size the byte buffer */
    uint32_t symbols_total = 0, bytes_total = 0;
    CHK(dctq_bits_pack(sym, symbytes, (const uint32_t *)off, nblk, (uint32_t *)boff, NULL, 0, bws, NULL));
    CHK(dctq_synchronize(NULL));
    CHK(dctq_memcpy_dtoh(&symbols_total, (const uint32_t *)off + nblk, 4));
    CHK(dctq_memcpy_dtoh(&bytes_total, (const uint32_t *)boff + nblk, 4));
    const size_t room = ((size_t)bytes_total + 3) / 4 * 4 + GUARD;
    uint8_t *hbytes = malloc(room);
    if (!hbytes) return 1;
    memset(hbytes, SENTINEL, room);
    CHK(dctq_malloc(&bytes, room));
    CHK(dctq_memcpy_htod(bytes, hbytes, room));
    CHK(dctq_bits_pack(sym, symbytes, (const uint32_t *)off, nblk, (uint32_t *)boff, (uint8_t *)bytes,
                       (long long)bytes_total, bws, NULL));

    /* A: symbols -> pixels; B: packed bytes -> pixels */
    CHK(dctq_decode_symbols_planes(plan, sym, symbytes, (const uint32_t *)off, ad ? vn : NULL, da, 3, NULL));
    CHK(dctq_decode_bits_planes(plan, (const uint8_t *)bytes, (const uint32_t *)boff, ad ? vn : NULL, db, 3, NULL));
    CHK(dctq_synchronize(NULL));
    int equal = 1, intact = 1, guard = 1;
    for (int k = 0; k < 3; ++k) {
        CHK(dctq_memcpy_dtoh(ha[k], outa[k], padded[k]));
        CHK(dctq_memcpy_dtoh(hb[k], outb[k], padded[k]));
        equal &= memcmp(ha[k], hb[k], padded[k]) == 0;
        for (int y = 0; y < ph[k]; ++y)
            for (int x = pw[k]; x < pw[k] + PAD; ++x) intact &= hb[k][(size_t)y * (size_t)(pw[k] + PAD) + x] == SENTINEL;
    }
    CHK(dctq_memcpy_dtoh(hbytes, bytes, room));
    for (size_t i = bytes_total; i < room; ++i) guard &= hbytes[i] == SENTINEL;
    printf("abi_version=%d\n", dctq_abi_version());
    printf("symbol_bytes=%d\n", symbytes);
    printf("blocks=%lld\n", nblk);
    printf("symbols_total=%u\n", (unsigned)symbols_total);
    printf("bytes_total=%u\n", (unsigned)bytes_total);
    printf("fused_equal=%d\n", equal);
    printf("padding_intact=%d\n", intact);
    printf("guard_intact=%d\n", guard);

    dctq_plan_destroy(plan);
    for (int k = 0; k < 3; ++k) {
        dctq_free(px[k]);
        dctq_free(outa[k]);
        dctq_free(outb[k]);
        free(ha[k]);
        free(hb[k]);
    }
    free(hbytes);
    dctq_free(coef);
    dctq_free(var);
    dctq_free(off);
    dctq_free(boff);
    dctq_free(sym);
    dctq_free(ws);
    dctq_free(bws);
    dctq_free(bytes);
    return 0;
}
