/*
 * batch_caller.c - several clips through ONE resident call from plain C (m2v_set_sequences): a file of planar 4:4:4 frames is cut into
 * clips of the given lengths, uploaded once, encoded by one m2v_encode_resident, and every clip's stream is written to a file of its own:
 *
 *     m2v_set_sequences(e, lengths, n) -> m2v_encode_resident(e, ..., d_frames, nframes, d_out, cap, &bytes, NULL)
 *     m2v_sequence_report(e, recs, n)  -> for every clip: out_%03d.m2v = d_out[recs[b].offset, + recs[b].bytes)
 *
 * Each file is, byte for byte, what m2v_encode_resident writes for that clip alone.  "batch_frames" is raised to the call's frames so
 * that one chunk holds the batch (the default, 96, is sized for 1920 x 1152 frames).
 *
 *     cc -std=c99 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include integration/batch_caller.c -Lfpga-mpeg2-encoder_amd -lm2v_mi355x \
 *        -L/opt/rocm/lib -lamdhip64 -o batch_caller
 *     batch_caller in.yuv WIDTH HEIGHT OUT_DIR PFRAMES LEN [LEN ...]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "m2v_mi355x.h"

int main(int argc, char **argv)
{
    if (argc < 7) {
        fprintf(stderr, "usage: %s in.yuv W H out_dir pframes len [len ...]\n", argv[0]);
        return 2;
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]);
    const unsigned pframes = (unsigned)atoi(argv[5]);
    const size_t n = (size_t)(argc - 6);
    if (W % 16 || H % 16 || W < 64 || H < 64) { fprintf(stderr, "batch_caller: sizes must be multiples of 16, >= 64\n"); return 2; }
    uint32_t *lengths = (uint32_t *)malloc(n * sizeof *lengths);
    m2v_sequence_stat *recs = (m2v_sequence_stat *)malloc(n * sizeof *recs);
    if (!lengths || !recs) { fprintf(stderr, "batch_caller: no memory\n"); return 2; }
    size_t nframes = 0;
    for (size_t b = 0; b < n; ++b) { lengths[b] = (uint32_t)atoi(argv[6 + b]); nframes += lengths[b]; }

    const size_t frame_bytes = (size_t)3 * W * H, in_bytes = nframes * frame_bytes;
    const size_t cap = in_bytes + 64 * n + 4096;                  /* no stream is longer than its frames; a tail per clip */
    unsigned char *h_in = (unsigned char *)malloc(in_bytes), *h_out = (unsigned char *)malloc(cap);
    FILE *fin = fopen(argv[1], "rb");
    if (!h_in || !h_out || !fin) { perror("batch_caller"); return 2; }
    if (fread(h_in, frame_bytes, nframes, fin) != nframes) { fprintf(stderr, "batch_caller: %s holds fewer than %zu frames\n", argv[1], nframes); return 2; }
    fclose(fin);

    void *d_in = NULL, *d_out = NULL;
    if (hipMalloc(&d_in, in_bytes) != hipSuccess || hipMalloc(&d_out, cap) != hipSuccess ||
        hipMemcpy(d_in, h_in, in_bytes, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "batch_caller: no device memory\n"); return 1; }

    int err = 0;
    m2v_enc *e = m2v_create(7, 7, 3, 2, 0, &err);
    if (!e) { fprintf(stderr, "batch_caller: m2v_create failed (%d): %s\n", err, m2v_last_error(NULL)); return 1; }
    if (m2v_set_option(e, "batch_frames", (long long)nframes) < 0 || m2v_set_sequences(e, lengths, n) < 0) {
        fprintf(stderr, "batch_caller: %s\n", m2v_last_error(e));
        return 1;
    }
    size_t bytes = 0;
    if (m2v_encode_resident(e, (unsigned)(W / 16), (unsigned)(H / 16), pframes, d_in, nframes, d_out, cap, &bytes, NULL) < 0) {
        fprintf(stderr, "batch_caller: m2v_encode_resident: %s\n", m2v_last_error(e));
        return 1;
    }
    /* (a list of one entry is no batch: one stream, no records) */
    int got = m2v_sequence_report(e, recs, n);
    if (n == 1 && got == 0) { recs[0].offset = 0; recs[0].bytes = bytes; got = 1; }
    if (got != (int)n || hipMemcpy(h_out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "batch_caller: %d records for %zu clips\n", got, n);
        return 1;
    }
    for (size_t b = 0; b < n; ++b) {
        char path[4096];
        snprintf(path, sizeof path, "%s/out_%03zu.m2v", argv[4], b);
        FILE *fout = fopen(path, "wb");
        if (!fout || recs[b].offset + recs[b].bytes > bytes || fwrite(h_out + recs[b].offset, 1, (size_t)recs[b].bytes, fout) != recs[b].bytes) {
            fprintf(stderr, "batch_caller: cannot write %s\n", path);
            return 1;
        }
        fclose(fout);
    }
    printf("batch_caller: %zu clips, %zu frames, %zu bytes\n", n, nframes, bytes);
    m2v_destroy(e);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    free(h_in); free(h_out); free(lengths); free(recs);
    return 0;
}
