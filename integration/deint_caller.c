/* deint_caller.c — the chain decode -> deinterlace -> encode from plain C (include/m2v_mi355x.h + hipMalloc for its own buffers), the
 * frames never leaving device memory:
 *     deint_caller in.m2v out.m2v mode rate order     mode: 0 = line, 1 = adaptive, 2 = blend; rate: 0 = a frame per frame, 1 = a frame
 *                                                     per field; order: 0 = top field first, 1 = bottom field first
 * in.m2v is an interlaced Main-Profile stream (frame pictures with field prediction and field DCT; B pictures too).  It is decoded on the
 * device (m2v_decode_device: a probe for the size, then the decode), the woven frames are deinterlaced where they lie
 * (m2v_deinterlace_device, on the handle's stream, no wait), and the progressive frames go into m2v_encode_resident420 on the same
 * stream with their size set as the source size (m2v_set_source_size): the picture is the frames' size rounded up to whole macroblocks,
 * 64 x 64 at least, and the resampler, which filters across neighbouring lines, now sees lines of one instant only.
 * Exit status 0: out.m2v written; 1: something failed; 3: the decoder refused the stream. */
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "m2v_mi355x.h"

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s in.m2v out.m2v mode rate order\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *es = (unsigned char *)malloc(n > 0 ? (size_t)n : 1);
    if (!es || fread(es, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    fclose(f);
    const int mode = atoi(argv[3]), rate = atoi(argv[4]), order = atoi(argv[5]);

    int err = 0, rc = 1;
    m2v_enc *e = m2v_create(7, 7, 3, 2, 0, &err);
    if (!e) { fprintf(stderr, "m2v_create: %s\n", m2v_last_error(NULL)); return 1; }
    void *d_es = NULL, *d_woven = NULL, *d_prog = NULL, *d_stream = NULL;
    unsigned char *stream = NULL;
    m2v_decode_stat r;
    if (hipMalloc(&d_es, (size_t)n + 1) != hipSuccess || hipMemcpy(d_es, es, (size_t)n, hipMemcpyHostToDevice) != hipSuccess) goto done;
    if (m2v_set_option(e, "decode_syntax", M2V_SYNTAX_MAIN) != M2V_OK || m2v_set_option(e, "decode_b_pictures", 1) != M2V_OK ||
        m2v_set_option(e, "decode_interlaced", 1) != M2V_OK) {
        fprintf(stderr, "m2v_set_option: %s\n", m2v_last_error(e));
        goto done;
    }
    /* 1. decode: the probe says how many frames of which size */
    if (m2v_decode_device(e, d_es, (size_t)n, NULL, 0, M2V_420_I420, M2V_DEC_ISO, NULL) != M2V_OK || m2v_decode_report(e, &r) != M2V_OK) {
        fprintf(stderr, "m2v_decode_device: %s\n", m2v_last_error(e));
        goto done;
    }
    if (r.status == M2V_DEC_OK) {
        if (hipMalloc(&d_woven, (size_t)r.out_bytes + 1) != hipSuccess) goto done;
        if (m2v_decode_device(e, d_es, (size_t)n, d_woven, (size_t)r.out_bytes, M2V_420_I420, M2V_DEC_ISO, NULL) != M2V_OK || m2v_decode_report(e, &r) != M2V_OK) {
            fprintf(stderr, "m2v_decode_device: %s\n", m2v_last_error(e));
            goto done;
        }
    }
    if (r.status != M2V_DEC_OK) {
        printf("refused: status %d err_offset %llu\n", (int)r.status, (unsigned long long)r.err_offset);
        rc = 3;
        goto done;
    }
    {
        /* 2. deinterlace: one launch, no wait */
        const size_t frames = (size_t)r.pictures * (rate == M2V_DEINT_FIELD_RATE ? 2u : 1u);
        const unsigned long long room = m2v_deinterlace_bound((int)r.width, (int)r.height, r.pictures, rate);
        if (!room || hipMalloc(&d_prog, (size_t)room) != hipSuccess) { fprintf(stderr, "no room for %llu bytes of frames\n", room); goto done; }
        if (m2v_deinterlace_device(e, d_woven, r.pictures, (int)r.width, (int)r.height, M2V_420_I420, mode, rate, order, d_prog, (size_t)room, NULL) != M2V_OK) {
            fprintf(stderr, "m2v_deinterlace_device: %s\n", m2v_last_error(e));
            goto done;
        }
        /* 3. encode, behind it on the same stream: the frames' size is the source size, the picture whole macroblocks */
        uint32_t xs = 0, ys = 0;
        if (m2v_fit_size((int)r.width, (int)r.height, &xs, &ys) != M2V_OK) goto done;
        if (xs < 4) xs = 4;
        if (ys < 4) ys = 4;
        const size_t cap = 4096 + frames * xs * ys * 16 * 16 * 3;
        size_t bytes = 0;
        if (hipMalloc(&d_stream, cap) != hipSuccess) goto done;
        if (m2v_set_source_size(e, (int)r.width, (int)r.height, M2V_SCALE_TRIANGLE) != M2V_OK ||
            m2v_encode_resident420(e, xs, ys, 5, d_prog, frames, M2V_420_I420, d_stream, cap, &bytes, NULL) != M2V_OK) {
            fprintf(stderr, "m2v_encode_resident420: %s\n", m2v_last_error(e));
            goto done;
        }
        stream = (unsigned char *)malloc(bytes ? bytes : 1);
        if (!stream || hipMemcpy(stream, d_stream, bytes, hipMemcpyDeviceToHost) != hipSuccess) goto done;
        f = fopen(argv[2], "wb");
        if (!f || fwrite(stream, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", argv[2]); goto done; }
        fclose(f);
        printf("%u woven frames %u x %u -> %zu progressive frames -> %zu bytes at %u x %u\n", r.pictures, r.width, r.height, frames, bytes, 16 * xs, 16 * ys);
        rc = 0;
    }
done:
    if (d_es) (void)hipFree(d_es);
    if (d_woven) (void)hipFree(d_woven);
    if (d_prog) (void)hipFree(d_prog);
    if (d_stream) (void)hipFree(d_stream);
    free(stream);
    free(es);
    m2v_destroy(e);
    return rc;
}
