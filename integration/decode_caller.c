/* decode_caller.c — a plain C caller of the device decoder (include/m2v_mi355x.h + hipMalloc for its own buffers):
 *     decode_caller in.m2v out.yuv layout mode        layout: 0 = I420, 1 = YV12, 2 = NV12, 3 = NV21; mode: 0 = ISO, 1 = module
 * The stream goes to device memory, a probe (d_dst == NULL) says how many pictures of which size it holds, the decode writes them,
 * and the frames are copied back and written out.  Exit status 0: decoded; 1: something failed; 3: the decoder refused the stream
 * (the record's status and err_offset are printed). */
#include <stdio.h>
#include <stdlib.h>

#include <hip/hip_runtime_api.h>

#include "m2v_mi355x.h"

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s in.m2v out.yuv layout mode\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *es = (unsigned char *)malloc(n > 0 ? (size_t)n : 1);
    if (!es || fread(es, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    fclose(f);
    const int layout = atoi(argv[3]), mode = atoi(argv[4]);

    int err = 0, rc = 1;
    m2v_enc *e = m2v_create(6, 6, 3, 2, 0, &err);          /* the decoder takes no part in XL / YL */
    if (!e) { fprintf(stderr, "m2v_create: %s\n", m2v_last_error(NULL)); return 1; }
    void *d_es = NULL, *d_out = NULL;
    unsigned char *frames = NULL;
    m2v_decode_stat r;
    if (hipMalloc(&d_es, (size_t)n + 1) != hipSuccess || hipMemcpy(d_es, es, (size_t)n, hipMemcpyHostToDevice) != hipSuccess) goto done;
    /* the probe: pictures, size, frame_bytes */
    if (m2v_decode_device(e, d_es, (size_t)n, NULL, 0, layout, mode, NULL) != M2V_OK || m2v_decode_report(e, &r) != M2V_OK) {
        fprintf(stderr, "m2v_decode_device: %s\n", m2v_last_error(e));
        goto done;
    }
    if (r.status == M2V_DEC_OK) {
        const size_t cap = (size_t)r.pictures * (size_t)r.frame_bytes;
        if (hipMalloc(&d_out, cap + 1) != hipSuccess) goto done;
        if (m2v_decode_device(e, d_es, (size_t)n, d_out, cap, layout, mode, NULL) != M2V_OK || m2v_decode_report(e, &r) != M2V_OK) {
            fprintf(stderr, "m2v_decode_device: %s\n", m2v_last_error(e));
            goto done;
        }
    }
    if (r.status != M2V_DEC_OK) {
        printf("refused: status %d err_offset %llu\n", (int)r.status, (unsigned long long)r.err_offset);
        rc = 3;
        goto done;
    }
    frames = (unsigned char *)malloc((size_t)r.out_bytes ? (size_t)r.out_bytes : 1);
    if (!frames || hipMemcpy(frames, d_out, (size_t)r.out_bytes, hipMemcpyDeviceToHost) != hipSuccess) goto done;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(frames, 1, (size_t)r.out_bytes, f) != (size_t)r.out_bytes) { fprintf(stderr, "cannot write %s\n", argv[2]); goto done; }
    fclose(f);
    printf("decoded: %u pictures %u x %u, %u GOPs, %llu bytes\n", r.pictures, r.width, r.height, r.gops, (unsigned long long)r.out_bytes);
    rc = 0;
done:
    if (d_es) (void)hipFree(d_es);
    if (d_out) (void)hipFree(d_out);
    free(frames);
    free(es);
    m2v_destroy(e);
    return rc;
}
