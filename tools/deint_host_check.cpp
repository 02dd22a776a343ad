// deint_host_check.cpp — the deinterlacer's arithmetic (csrc/m2v_deint_kernels.hpp, walked as k_deint walks it: tools/deint_host.hpp) as a
// program of its own, for a build with -fsanitize=address,undefined: every source and every output lies in a heap block of exactly its
// size, so a lane that reads or writes one byte beyond a row's end, a plane's last row or the call's last frame is reported.
//   deint_host_check cases.bin out.bin
// cases.bin: for every case eight int32 (width, height, frames, layout, mode, rate, order, blocks at most; 0: the kernel's cap) and the
// frames; out.bin receives the outputs one behind the other (tests/test_deint_cases.py holds them against deinterlace_frames).  One line
// per case: the answer and the bytes written.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "deint_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t hd[8];
    while (fread(hd, sizeof hd, 1, in) == 1) {
        const int w = hd[0], h = hd[1], layout = hd[3], mode = hd[4], rate = hd[5], order = hd[6];
        const uint64_t n = (uint64_t)hd[2];
        const uint64_t fb = m2v::deint::make_frame(layout, (uint32_t)w, (uint32_t)h).bytes, need = m2v::deint::bound(w, h, n, rate);
        const uint64_t in_bytes = n * fb;
        uint8_t *src = (uint8_t *)malloc(in_bytes ? in_bytes : 1), *dst = (uint8_t *)malloc(need ? need : 1);
        if (!src || !dst) return 3;
        if (n && fread(src, fb, n, in) != n) { fprintf(stderr, "cases.bin ends inside a case\n"); return 2; }
        const int r = deint_host::run(src, n, w, h, layout, mode, rate, order, dst, need, (uint32_t)hd[7]);
        if (r == m2v::deint::kOk && need && fwrite(dst, need, 1, out) != 1) return 3;
        printf("%d %llu\n", r, r == m2v::deint::kOk ? (unsigned long long)need : 0ull);
        free(src);
        free(dst);
    }
    fclose(in);
    return fclose(out) ? 3 : 0;
}
