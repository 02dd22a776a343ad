// dec_streams_ex_host_check.cpp — batches of main-syntax streams through the host build of m2v_decode_streams_main_ex_device
// (tools/dec_streams_ex_host.hpp: decode_streams, over csrc/m2v_decode_kernels.hpp and csrc/m2v_decode_streams_ex.hpp): every segment
// in a heap allocation of exactly its size and the output in one of exactly cap bytes.  Built with -fsanitize=address,undefined it shows
// that the scan clamped to the segment, the chunk tables built from the pictures' slice counts, the spans, the rows the slice codes
// name, the two carried slots, the reference slots and the output stay inside them, for valid, refused and overflowing streams alike.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I fpga-mpeg2-encoder_amd/csrc -I tools tools/dec_streams_ex_host_check.cpp
//   dec_streams_ex_host_check FILE   FILE: uint32 count, then per batch uint32 flags, uint32 layout, uint64 cap (all ones: exactly the
//                                      rooms a probe reports), uint32 decode_batch, uint32 streams, then per stream uint64 length, the
//                                      bytes (tests/decstreams_ex_cases.pack_batches)
// Prints one line per stream - batch, stream, status, err_offset, pictures, out_offset - and one per batch with a checksum of the output,
// and answers 0.
#include <stdio.h>
#include <stdlib.h>

#include "dec_streams_ex_host.hpp"

namespace H = dec_streams_ex_host;

static bool read_exact(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (!read_exact(f, &count, 4)) { fprintf(stderr, "short file\n"); return 2; }
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t flags = 0, layout = 0, decode_batch = 0, n = 0;
        uint64_t cap = 0;
        if (!read_exact(f, &flags, 4) || !read_exact(f, &layout, 4) || !read_exact(f, &cap, 8) || !read_exact(f, &decode_batch, 4) || !read_exact(f, &n, 4)) {
            fprintf(stderr, "short file\n");
            return 2;
        }
        std::vector<H::Segment> seg(n);
        for (uint32_t b = 0; b < n; ++b) {
            uint64_t len = 0;
            if (!read_exact(f, &len, 8)) { fprintf(stderr, "short file\n"); return 2; }
            uint8_t *es = (uint8_t *)malloc(len ? len : 1);          // exactly the segment: a read past it is the sanitizer's to find
            if (len && !read_exact(f, es, len)) { fprintf(stderr, "short file\n"); return 2; }
            seg[b] = H::Segment{es, len};
        }
        if (cap == ~0ull) {
            cap = 0;
            for (const H::StreamRecord &r : H::decode_streams(seg.data(), n, (int)layout, flags, nullptr, 0, decode_batch))
                cap = std::max<uint64_t>(cap, r.out_offset + r.rec.out_bytes);
        }
        uint8_t *out = (uint8_t *)malloc(cap ? cap : 1);             // exactly cap: a write past it, too
        memset(out, 0xA5, cap ? cap : 1);
        const std::vector<H::StreamRecord> recs = H::decode_streams(seg.data(), n, (int)layout, flags, out, cap, decode_batch);
        for (uint32_t b = 0; b < n; ++b)
            printf("%u %u %d %llu %u %llu\n", k, b, recs[b].rec.status, (unsigned long long)recs[b].rec.err_offset, recs[b].rec.pictures,
                   (unsigned long long)recs[b].out_offset);
        uint32_t sum = 0;
        for (uint64_t o = 0; o < cap; ++o) sum = sum * 31u + out[o];
        printf("%u sum %08x\n", k, sum);
        free(out);
        for (uint32_t b = 0; b < n; ++b) free((void *)seg[b].p);
    }
    fclose(f);
    return 0;
}
