// dec_c_host_check.cpp — every stream of a file through the host build of the device decoder with damaged slices concealed
// (tools/dec_c_host.hpp over the c_ functions of csrc/m2v_decode_kernels.hpp), each in a heap allocation of exactly its size, as
// tools/dec_j_host_check.cpp does for the join: built with -fsanitize=address,undefined it shows that the walk of a damaged slice stays
// inside the stream and inside the records, DC values and levels of the macroblock row its code names - every walk gets a heap block of
// exactly that row -, and that the verdict per row and the search for a slice's picture stay inside the spans and the tables, with
// pictures that have no slice.  Every stream is planned in 256 ranges of events, as the device does, in one, and in 2, 5 and 37 - all
// must agree.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I fpga-mpeg2-encoder_amd/csrc -I tools tools/dec_c_host_check.cpp
//   dec_c_host_check FILE      FILE: uint32 count, then per stream uint32 (bit 0: "decode_b_pictures", bits 1 .. 2: "decode_join"),
//                              uint64 length, the bytes
// Prints one line per stream - status, err_offset, pictures, the report, a checksum of the frames - and answers 0; 1 where two plans
// differ.
#include <stdio.h>
#include <stdlib.h>

#include "dec_c_host.hpp"

static bool read_exact(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (!read_exact(f, &count, 4)) { fprintf(stderr, "short file\n"); return 2; }
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t flags = 0;
        uint64_t n = 0;
        if (!read_exact(f, &flags, 4) || !read_exact(f, &n, 8)) { fprintf(stderr, "short file\n"); return 2; }
        uint8_t *es = (uint8_t *)malloc(n ? n : 1);              // exactly the stream: a read past it is the sanitizer's to find
        if (n && !read_exact(f, es, n)) { fprintf(stderr, "short file\n"); return 2; }
        const bool b = (flags & 1u) != 0;
        const int join = (int)((flags >> 1) & 3u);
        std::vector<uint8_t> frames, again;
        dec_c_host::Join jr, jq;
        dec_c_host::Conceal cr, cq;
        const dec_host::Record r = dec_c_host::decode(n ? es : nullptr, n, (int)(k & 3u), ~0ull, b, join, frames, jr, cr);
        static const uint32_t kLanes[] = {1, 2, 5, 37};
        for (uint32_t lanes : kLanes) {
            const dec_host::Record q = dec_c_host::decode(n ? es : nullptr, n, (int)(k & 3u), ~0ull, b, join, again, jq, cq, lanes);
            if (r.status != q.status || r.err_offset != q.err_offset || r.pictures != q.pictures || frames != again || jr.join_offset != jq.join_offset ||
                jr.tail_offset != jq.tail_offset || cr.first_offset != cq.first_offset || cr.bad_slices != cq.bad_slices || cr.concealed_rows != cq.concealed_rows ||
                cr.grey_rows != cq.grey_rows || cr.damaged_pictures != cq.damaged_pictures) {
                fprintf(stderr, "stream %u: planned in %u ranges it is another stream\n", k, lanes);
                return 1;
            }
        }
        uint32_t sum = 0;
        for (uint8_t v : frames) sum = sum * 31u + v;
        printf("%u %d %llu %u %llu %u %u %u %u %08x\n", k, r.status, (unsigned long long)r.err_offset, r.pictures, (unsigned long long)cr.first_offset, cr.bad_slices,
               cr.concealed_rows, cr.grey_rows, cr.damaged_pictures, sum);
        free(es);
    }
    fclose(f);
    return 0;
}
