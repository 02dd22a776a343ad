// dec_f_host_check.cpp — every stream of a file through the host build of the device decoder's field-picture path
// (tools/dec_f_host.hpp over the fp_ functions of csrc/m2v_decode_kernels.hpp), each in a heap allocation of exactly its size, as
// tools/dec_t_host_check.cpp does for the macroblock tools: built with -fsanitize=address,undefined it shows that the pairing, the
// walk back to a slice's coding extension, the 16 x 8 and dual-prime vectors and the reads they cause stay inside the stream, inside
// the tables, inside the records and inside the reference's fields.  Every stream is planned twice: in 256 ranges of events, as the
// device does, and in 5 - the two must agree.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I fpga-mpeg2-encoder_amd/csrc -I tools tools/dec_f_host_check.cpp
//   dec_f_host_check FILE      FILE: uint32 count, then per stream uint32 (bit 0: "decode_b_pictures"), uint64 length, the bytes
// Prints one line per stream - status, err_offset, pictures, a checksum of the frames - and answers 0; 1 where the two plans differ.
#include <stdio.h>
#include <stdlib.h>

#include "dec_f_host.hpp"

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
        std::vector<uint8_t> frames, again;
        const dec_host::Record r = dec_f_host::decode(n ? es : nullptr, n, (int)(k & 3u), ~0ull, (flags & 1u) != 0, frames);
        const dec_host::Record q = dec_f_host::decode(n ? es : nullptr, n, (int)(k & 3u), ~0ull, (flags & 1u) != 0, again, 5);
        if (r.status != q.status || r.err_offset != q.err_offset || r.pictures != q.pictures || frames != again) {
            fprintf(stderr, "stream %u: planned in 5 ranges it is another stream\n", k);
            return 1;
        }
        uint32_t sum = 0;
        for (uint8_t v : frames) sum = sum * 31u + v;
        printf("%u %d %llu %u %08x\n", k, r.status, (unsigned long long)r.err_offset, r.pictures, sum);
        free(es);
    }
    fclose(f);
    return 0;
}
