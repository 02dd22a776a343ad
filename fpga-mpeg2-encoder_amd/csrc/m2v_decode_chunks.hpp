// m2v_decode_chunks.hpp — the chunk schedule of a main-syntax stream with B pictures, on the host behind the plan's wait: which pictures
// of a chunk are reconstructed in which launch, and what the chunk leaves in the two carried slots for the next.  dec_b_chunks,
// dec_i_chunks and dec_x_chunks run it; dec_f_chunks schedules coded pictures inside chunks of whole frames - the second field of a
// frame is a step behind its first - and keeps its own loop over the same two structures.  Plain C++ without HIP types.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace m2v {

struct DecLaunch { size_t off, count; };           // h_list[off, off + count): the coded indices of one launch's pictures
struct DecChunk { std::vector<DecLaunch> steps; DecLaunch b; long c1, carry0, carry1; };      // c1: the last anchor in front of the chunk; carry: the chunk's slot to copy into slot 0 / 1 (-1: nothing)

// pictures [0, np) of the given types (1 I, 2 P, 3 B) in coded order, B to a chunk.  Every chunk's anchors ordered by their step inside
// the chunk - a chain starts at its I picture, or at the chunk's first anchor -, then its B pictures, into h_list (np words: chunk
// [p0, p0 + nb) fills h_list[p0, p0 + nb)); and what the chunk leaves in slots 0 and 1 for the next
inline std::vector<DecChunk> dec_chunk_schedule(const uint8_t *types, size_t np, size_t B, uint32_t *h_list)
{
    std::vector<DecChunk> chunks;
    long a1 = -1, a2 = -1;                                             // the last two anchors in front of the chunk, coded indices
    for (size_t p0 = 0; p0 < np; p0 += B) {
        const size_t nb = std::min(B, np - p0);
        DecChunk C;
        C.c1 = a1;
        std::vector<long> step(nb, -1);
        long deepest = -1, prev = -1;
        for (size_t k = 0; k < nb; ++k) {
            if (types[p0 + k] == 3) continue;
            step[k] = prev >= 0 && types[p0 + k] != 1 ? step[prev] + 1 : 0;
            deepest = std::max(deepest, step[k]);
            prev = (long)k;
        }
        size_t at = p0;
        for (long j = 0; j <= deepest; ++j) {
            const size_t first = at;
            for (size_t k = 0; k < nb; ++k) if (step[k] == j) h_list[at++] = (uint32_t)(p0 + k);
            C.steps.push_back(DecLaunch{first, at - first});
        }
        C.b.off = at;
        for (size_t k = 0; k < nb; ++k) if (types[p0 + k] == 3) h_list[at++] = (uint32_t)(p0 + k);
        C.b.count = at - C.b.off;
        auto slot = [&](long r) { return r >= (long)p0 ? 2 + (r - (long)p0) : r == C.c1 ? 1L : 0L; };
        long n1 = a1, n2 = a2;
        for (size_t k = 0; k < nb; ++k) if (types[p0 + k] != 3) { n2 = n1; n1 = (long)(p0 + k); }
        C.carry0 = n2 >= 0 && slot(n2) != 0 ? slot(n2) : -1;
        C.carry1 = n1 >= 0 && slot(n1) != 1 ? slot(n1) : -1;
        a1 = n1; a2 = n2;
        chunks.push_back(C);
    }
    return chunks;
}

}  // namespace m2v
