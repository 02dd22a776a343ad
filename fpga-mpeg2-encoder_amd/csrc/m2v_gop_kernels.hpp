// m2v_gop_kernels.hpp — device code of option "gop_bytes_max" (m2v_gop.hip tells the whole story): k_gop_judge, the size of every GOP of
// a chunk against the cap.  Included by m2v_launch.hip behind m2v_kernels.hpp, whose frame_header_bytes and wave_sum it uses (that header
// defines kernels and device globals with external linkage, so one unit only can include it).
#pragma once
#include "../../include/m2v_mi355x.h"
#include "m2v_kernels.hpp"

static_assert(sizeof(m2v_gop_stat) == 32 && offsetof(m2v_gop_stat, bytes) == 16 && offsetof(m2v_gop_stat, over) == 28,
              "k_gop_judge writes the record in place");

namespace m2v {

constexpr int kJudgeThreads = 256;

// One block per GOP of the chunk: GOP sg = frames [sg * gop, min((sg + 1) * gop, nf)) - with the cap on a chunk holds whole GOPs, only
// the sequence's last one may be cut short.  Its size is what k_frame_scan will add up for these frames: their headers
// (frame_header_bytes; the sequence header is not a GOP's, and neither is a copy of it that repeat_headers of m2v_set_stream_desc puts in
// front of the GOP) and the bytes of their slices (k_slice_scan).  A GOP whose record says it is
// settled - it fitted, or it was coded at level 4 - is left alone; the others are measured, and one that is over the cap below level 4
// gets FrameJob::q of its frames raised by one: the host (gop_cap_chunk) reads the record in pinned memory and codes it again.
// Integers only, one block per GOP: the verdict depends on nothing but the GOP's own bytes.
__global__ __launch_bounds__(kJudgeThreads) void k_gop_judge(FrameJob *__restrict__ jobs, Geom g, int nf, int gop,
                                                             const uint32_t *__restrict__ slice_bytes, unsigned long long cap,
                                                             m2v_gop_stat *__restrict__ recs, m2v_gop_stat *__restrict__ h_recs)
{
    __shared__ unsigned long long s_sum;
    const int tid = threadIdx.x, sg = blockIdx.x;
    const int a = sg * gop, b = a + gop < nf ? a + gop : nf;
    if (a >= nf) return;
    const m2v_gop_stat prev = recs[sg];                        // (block-uniform; zeroed in front of the chunk's first try)
    if (prev.tries && (!prev.over || prev.level >= 4u)) return;
    if (tid == 0) s_sum = 0ull;
    const uint32_t level = jobs[a].q;                          // read by everyone before anyone raises it (the barrier below)
    __syncthreads();
    unsigned long long sum = 0;
    const uint32_t items = (uint32_t)(b - a) * (uint32_t)g.mbh;
    const uint32_t *const sb = slice_bytes + (size_t)a * (size_t)g.mbh;
    for (uint32_t i = (uint32_t)tid; i < items; i += kJudgeThreads) sum += sb[i];
    for (int f = a + tid; f < b; f += kJudgeThreads) sum += frame_header_bytes(jobs[f].i_frame);
    // a wavefront's sum by DPP, which moves 32 bits: three parts whose totals cannot wrap (k_frame_scan does the same)
    const unsigned long long w = (unsigned long long)(uint32_t)wave_sum((int)((uint32_t)sum & 0xFFFFu)) +
                                 ((unsigned long long)(uint32_t)wave_sum((int)(((uint32_t)sum >> 16) & 0xFFFFu)) << 16) +
                                 ((unsigned long long)(uint32_t)wave_sum((int)(uint32_t)(sum >> 32)) << 32);
    if ((tid & 63) == 0) atomicAdd(&s_sum, w);
    __syncthreads();
    const unsigned long long size = s_sum;
    const bool over = size > cap;
    if (over && level < 4u)
        for (int f = a + tid; f < b; f += kJudgeThreads) jobs[f].q = level + 1u;
    if (tid == 0) {
        m2v_gop_stat r;
        r.first_frame = jobs[a].n;
        r.gop = r.first_frame / (uint32_t)gop;
        r.frames = (uint32_t)(b - a);
        r.level = level;
        r.bytes = size;
        r.tries = prev.tries + 1u;
        r.over = over ? 1u : 0u;
        recs[sg] = r;
        h_recs[sg] = r;
        __threadfence_system();
    }
}

}  // namespace m2v
