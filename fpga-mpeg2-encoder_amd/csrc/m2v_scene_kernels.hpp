// m2v_scene_kernels.hpp — device code of option "scene_cut" (m2v_scene.hip tells the whole story): k_mbsum, the luma sum of every
// macroblock of a chunk's frames, and k_scene_judge, the frame-to-frame difference of those sums against the threshold.  Included by
// m2v_launch.hip behind m2v_kernels.hpp, whose wave_sum it uses (that header defines kernels and device globals with external
// linkage, so one unit only can include it).
#pragma once
#include "m2v_kernels.hpp"

namespace m2v {

constexpr int kSceneThreads = 256;

// 16 bytes of a picture row at p.  ALIGNED: p is 16-byte aligned, one dwordx4 load.  Otherwise: the five naturally aligned dwords
// that cover them, shifted into place (v_alignbyte) - the first starts at most 3 bytes in front of p and the last ends at most 3
// bytes behind p + 16, both inside the frame: an allocation starts on a dword boundary, and the chroma planes follow the luma plane.
template <bool ALIGNED>
__device__ __forceinline__ uint4 load_row16(const uint8_t *p)
{
    if (ALIGNED) return *(const uint4 *)p;
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t *q = (const uint32_t *)(p - sh);
    const uint32_t a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
    uint4 r;
    r.x = __builtin_amdgcn_alignbyte(b, a, sh);
    r.y = __builtin_amdgcn_alignbyte(c, b, sh);
    r.z = __builtin_amdgcn_alignbyte(d, c, sh);
    r.w = __builtin_amdgcn_alignbyte(e, d, sh);
    return r;
}

// One wavefront per 16 picture rows x 256 columns (16 macroblocks of one macroblock row): lane l reads the 16 bytes of macroblock
// l % 16 in rows 4 i + l / 16, i = 0..3 - four loads of 1 KB per wavefront, 256 contiguous bytes per row, all issued before the first
// use - sums them with v_dot4 and the four row groups meet in two cross-lane steps.  Every luma byte of the chunk is read exactly once
// and every sum has one writer.  unit = blockIdx.x: (frame, macroblock row, 256-column unit), the unit fastest.
// frames: the chunk's planar 4:4:4 frames (3 * ysz bytes each, luma first); sums: [frame][mb].
template <bool ALIGNED>
__global__ __launch_bounds__(64) void k_mbsum(const uint8_t *__restrict__ frames, Geom g, int units_x, uint32_t *__restrict__ sums)
{
    const int lane = threadIdx.x;
    const uint32_t unit = blockIdx.x;
    const int ux = (int)(unit % (uint32_t)units_x);
    const uint32_t fr = unit / (uint32_t)units_x;           // frame * mbh + macroblock row
    const int mby = (int)(fr % (uint32_t)g.mbh);
    const size_t f = fr / (uint32_t)g.mbh;
    const int mbx = ux * 16 + (lane & 15);
    const bool inside = mbx < g.mbw;                         // the tail of a row whose macroblocks are no multiple of 16
    uint32_t acc = 0;
    if (inside) {
        const uint8_t *p = frames + f * (size_t)g.ysz * 3 + (size_t)(mby * 16 + (lane >> 4)) * (size_t)g.W + (size_t)mbx * 16;
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = load_row16<ALIGNED>(p + (size_t)(4 * i) * (size_t)g.W);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc = __builtin_amdgcn_udot4(v[i].x, 0x01010101u, acc, false);
            acc = __builtin_amdgcn_udot4(v[i].y, 0x01010101u, acc, false);
            acc = __builtin_amdgcn_udot4(v[i].z, 0x01010101u, acc, false);
            acc = __builtin_amdgcn_udot4(v[i].w, 0x01010101u, acc, false);
        }
    }
    acc += (uint32_t)__shfl_xor((int)acc, 16, 64);
    acc += (uint32_t)__shfl_xor((int)acc, 32, 64);
    if (lane < 16 && inside) sums[f * (size_t)g.mbs + (size_t)mby * (size_t)g.mbw + (size_t)mbx] = acc;
}

// One block per frame of the chunk: D = the sum over the macroblocks of |S(frame) - S(frame before)|, flagged iff D > T * mbs.  The
// frame in front of the chunk's first one is the previous chunk's last: its sums are in carry_in (null: the sequence starts here, D = 0).
// The block of the chunk's last frame leaves that frame's sums in carry_out - ANOTHER buffer than carry_in, which block 0 may still be
// reading.  The record goes to the device array and, the same bytes, to pinned memory the host reads after its wait.
__global__ __launch_bounds__(kSceneThreads) void k_scene_judge(const uint32_t *__restrict__ sums, int mbs, int nf, unsigned long long limit,
                                                               const uint32_t *__restrict__ carry_in, uint32_t *__restrict__ carry_out,
                                                               SceneRec *__restrict__ recs, SceneRec *__restrict__ h_recs)
{
    __shared__ unsigned long long s_sum;
    const int tid = threadIdx.x, f = blockIdx.x;
    if (f >= nf) return;
    if (tid == 0) s_sum = 0ull;
    __syncthreads();
    const uint32_t *const cur = sums + (size_t)f * (size_t)mbs;
    const uint32_t *const prev = f > 0 ? cur - mbs : carry_in;
    uint32_t d = 0;                                          // at most 64 macroblocks per thread (128 x 128 of them), 65280 each
    if (prev)
        for (int i = tid; i < mbs; i += kSceneThreads) {
            const uint32_t a = cur[i], b = prev[i];
            d += a > b ? a - b : b - a;
        }
    if (f == nf - 1)
        for (int i = tid; i < mbs; i += kSceneThreads) carry_out[i] = cur[i];
    // a wavefront's sum by DPP, which moves 32 bits: two halves whose totals cannot wrap
    const unsigned long long w = (unsigned long long)(uint32_t)wave_sum((int)(d & 0xFFFFu)) +
                                 ((unsigned long long)(uint32_t)wave_sum((int)(d >> 16)) << 16);
    if ((tid & 63) == 0) atomicAdd(&s_sum, w);
    __syncthreads();
    if (tid == 0) {
        SceneRec r;
        r.diff = s_sum;
        r.flag = r.diff > limit ? 1u : 0u;
        r.pad = 0;
        recs[f] = r;
        h_recs[f] = r;
        __threadfence_system();
    }
}

}  // namespace m2v
