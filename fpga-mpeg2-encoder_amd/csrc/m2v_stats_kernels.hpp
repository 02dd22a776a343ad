// m2v_stats_kernels.hpp — device code of option "stats" (m2v_stats.hip tells the whole story): k_picstat, the squared error of a GOP
// step's pictures against their reconstruction, and k_picstat_mb, the macroblock counts and bits of a chunk's pictures.  Included by
// m2v_launch.hip behind m2v_kernels.hpp, whose tile offsets (rec_luma_off / rec_chroma_off), packed means (avg2x4) and wave_sum it uses:
// that header defines kernels and device globals with external linkage, so one unit only can include it.
#pragma once
#include "../../include/m2v_mi355x.h"
#include "m2v_kernels.hpp"

static_assert(offsetof(m2v_picture_stat, sse) == 8 && offsetof(m2v_picture_stat, mb_bits) == 32 && offsetof(m2v_picture_stat, reserved) == 60,
              "k_picstat and k_picstat_mb fill the record in place");

namespace m2v {

constexpr int kStatThreads = 256;
constexpr int kStatWaves = kStatThreads / 64;
// A wavefront's unit of work is 8 reconstruction tiles of one tile row (8 macroblocks' worth of samples); it takes at most this many
// before it adds to the block's sums.  A lane sees 32 luma samples per unit, <= 32 x 255^2 = 2.08e6, so its 32-bit sums hold and the
// wavefront's total (x 64 lanes x 4 units = 5.3e8) still fits the signed DPP sum; from there on the sums are 64-bit.
constexpr int kUnitsPerWave = 4;
constexpr uint32_t kSliceHeaderBits = 38;      // k_slice_scan counts the slice header with the first macroblock of a row

struct StatRegion { int w, h, cw, ch; };       // measured region: luma w x h, each chroma plane cw x ch (top left)

// what a lane loads at once, through explicit global-address-space pointers like k_mb's (a pointer that comes out of a FrameJob is a
// generic one to the compiler: flat loads).  8 source bytes: a caller's frames are only known to be dword aligned
typedef uint32_t src8_t __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t rec8_t __attribute__((ext_vector_type(2)));
typedef uint32_t rec16_t __attribute__((ext_vector_type(4)));

// byte mask of the four samples x .. x + 3 that lie in [0, lim)   (x is a multiple of 4)
__device__ __forceinline__ uint32_t keep_bytes(int x, int lim)
{
    const int n = lim - x;
    return x < 0 || n <= 0 ? 0u : n >= 4 ? 0xFFFFFFFFu : (1u << (8 * n)) - 1u;
}

// acc + sum over the four bytes of (a - b)^2, as a.a + b.b - 2 a.b on the dot-product unit
__device__ __forceinline__ uint32_t sq_err4(uint32_t a, uint32_t b, uint32_t acc)
{
    acc = __builtin_amdgcn_udot4(a, a, acc, false);
    acc = __builtin_amdgcn_udot4(b, b, acc, false);
    return acc - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}

// grid = (blocks, pictures of the launch list); jobs = the list as jobs (k_mb's own array: fidx = the picture's index in the chunk).
// Lane (p = lane >> 3, t = lane & 7) of a unit takes luma rows 2p, 2p + 1 of tile t: 32 contiguous bytes of the shifted tile
// (rec_luma_off), 8 + 8 of the chroma tile's row p, and from the source the same 16 columns of two rows of Y, U and V - eight lanes
// of one p read 128 contiguous bytes of a source row, the wavefront 2 KB of contiguous luma tiles.  The source chroma is formed with
// k_mb's two packed means.  The outer half of the first and last tile column lies outside the picture: masked, like everything
// outside the measured region.
__global__ __launch_bounds__(kStatThreads) void k_picstat(const FrameJob *__restrict__ jobs, Geom g, StatRegion m, m2v_picture_stat *__restrict__ out)
{
    __shared__ unsigned long long s_acc[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 3) s_acc[threadIdx.x] = 0ull;
    __syncthreads();
    const FrameJob job = jobs[blockIdx.y];
    if (!job.rec) return;                                      // (block-uniform; plan_chunk gives every picture a slot while the option is on)
    const uint32_t tw = (uint32_t)g.mbw + 1u, ngrp = (tw + 7u) >> 3, units = ngrp * (uint32_t)g.mbh;
    const uint32_t t8 = (uint32_t)lane & 7u, p = (uint32_t)lane >> 3;
    const bool cut = job.valid_beats < (g.ysz >> 2);           // a frame cut short by the stop: its later beats are black (RTL:1048-1056)
    const uint8_t *inY = job.in, *inU = inY + g.ysz, *inV = inU + g.ysz;
    uint32_t sy = 0, su = 0, sv = 0;
    for (uint32_t u = blockIdx.x * kStatWaves + (uint32_t)wave; u < units; u += gridDim.x * kStatWaves) {
        const uint32_t ty = u / ngrp, tx = (u - ty * ngrp) * 8u + t8;
        if (tx >= tw) continue;
        const int x0 = 16 * (int)tx - 8, c0 = 8 * (int)tx - 4;              // the tile's first luma / chroma column
        const uint32_t y0 = 16u * ty + 2u * p, cy = 8u * ty + p;
        // every load of the unit is issued before anything waits for one: the wavefront pays one memory round trip per unit
        uint32_t Y[2][4], U[2][4], V[2][4], off[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // (a half outside the picture reads the row's first / last eight samples instead: every byte of it is masked below)
                const int xs = x0 + 8 * h < 0 ? 0 : x0 + 8 * h >= g.W ? g.W - 8 : x0 + 8 * h;
                off[r][h] = (y0 + (uint32_t)r) * (uint32_t)g.W + (uint32_t)xs;
                const src8_t a = *(const __attribute__((address_space(1))) src8_t *)(inY + off[r][h]);
                const src8_t b = *(const __attribute__((address_space(1))) src8_t *)(inU + off[r][h]);
                const src8_t c = *(const __attribute__((address_space(1))) src8_t *)(inV + off[r][h]);
                Y[r][2 * h] = a.x; Y[r][2 * h + 1] = a.y;
                U[r][2 * h] = b.x; U[r][2 * h + 1] = b.y;
                V[r][2 * h] = c.x; V[r][2 * h + 1] = c.y;
            }
        const auto *rl = (const __attribute__((address_space(1))) rec16_t *)(job.rec + rec_luma_off((uint32_t)x0, y0, g));      // rows y0 and y0 + 1 of the tile follow each other
        const rec16_t ra = rl[0], rb = rl[1];
        const uint32_t co = rec_chroma_off(0u, (uint32_t)c0, cy, g);
        const rec8_t ru = *(const __attribute__((address_space(1))) rec8_t *)(job.rec + co), rv = *(const __attribute__((address_space(1))) rec8_t *)(job.rec + co + 64u);
        if (cut) {                              // block-uniform, almost never: a beat is four samples of each plane
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((off[r][k >> 1] >> 2) + (uint32_t)(k & 1) >= job.valid_beats) { Y[r][k] = 0u; U[r][k] = 0x80808080u; V[r][k] = 0x80808080u; }
        }
        const uint32_t R[2][4] = {{ra.x, ra.y, ra.z, ra.w}, {rb.x, rb.y, rb.z, rb.w}};
        const uint32_t row_in[2] = {(int)y0 < m.h ? 0xFFFFFFFFu : 0u, (int)y0 + 1 < m.h ? 0xFFFFFFFFu : 0u};
        const uint32_t crow_in = (int)cy < m.ch ? 0xFFFFFFFFu : 0u;
        uint32_t cu[4], cv[4];                  // the 4:2:0 samples, in bytes 0 and 2 (RTL:1086-1089 horizontal mean2, RTL:1167-1170 vertical mean2 of the two means)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t keep = keep_bytes(x0 + 4 * k, m.w);
            sy = sq_err4(Y[0][k] & keep & row_in[0], R[0][k] & keep & row_in[0], sy);
            sy = sq_err4(Y[1][k] & keep & row_in[1], R[1][k] & keep & row_in[1], sy);
            cu[k] = avg2x4(avg2x4(U[0][k], U[0][k] >> 8), avg2x4(U[1][k], U[1][k] >> 8));
            cv[k] = avg2x4(avg2x4(V[0][k], V[0][k] >> 8), avg2x4(V[1][k], V[1][k] >> 8));
        }
        const uint32_t RU[2] = {ru.x, ru.y}, RV[2] = {rv.x, rv.y};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t keep = keep_bytes(c0 + 4 * j, m.cw) & crow_in;
            su = sq_err4(__builtin_amdgcn_perm(cu[2 * j + 1], cu[2 * j], 0x06040200u) & keep, RU[j] & keep, su);
            sv = sq_err4(__builtin_amdgcn_perm(cv[2 * j + 1], cv[2 * j], 0x06040200u) & keep, RV[j] & keep, sv);
        }
    }
    const int wy = wave_sum((int)sy), wu = wave_sum((int)su), wv = wave_sum((int)sv);
    if (lane == 0) {
        atomicAdd(&s_acc[0], (unsigned long long)(uint32_t)wy);
        atomicAdd(&s_acc[1], (unsigned long long)(uint32_t)wu);
        atomicAdd(&s_acc[2], (unsigned long long)(uint32_t)wv);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_acc[threadIdx.x]) atomicAdd((unsigned long long *)&out[job.fidx].sse[threadIdx.x], s_acc[threadIdx.x]);
}

// one block per picture of the chunk: everything of its record but the three sums above (which it leaves alone)
__global__ __launch_bounds__(kStatThreads) void k_picstat_mb(const FrameJob *__restrict__ jobs, Geom g, const uint32_t *__restrict__ mbinfo,
                                                             const uint32_t *__restrict__ mblen, m2v_picture_stat *__restrict__ out)
{
    __shared__ uint32_t s_sum[5];
    const uint32_t f = blockIdx.x;
    if (threadIdx.x < 5) s_sum[threadIdx.x] = 0u;
    __syncthreads();
    const size_t base = (size_t)f * (size_t)g.mbs;
    uint32_t bits = 0, inter = 0, coded = 0, ax = 0, ay = 0;       // (a picture's bits: at most 16384 macroblocks x 9300 < 2^32)
    for (uint32_t i = threadIdx.x; i < (uint32_t)g.mbs; i += kStatThreads) {
        const uint32_t info = mbinfo[base + i];
        bits += mblen[base + i];
        inter += info & 1u;
        coded += (uint32_t)__popc((info >> 1) & 63u);
        if (info & 1u) { ax += (uint32_t)iabs(sext((int)(info >> 8), 8)); ay += (uint32_t)iabs(sext((int)(info >> 16), 8)); }
    }
    atomicAdd(&s_sum[0], bits); atomicAdd(&s_sum[1], inter); atomicAdd(&s_sum[2], coded); atomicAdd(&s_sum[3], ax); atomicAdd(&s_sum[4], ay);
    __syncthreads();
    if (threadIdx.x == 0) {
        m2v_picture_stat &r = out[f];
        r.frame = jobs[f].n;
        r.coding_type = jobs[f].i_frame == 0 ? 1u : 2u;
        r.mb_bits = (uint64_t)(s_sum[0] - kSliceHeaderBits * (uint32_t)g.mbh);
        r.intra_mbs = (uint32_t)g.mbs - s_sum[1];
        r.inter_mbs = s_sum[1];
        r.coded_blocks = s_sum[2];
        r.mv_abs_x = s_sum[3];
        r.mv_abs_y = s_sum[4];
        r.reserved = 0u;
    }
}

}  // namespace m2v
