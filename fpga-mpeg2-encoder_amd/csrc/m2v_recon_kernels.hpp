// m2v_recon_kernels.hpp — device code of m2v_set_recon_out (m2v_recon.hip tells the whole story): k_recon_out, the reconstruction of a
// GOP step's pictures out of their tiled slots into plain 4:2:0 frames in the caller's buffer.  Included by m2v_launch.hip behind
// m2v_kernels.hpp, whose tile offsets (rec_luma_off / rec_chroma_off) it uses: that header defines kernels and device globals with
// external linkage, so one unit only can include it.
#pragma once
#include "../../include/m2v_mi355x.h"
#include "m2v_kernels.hpp"

namespace m2v {

constexpr int kReconThreads = 256;

// The written region and how a picture's work is counted: luma w x h, each chroma plane cw x ch (top left of the coded picture).
// A unit is 16 consecutive output bytes of one row, a wavefront's 64 units are 8 rows of one band of columns: 128 luma columns
// (grp_y bands per picture), or 64 chroma columns of both planes (grp_c bands).  Those are whole cache lines of the tiled
// reconstruction - rows 0 - 7 or 8 - 15 of a luma tile, the 8 x 8 U and V of a chroma tile, are 128 bytes each - every one of which is
// read by one wavefront in one instruction.  magic_* = floor(2^32 / grp_*): the band row by one multiplication (recon_split).
struct ReconOut {
    int w, h, cw, ch;
    uint32_t grp_y, grp_c, magic_y, magic_c;
    uint32_t n_y, n_c;                      // units (64 per wavefront) of the luma plane, of the chroma planes
};

// i = q * d + r with magic = floor(2^32 / d): the estimate is q or q - 1 for every 32-bit i
__device__ __forceinline__ void recon_split(uint32_t i, uint32_t d, uint32_t magic, uint32_t &q, uint32_t &r)
{
    q = __umulhi(i, magic);
    r = i - q * d;
    if (r >= d) { ++q; r -= d; }
}

typedef uint32_t rtile4_t;
typedef uint32_t rtile8_t __attribute__((ext_vector_type(2)));
typedef uint32_t rstore_t __attribute__((ext_vector_type(4), aligned(1)));      // 16, 8, 4, 2 bytes to any address
typedef uint32_t rstore8_t __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t rstore4_t __attribute__((aligned(1)));
typedef uint16_t rstore2_t __attribute__((aligned(1)));

// The lane's 16 bytes v[0 .. 3] to p, of which the first `valid` (> 0) lie inside the row: whole, or - the last lane of a row whose
// length is no multiple of 16 - as the 8, 4, 2 and 1 bytes of valid's binary digits, each store under the lanes that have the digit.
// Nothing past the row's end is stored.
__device__ __forceinline__ void recon_store(uint8_t *p, const uint32_t (&v)[4], int valid)
{
    auto *gp = (__attribute__((address_space(1))) uint8_t *)p;
    if (valid >= 16) {
        *(__attribute__((address_space(1))) rstore_t *)gp = rstore_t{v[0], v[1], v[2], v[3]};
        return;
    }
    uint32_t lo = v[0], hi = v[1];                             // the next eight bytes to go
    if (valid & 8) { *(__attribute__((address_space(1))) rstore8_t *)gp = rstore8_t{lo, hi}; gp += 8; lo = v[2]; hi = v[3]; }
    if (valid & 4) { *(__attribute__((address_space(1))) rstore4_t *)gp = lo; gp += 4; lo = hi; }
    if (valid & 2) { *(__attribute__((address_space(1))) rstore2_t *)gp = (uint16_t)lo; gp += 2; lo >>= 16; }
    if (valid & 1) *gp = (uint8_t)lo;
}

// grid = (blocks, pictures of the launch list); jobs = the list as jobs (k_mb's own array).  One lane per unit, every plane of every
// picture in the one launch.  The loads are the aligned side: a luma unit is the right half of one tile row and the left half of the
// next (two 8-byte loads; tile tx holds columns 16 tx - 8 .. 16 tx + 7), a planar chroma unit a right half, a whole row and a left half
// of three chroma tiles (4 + 8 + 4; tile tx holds columns 8 tx - 4 .. 8 tx + 3), an interleaved one the 4 + 4 bytes of U and of V
// merged with v_perm_b32.  All of a lane's loads are issued before the first is used.  Lane -> unit: luma and interleaved chroma
// (row = lane >> 3, piece = lane & 7): eight lanes store 128 contiguous bytes of a row; planar chroma (plane = lane >> 5, row =
// (lane >> 2) & 7, piece = lane & 3): four lanes store 64.  The store is one global_store_dwordx4 at whatever address the packed output
// gives it (rows of w, cw or 2 cw bytes without padding).  Units outside the region end at once.  Offsets inside a frame are 32 bits
// (2048 x 2048 x 3 / 2), the frame's place in the caller's buffer 64.  No LDS, no scratch.
// LAYOUT = M2V_420_*: bit 1 = interleaved chroma, bit 0 = V first.
template <int LAYOUT>
__global__ __launch_bounds__(kReconThreads) void k_recon_out(const FrameJob *__restrict__ jobs, Geom g, ReconOut m, uint8_t *__restrict__ dst, size_t frame_bytes)
{
    constexpr bool SEMI = (LAYOUT & 2) != 0, VFIRST = (LAYOUT & 1) != 0;
    const FrameJob job = jobs[blockIdx.y];
    if (!job.rec) return;                                      // (block-uniform; plan_chunk gives every picture a slot while a buffer is set)
    const uint32_t idx = blockIdx.x * (uint32_t)kReconThreads + threadIdx.x;
    if (idx >= m.n_y + m.n_c) return;
    const uint8_t *rec = job.rec;
    uint8_t *out = dst + (size_t)job.n * frame_bytes;
    auto ld4 = [&](uint32_t off) { return *(const __attribute__((address_space(1))) rtile4_t *)(rec + off); };
    auto ld8 = [&](uint32_t off) { return *(const __attribute__((address_space(1))) rtile8_t *)(rec + off); };
    const uint32_t ysz = (uint32_t)m.w * (uint32_t)m.h, lane = idx & 63u;
    uint32_t band_row, band;
    if (idx < m.n_y) {
        recon_split(idx >> 6, m.grp_y, m.magic_y, band_row, band);
        const uint32_t y = 8u * band_row + (lane >> 3), x = 128u * band + 16u * (lane & 7u);
        if ((int)y >= m.h || (int)x >= m.w) return;
        const rtile8_t a = ld8(rec_luma_off(x, y, g)), b = ld8(rec_luma_off(x + 8u, y, g));     // (16 s < w <= 16 mbw: tile s + 1 exists)
        const uint32_t v[4] = {a.x, a.y, b.x, b.y};
        recon_store(out + y * (uint32_t)m.w + x, v, m.w - (int)x);
    } else if (SEMI) {
        recon_split((idx - m.n_y) >> 6, m.grp_c, m.magic_c, band_row, band);
        const uint32_t y = 8u * band_row + (lane >> 3), x = 64u * band + 8u * (lane & 7u);      // chroma column; 8 s < cw <= 8 mbw: tile s + 1 exists
        if ((int)y >= m.ch || (int)x >= m.cw) return;
        const uint32_t ou = rec_chroma_off(0u, x, y, g), ou2 = rec_chroma_off(0u, x + 4u, y, g);
        const uint32_t u0 = ld4(ou), u1 = ld4(ou2), v0 = ld4(ou + 64u), v1 = ld4(ou2 + 64u);
        const uint32_t lo0 = VFIRST ? v0 : u0, hi0 = VFIRST ? u0 : v0, lo1 = VFIRST ? v1 : u1, hi1 = VFIRST ? u1 : v1;
        const uint32_t v[4] = {__builtin_amdgcn_perm(hi0, lo0, 0x05010400u), __builtin_amdgcn_perm(hi0, lo0, 0x07030602u),
                               __builtin_amdgcn_perm(hi1, lo1, 0x05010400u), __builtin_amdgcn_perm(hi1, lo1, 0x07030602u)};
        recon_store(out + ysz + (y * (uint32_t)m.cw + x) * 2u, v, 2 * (m.cw - (int)x));
    } else {
        recon_split((idx - m.n_y) >> 6, m.grp_c, m.magic_c, band_row, band);
        const uint32_t second = lane >> 5;                     // the second chroma plane of the frame
        const uint32_t y = 8u * band_row + ((lane >> 2) & 7u), x = 64u * band + 16u * (lane & 3u), pl = second ^ (VFIRST ? 1u : 0u);
        if ((int)y >= m.ch || (int)x >= m.cw) return;
        // (the third piece of a row's last unit may lie past the coded row, in a tile that does not exist: the row's last four samples
        // instead - every byte of it is outside the region, and recon_store leaves it out)
        const uint32_t x3 = min(x + 12u, (uint32_t)g.cw - 4u);
        const rtile4_t a = ld4(rec_chroma_off(pl, x, y, g));
        const rtile8_t b = ld8(rec_chroma_off(pl, x + 4u, y, g));
        const rtile4_t c = ld4(rec_chroma_off(pl, x3, y, g));
        const uint32_t v[4] = {a, b.x, b.y, c};
        recon_store(out + ysz + second * (uint32_t)m.cw * (uint32_t)m.ch + y * (uint32_t)m.cw + x, v, m.cw - (int)x);
    }
}

}  // namespace m2v
