// deint_host.hpp — csrc/m2v_deint_kernels.hpp walked on a CPU as k_deint walks it (csrc/m2v_deint.hip): the grid of blocks, the threads of
// a block, the items handed out grid-strided, sixteen lanes a tile, each with its 16 bytes of the rows - and the lane the row ends in
// with fewer.  Every byte is read and written at its own address and nothing beyond it, so a sanitizer sees what a lane would touch.
// Shared by tests/deint_cases.py (compiled into a library of its own) and tools/deint_host_check.cpp (the stand-alone program).
#pragma once
#include <cstring>

#include "m2v_deint_kernels.hpp"

namespace deint_host {

using namespace m2v::deint;

struct LaneIO {
    const uint8_t *src[3];
    uint8_t *dst[2];
    uint32_t rb, n;
    Vec load(int which, uint32_t y) const
    {
        uint8_t b[kVec] = {};
        memcpy(b, src[which] + (size_t)y * rb, n);
        Vec v{};
        for (uint32_t i = 0; i < (uint32_t)kVec; ++i) v.d[i >> 2] |= (uint32_t)b[i] << (8u * (i & 3u));
        return v;
    }
    void store(int out, uint32_t y, const Vec &v) const
    {
        uint8_t b[kVec];
        for (uint32_t i = 0; i < (uint32_t)kVec; ++i) b[i] = (uint8_t)(v.d[i >> 2] >> (8u * (i & 3u)));
        memcpy(dst[out] + (size_t)y * rb, b, n);
    }
};

template <int MODE, int RATE>
void kernel(uint32_t blocks, const uint8_t *src, uint8_t *dst, const Frame &fr, uint64_t nframes, uint32_t p)
{
    for (uint32_t block = 0; block < blocks; ++block)
        for (uint32_t tid = 0; tid < (uint32_t)kBlock; ++tid) {
            const uint32_t lane = tid & (kLanes - 1u);
            const uint64_t items = nframes * fr.tiles, step = (uint64_t)blocks * kItemsPerBlock;
            for (uint64_t it = (uint64_t)block * kItemsPerBlock + (tid / kLanes); it < items; it += step) {
                const uint64_t f = it / fr.tiles;
                uint32_t y0, x0;
                Plane pl;
                tile_of(fr, (uint32_t)(it - f * fr.tiles), pl, y0, x0);
                const uint32_t x = x0 + lane * kVec;
                if (x >= pl.rb) continue;
                uint64_t fP, fN;
                walk_frames(f, nframes, fP, fN);
                LaneIO io;
                const size_t at = (size_t)pl.off + x;
                io.src[0] = src + f * fr.bytes + at;
                io.src[1] = src + fP * fr.bytes + at;
                io.src[2] = src + fN * fr.bytes + at;
                io.dst[0] = dst + out_frame(f, RATE, 0) * fr.bytes + at;
                io.dst[1] = dst + out_frame(f, RATE, 1) * fr.bytes + at;
                io.rb = pl.rb;
                io.n = pl.rb - x < (uint32_t)kVec ? pl.rb - x : (uint32_t)kVec;
                const uint32_t y1 = y0 + kTileRows < pl.rows ? y0 + kTileRows : pl.rows;
                walk<MODE, RATE>(io, pl.rows, y0, y1, p);
            }
        }
}

// what m2v_deinterlace_device does with legal arguments, on `max_blocks` blocks at most (0: the kernel's own cap); its answer otherwise
inline int run(const uint8_t *src, uint64_t nframes, int w, int h, int layout, int mode, int rate, int order, uint8_t *dst, uint64_t cap, uint32_t max_blocks)
{
    const int r = check_args((uint64_t)(uintptr_t)src, nframes, w, h, layout, mode, rate, order, (uint64_t)(uintptr_t)dst, cap, nullptr);
    if (r != kOk || !nframes) return r;
    const Frame fr = make_frame(layout, (uint32_t)w, (uint32_t)h);
    const uint64_t items = nframes * fr.tiles, want = (items + kItemsPerBlock - 1) / kItemsPerBlock, most = max_blocks ? max_blocks : (uint32_t)kMaxBlocks;
    const uint32_t blocks = (uint32_t)(want < most ? want : most), p = (uint32_t)order;
    if (mode == kBlend) kernel<kBlend, kFrameRate>(blocks, src, dst, fr, nframes, p);
    else if (mode == kLine && rate == kFrameRate) kernel<kLine, kFrameRate>(blocks, src, dst, fr, nframes, p);
    else if (mode == kLine) kernel<kLine, kFieldRate>(blocks, src, dst, fr, nframes, p);
    else if (rate == kFrameRate) kernel<kAdaptive, kFrameRate>(blocks, src, dst, fr, nframes, p);
    else kernel<kAdaptive, kFieldRate>(blocks, src, dst, fr, nframes, p);
    return kOk;
}

}  // namespace deint_host
