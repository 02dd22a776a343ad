// m2v_deint.hip — m2v_deinterlace_device: woven 4:2:0 frames in device memory to progressive frames (include/m2v_mi355x.h has the
// definition to the bit).  The entry, k_deint and its launch.  Every function that decides a byte or an address is in
// m2v_deint_kernels.hpp, for the device and the host alike; the kernel touches no device global and nothing of m2v_kernels.hpp, so it
// lives here with its launch, as the resampler's does in m2v_scale.hip.
#include "m2v_host.hpp"
#include "m2v_deint_kernels.hpp"

namespace m2v {
namespace {

using namespace deint;

// a lane's kVec bytes of the rows of a tile: the three source frames and the two outputs at the lane's column of the plane.  A lane whose
// bytes all lie inside the row moves them with one 16-byte instruction, at whatever address the row starts (global memory takes any
// alignment); the lane the row ends in moves its n < kVec bytes one by one.
struct LaneIO {
    const uint8_t *src[3];
    uint8_t *dst[2];
    uint32_t rb, n;
    __device__ Vec load(int which, uint32_t y) const
    {
        Vec v{};
        const uint8_t *p = src[which] + y * rb;
        if (n == (uint32_t)kVec) {
            __builtin_memcpy(&v, p, kVec);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < (uint32_t)kVec; ++i)
                if (i < n) v.d[i >> 2] |= (uint32_t)p[i] << (8u * (i & 3u));
        }
        return v;
    }
    __device__ void store(int out, uint32_t y, const Vec &v) const
    {
        uint8_t *p = dst[out] + y * rb;
        if (n == (uint32_t)kVec) {
            __builtin_memcpy(p, &v, kVec);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < (uint32_t)kVec; ++i)
                if (i < n) p[i] = (uint8_t)(v.d[i >> 2] >> (8u * (i & 3u)));
        }
    }
};

// One launch for all frames, planes and outputs of a call.  A work item is one tile (kTileRows rows of kTileCols bytes) of one plane of
// one frame; kLanes = 16 lanes share it, each walking down the rows with kVec = 16 bytes of them: a wave instruction moves four tiles'
// rows, 256 contiguous bytes each, and the four tiles lie next to each other along the row where the plane is that wide.  Items are
// numbered frame by frame and handed out grid-strided (the grid is capped at kMaxBlocks).  The rows above and below are carried in
// registers (deint::walk), samples stay packed four to a dword; no LDS.  Offsets inside a frame fit 32 bits (16384 * 16384 * 3 / 2), a
// frame's place is 64 bits.  HBM traffic: what the mode must read (the row above and below a strip once more) and the outputs.
template <int MODE, int RATE>
__global__ __launch_bounds__(kBlock) void k_deint(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, Frame fr, uint64_t nframes, uint32_t p)
{
    const uint32_t lane = threadIdx.x & (kLanes - 1u);
    const uint64_t items = nframes * fr.tiles, step = (uint64_t)gridDim.x * kItemsPerBlock;
    for (uint64_t it = (uint64_t)blockIdx.x * kItemsPerBlock + (threadIdx.x / kLanes); it < items; it += step) {
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

struct DeintArgs { const uint8_t *src; size_t nframes; int w, h, layout, mode, rate, order; uint8_t *dst; hipStream_t s; };

int deint_impl(m2v_enc *e, void *argp)
{
    auto *a = (DeintArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    const Frame fr = make_frame(a->layout, (uint32_t)a->w, (uint32_t)a->h);
    const uint64_t n = a->nframes, items = n * fr.tiles;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((items + kItemsPerBlock - 1) / kItemsPerBlock, kMaxBlocks);
    const uint32_t p = (uint32_t)a->order;
    timer_break(e);
    const dim3 g(grid), b(kBlock);
    if (a->mode == M2V_DEINT_BLEND) hipLaunchKernelGGL((k_deint<kBlend, kFrameRate>), g, b, 0, s, a->src, a->dst, fr, n, p);
    else if (a->mode == M2V_DEINT_LINE && a->rate == M2V_DEINT_FRAME_RATE) hipLaunchKernelGGL((k_deint<kLine, kFrameRate>), g, b, 0, s, a->src, a->dst, fr, n, p);
    else if (a->mode == M2V_DEINT_LINE) hipLaunchKernelGGL((k_deint<kLine, kFieldRate>), g, b, 0, s, a->src, a->dst, fr, n, p);
    else if (a->rate == M2V_DEINT_FRAME_RATE) hipLaunchKernelGGL((k_deint<kAdaptive, kFrameRate>), g, b, 0, s, a->src, a->dst, fr, n, p);
    else hipLaunchKernelGGL((k_deint<kAdaptive, kFieldRate>), g, b, 0, s, a->src, a->dst, fr, n, p);
    HIPCHK(hipGetLastError());
    return M2V_OK;
}

}  // namespace
}  // namespace m2v

extern "C" {

using namespace m2v;

unsigned long long m2v_deinterlace_bound(int width, int height, size_t nframes, int rate)
{
    static_assert(M2V_DEINT_LINE == deint::kLine && M2V_DEINT_ADAPTIVE == deint::kAdaptive && M2V_DEINT_BLEND == deint::kBlend &&
                  M2V_DEINT_FRAME_RATE == deint::kFrameRate && M2V_DEINT_FIELD_RATE == deint::kFieldRate && M2V_DEINT_TFF == deint::kTff &&
                  M2V_DEINT_BFF == deint::kBff, "include/m2v_mi355x.h and m2v_deint_kernels.hpp");
    return deint::bound(width, height, nframes, rate);
}

int m2v_deinterlace_tile(int *cols, int *rows)
{
    if (cols) *cols = deint::kTileCols;
    if (rows) *rows = deint::kTileRows;
    return M2V_OK;
}

int m2v_deinterlace_device(m2v_enc *e, const void *d_src, size_t nframes, int width, int height, int layout, int mode, int rate, int order,
                           void *d_dst, size_t cap, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    static_assert(M2V_OK == deint::kOk && M2V_E_PARAM == deint::kParam && M2V_E_OVERFLOW == deint::kOverflow, "include/m2v_mi355x.h and m2v_deint_kernels.hpp");
    const char *why = "";
    const int r = deint::check_args((uintptr_t)d_src, nframes, width, height, layout, mode, rate, order, (uintptr_t)d_dst, cap, &why);
    if (r != M2V_OK) {
        e->set_err("m2v_deinterlace_device: %s (%zu frames of %d x %d, layout %d, mode %d, rate %d, order %d, cap %zu)", why, nframes, width, height, layout, mode,
                   rate, order, cap);
        return r;
    }
    if (in_progress(e, "m2v_deinterlace_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    if (!nframes) return M2V_OK;
    DeintArgs a{(const uint8_t *)d_src, nframes, width, height, layout, mode, rate, order, (uint8_t *)d_dst, (hipStream_t)hip_stream};
    return guard(e, deint_impl, &a);
}

}  // extern "C"
