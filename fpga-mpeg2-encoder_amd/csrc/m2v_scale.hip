// m2v_scale.hip — m2v_set_source_size: frames of another size, resampled to the picture size on the device in front of the conversions
// (include/m2v_mi355x.h has the definition to the bit).  The setting, the tap tables (m2v_scale_taps is their single source), k_scale and
// its launch.  Every function that decides a byte is in m2v_scale_kernels.hpp, for the device and the host alike; the kernel touches no
// device global and nothing of m2v_kernels.hpp, so it lives here with its launch, as the muxer's do in m2v_mux.hip.
#include "m2v_host.hpp"
#include "m2v_scale_kernels.hpp"

namespace m2v {
namespace {

using namespace scale;

// One tile of one plane of one frame per block: kTileRows rows of kTileCols bytes of the padded plane (grid: x = the tile, y = the plane,
// z = frames, strided).  A plane is scols x srows elements of es bytes (1: a planar sample, 2: an NV12 chroma pair, 3 / 4: an RGB pixel),
// every byte of an element filtered on its own; ES is the run's largest element, and a run of ES = 2 also holds its luma plane.
//   - the tile's taps go to LDS once: one Taps per byte column (the column's element, clamped to the last: the edge repeat) and per row
//   - horizontal pass: the source rows that the tile's vertical taps reach (tile_span: 73 at most, at a ratio of 8), one thread per byte
//     column and every fourth row, from global memory - byte loads at any address, a wavefront's 64 columns next to each other - into LDS
//     as 16-bit values
//   - vertical pass from LDS: a thread makes two neighbouring bytes of one row; they meet in LDS and 32 lanes store 16 aligned bytes each.
//     Only the W / 2-byte chroma rows of I420 / YV12, which start 8-byte aligned, are stored byte by byte (Plane::vec = 0).
// Products are v_mad_u32_u24 (coefficients below 2^15, samples below 2^14); both passes take four taps per step (hpass, vpass).  Offsets inside a plane fit 32 bits (16384 * 16384 * 4), the
// frame's place is 64 bits.  dst 16-byte aligned.  HBM traffic: the source rows under the tile's columns in (rows shared by two tiles
// above each other twice), the padded frame out.
template <int ES>
__global__ __launch_bounds__(256) void k_scale(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const Taps *__restrict__ tabs, Run run,
                                               size_t sstride, size_t dstride, uint32_t nframes)
{
    __shared__ uint16_t t[kMaxSpan * kTileCols];
    __shared__ Taps hts[kTileCols], vts[kTileRows];
    __shared__ uint4 stage[kTileRows * kTileCols / 16];
    const Plane &p = run.p[blockIdx.y];
    const uint32_t es = ES == 2 ? p.es : (uint32_t)ES;
    const uint32_t srow = p.scols * es, drow = p.COLS * es, tiles_x = (drow + kTileCols - 1) / kTileCols;
    if (blockIdx.x >= tiles_x * (p.ROWS / kTileRows)) return;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * kTileRows, xb0 = tx * kTileCols;
    const uint32_t tid = threadIdx.x, col = tid & (kTileCols - 1);
    const Taps *ht = tabs + p.htab, *vt = tabs + p.vtab;
    uint32_t xo, b;
    column(xb0 + col, es, p.w, xo, b);
    const bool live = xb0 + col < drow;
    if (tid < kTileCols) hts[tid] = ht[xo];
    else if (tid < kTileCols + kTileRows) vts[tid - kTileCols] = vt[row_of(y0 + tid - kTileCols, p.h)];
    int rlo, rhi;
    tile_span(vt, y0, p.h, p.srows, rlo, rhi);
    const uint32_t span = (uint32_t)(rhi - rlo + 1);
    const uint32_t ry = tid >> 5, c2 = (tid & 31u) * 2u;
    __syncthreads();
    for (uint32_t f = blockIdx.z; f < nframes; f += gridDim.z) {
        const uint8_t *sp = src + (size_t)f * sstride + p.soff;
        uint8_t *dp = dst + (size_t)f * dstride + p.doff;
        if (live)
            for (uint32_t rr = tid >> 6; rr < span; rr += 4u)
                t[rr * kTileCols + col] = (uint16_t)hpass(sp + ((uint32_t)rlo + rr) * srow, es, b, hts[col], p.scols);
        __syncthreads();
        const uint32_t o0 = vpass(t + c2, kTileCols, rlo, vts[ry], p.srows), o1 = vpass(t + c2 + 1, kTileCols, rlo, vts[ry], p.srows);
        const uint32_t at = (y0 + ry) * drow + xb0 + c2;
        if (p.vec) {
            ((uint16_t *)stage)[tid] = (uint16_t)(o0 | (o1 << 8));
            __syncthreads();
            // (a row is whole 16-byte pieces here: a piece is inside the row or outside it)
            if (tid < 32u && xb0 + (tid & 3u) * 16u < drow) *(uint4 *)(dp + (y0 + (tid >> 2)) * drow + xb0 + (tid & 3u) * 16u) = stage[tid];
        } else {
            if (xb0 + c2 < drow) dp[at] = (uint8_t)o0;
            if (xb0 + c2 + 1u < drow) dp[at + 1u] = (uint8_t)o1;
        }
        __syncthreads();
    }
}

// what a run kind is to make_run: its form and, for packed pixels, their bytes
void run_form(int kind, int &form, int &es)
{
    es = 1;
    if (kind >= kPkRgb) {
        const int layout = (kind - kPkRgb) & 7;
        form = layout == M2V_RGB_RGBP ? kPlanar3 : kPacked;
        es = rgb_bpp(layout);
    } else if (kind == kPk444) {
        form = kPlanar3;
    } else {
        const int layout = kind - kPk420;
        form = layout == M2V_420_NV12 || layout == M2V_420_NV21 ? k420Semi : k420Planar;
    }
}

}  // namespace

void scale_prepare(m2v_enc *e, hipStream_t s)
{
    const SrcSize a = e->seq.src, b = e->seq.pic;
    const int key[5] = {a.w, a.h, b.w, b.h, e->seq.filter};
    if (e->d_scale_tab.p && !memcmp(key, e->scale_key, sizeof key)) return;
    // luma horizontal, luma vertical, chroma horizontal, chroma vertical: where make_run looks for them
    const int dims[4][2] = {{a.w, b.w}, {a.h, b.h}, {chroma(a.w), chroma(b.w)}, {chroma(a.h), chroma(b.h)}};
    size_t n = 0;
    for (auto &d : dims) n += (size_t)d[1];
    const size_t bytes = n * sizeof(Taps);
    if (e->h_scale_cap < bytes) {
        if (e->h_scale_tab) (void)hipHostFree(e->h_scale_tab);
        e->h_scale_tab = nullptr;
        e->h_scale_cap = 0;
        HIPCHK(hipHostMalloc((void **)&e->h_scale_tab, bytes));
        e->h_scale_cap = bytes;
    }
    Taps *t = (Taps *)e->h_scale_tab;
    for (auto &d : dims)
        for (int x = 0; x < d[1]; ++x)
            HIPCHK(build_taps(e->seq.filter, d[0], d[1], x, *t++) > 0 ? hipSuccess : hipErrorInvalidValue);       // (the starting call has checked the ratio)
    // (k_scale keeps a tile's horizontal results in kMaxSpan rows of LDS)
    const Taps *vt = (const Taps *)e->h_scale_tab + b.w;
    for (int c = 0; c < 2; ++c, vt += b.h + chroma(b.w)) {
        const uint32_t h = (uint32_t)dims[2 * c + 1][1], srows = (uint32_t)dims[2 * c + 1][0];
        for (uint32_t y0 = 0; y0 < h; y0 += kTileRows) {
            int rlo, rhi;
            tile_span(vt, y0, h, srows, rlo, rhi);
            HIPCHK(rhi >= rlo && rhi - rlo < kMaxSpan ? hipSuccess : hipErrorInvalidValue);
        }
    }
    e->scale_key[0] = 0;                // (not the handle's until the upload is queued)
    e->d_scale_tab.recorded = false;
    e->d_scale_tab.ensure(bytes);
    HIPCHK(hipMemcpyAsync(e->d_scale_tab.p, e->h_scale_tab, bytes, hipMemcpyHostToDevice, s));
    memcpy(e->scale_key, key, sizeof key);
}

void launch_scale(m2v_enc *e, hipStream_t s, int kind, const uint8_t *src, uint8_t *dst, uint32_t nframes)
{
    const Geom &g = e->g;
    const SrcSize a = e->seq.src, b = e->seq.pic;
    int form = 0, es = 1;
    run_form(kind, form, es);
    const Run run = make_run(form, es, a.w, a.h, b.w, b.h, g.W, g.H);
    const size_t sfb = pk_frame_bytes(kind, g, a), dfb = pk_frame_bytes(kind, g, SrcSize{});
    const Taps *tabs = (const Taps *)e->d_scale_tab.p;
    const dim3 grid(run.max_tiles, run.nplanes, std::min<uint32_t>(nframes, 32768u)), block(256);
    if (form == k420Semi) hipLaunchKernelGGL((k_scale<2>), grid, block, 0, s, src, dst, tabs, run, sfb, dfb, nframes);
    else if (form != kPacked) hipLaunchKernelGGL((k_scale<1>), grid, block, 0, s, src, dst, tabs, run, sfb, dfb, nframes);
    else if (es == 3) hipLaunchKernelGGL((k_scale<3>), grid, block, 0, s, src, dst, tabs, run, sfb, dfb, nframes);
    else hipLaunchKernelGGL((k_scale<4>), grid, block, 0, s, src, dst, tabs, run, sfb, dfb, nframes);
    HIPCHK(hipGetLastError());
}

void scale_release(m2v_enc *e)
{
    e->d_scale_tab.release();
    if (e->h_scale_tab) (void)hipHostFree(e->h_scale_tab);
    e->h_scale_tab = nullptr;
    e->h_scale_cap = 0;
    e->scale_key[0] = 0;
}

}  // namespace m2v

extern "C" {

int m2v_scale_taps(int filter, int src, int dst, int x, int *first, uint16_t coeff[M2V_SCALE_MAXTAPS])
{
    static_assert(M2V_SCALE_MAXTAPS == m2v::scale::kMaxTaps && M2V_SCALE_TRIANGLE == m2v::scale::kTriangle && M2V_SCALE_AREA == m2v::scale::kArea,
                  "include/m2v_mi355x.h and m2v_scale_kernels.hpp");
    m2v::scale::Taps t{};
    const int n = m2v::scale::build_taps(filter, src, dst, x, t);
    if (n < 1) return M2V_E_PARAM;
    if (first) *first = t.first;
    if (coeff) memcpy(coeff, t.c, sizeof t.c);
    return n;
}

int m2v_set_source_size(m2v_enc *e, int src_width, int src_height, int filter)
{
    if (!e) return M2V_E_PARAM;
    if (in_progress(e, "m2v_set_source_size", "the size is sampled when a sequence starts")) return M2V_E_STATE;
    if (filter != M2V_SCALE_TRIANGLE && filter != M2V_SCALE_AREA) { e->set_err("m2v_set_source_size: unknown filter %d", filter); return M2V_E_PARAM; }
    if (src_width < 0 || src_height < 0 || !src_width != !src_height || src_width > m2v::scale::kMaxSize || src_height > m2v::scale::kMaxSize) {
        e->set_err("m2v_set_source_size: %d x %d is no source size (1 ... %d either way, or 0 x 0 for none)", src_width, src_height, m2v::scale::kMaxSize);
        return M2V_E_PARAM;
    }
    // (what the last sequence sampled goes with the old setting)
    e->seq.src = e->seq.pic = SrcSize{};
    e->set.src = SrcSize{src_width, src_height};
    e->set.filter = src_width ? filter : M2V_SCALE_TRIANGLE;
    return M2V_OK;
}

}  // extern "C"
