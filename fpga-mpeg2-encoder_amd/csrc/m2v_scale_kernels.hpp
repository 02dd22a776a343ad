// m2v_scale_kernels.hpp — the arithmetic of the resampling pass (m2v_set_source_size; include/m2v_mi355x.h has the definition, m2v_scale.hip
// the kernel and its launch): every function that decides a byte, in __host__ __device__ inline form - the tap builder, the planes of a
// frame, the source rows a tile needs, the two passes and their clamps.  k_scale is a thin loop over these functions, and the same header
// compiles with a plain C++ compiler (the qualifiers defined empty), so the whole pass can be walked tile by tile on a CPU and held
// against the numpy statement of the definition (scale_frames; tests/test_input_scale.py).  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define M2V_SC_HD __host__ __device__
#else
#define M2V_SC_HD
#endif

namespace m2v {
namespace scale {

enum { kTriangle = 0, kArea = 1 };              // M2V_SCALE_TRIANGLE / M2V_SCALE_AREA
constexpr int kMaxTaps = 16;                    // M2V_SCALE_MAXTAPS: what a ratio of 8 needs
constexpr int kMaxSize = 16384;                 // a source dimension
constexpr int kMaxRatio = 8;                    // source over picture, either dimension
constexpr int kTileRows = 8, kTileCols = 64;    // a block's tile: rows x bytes of a padded row
// source rows under a tile: the last row's last tap minus the first row's first, ((2 * 7 + 1) * src + 2 * R) / (2 * dst) + 1 <= 9 * 8 + 1
constexpr int kMaxSpan = 76;

// the taps of one output sample: samples first .. first + n - 1 (clamped to the plane when read), coefficients that sum to 2^14
// (both passes take the taps four at a time, the coefficients beyond n being 0: four loads in flight instead of one)
struct alignas(8) Taps { int32_t first; uint32_t n; uint16_t c[kMaxTaps]; };      // 40 bytes

M2V_SC_HD inline long long floordiv(long long a, long long b) { const long long q = a / b; return a % b < 0 ? q - 1 : q; }        // b > 0
M2V_SC_HD inline int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
M2V_SC_HD inline uint32_t minu(uint32_t a, uint32_t b) { return a < b ? a : b; }
M2V_SC_HD inline int chroma(int v) { return (v + 1) / 2; }       // samples of a 4:2:0 chroma plane along a dimension of v luma samples

// c * v + acc, c and v below 2^24 (one v_mad_u32_u24)
M2V_SC_HD inline uint32_t mad24(uint32_t c, uint32_t v, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(c, v) + acc;
#else
    return c * v + acc;
#endif
}

// the taps of output sample x of dst, from src samples, sample centres aligned.  Returns n, or -1 for arguments out of range.
M2V_SC_HD inline int build_taps(int filter, int src, int dst, int x, Taps &t)
{
    if ((filter != kTriangle && filter != kArea) || src < 1 || dst < 1 || src > kMaxSize || dst > kMaxSize || x < 0 || x >= dst) return -1;
    if ((long long)src > (long long)kMaxRatio * dst) return -1;
    long long a[kMaxTaps], lo, hi, A = 0;
    int n = 0;
    if (filter == kTriangle) {
        // a(i) = R - |D * i - P| > 0: P - R < D * i < P + R
        const long long P = (2ll * x + 1) * src - dst, R = 2ll * (src > dst ? src : dst), D = 2ll * dst;
        lo = floordiv(P - R, D) + 1;
        hi = floordiv(P + R - 1, D);
        for (long long i = lo; i <= hi; ++i) {
            if (n == kMaxTaps) return -1;
            const long long d = D * i - P;
            a[n++] = R - (d < 0 ? -d : d);
        }
    } else {
        // the part of source sample i under output sample x, both scaled to src * dst
        const long long x0 = (long long)x * src, x1 = x0 + src;
        lo = floordiv(x0, dst);
        hi = floordiv(x1 - 1, dst);
        for (long long i = lo; i <= hi; ++i) {
            if (n == kMaxTaps) return -1;
            const long long s0 = i * dst, s1 = s0 + dst;
            a[n++] = (s1 < x1 ? s1 : x1) - (s0 > x0 ? s0 : x0);
        }
    }
    int best = 0;
    for (int k = 0; k < n; ++k) { A += a[k]; if (a[k] > a[best]) best = k; }
    uint32_t sum = 0;
    for (int k = 0; k < kMaxTaps; ++k) {
        t.c[k] = k < n ? (uint16_t)((a[k] << 14) / A) : 0;
        sum += t.c[k];
    }
    t.c[best] = (uint16_t)(t.c[best] + ((1u << 14) - sum));
    t.first = (int32_t)lo;
    t.n = (uint32_t)n;
    return n;
}

// One plane of a frame: scols x srows elements of es bytes at soff in the source frame -> w x h, written as COLS x ROWS (whole
// macroblocks: the last column and row repeated) at doff in the padded frame.  htab / vtab: where its tables start among the four.
struct Plane { uint32_t soff, doff, scols, srows, w, h, COLS, ROWS, es, htab, vtab, vec; };
struct Run { Plane p[3]; uint32_t nplanes, max_tiles; };

enum { kPlanar3 = 0, k420Planar = 1, k420Semi = 2, kPacked = 3 };      // three full planes; Y + two chroma planes; Y + one plane of pairs; one plane of pixels

M2V_SC_HD inline uint32_t plane_tiles(const Plane &p) { return ((p.COLS * p.es + kTileCols - 1) / kTileCols) * (p.ROWS / kTileRows); }

// the planes of a run of `form` (kPacked: pixels of es bytes): sw x sh -> w x h, padded to W x H.  The tables lie luma horizontal (w
// entries), luma vertical (h), chroma horizontal (cw), chroma vertical (ch).
M2V_SC_HD inline Run make_run(int form, int es, int sw, int sh, int w, int h, int W, int H)
{
    Run r{};
    const uint32_t px = (uint32_t)sw * sh, ysz = (uint32_t)W * H;
    const uint32_t scw = chroma(sw), sch = chroma(sh), cw = chroma(w), ch = chroma(h);
    const Plane luma{0, 0, (uint32_t)sw, (uint32_t)sh, (uint32_t)w, (uint32_t)h, (uint32_t)W, (uint32_t)H, 1, 0, (uint32_t)w, 1};
    Plane c{px, ysz, scw, sch, cw, ch, (uint32_t)W / 2, (uint32_t)H / 2, 1, (uint32_t)(w + h), (uint32_t)(w + h) + cw, 1};
    r.p[0] = luma;
    switch (form) {
    case kPlanar3:
        for (uint32_t k = 1; k < 3; ++k) { r.p[k] = luma; r.p[k].soff = k * px; r.p[k].doff = k * ysz; }
        r.nplanes = 3;
        break;
    case k420Planar:
        c.vec = (W / 2) % 16 == 0;          // a row of W / 2 bytes starts 8-byte aligned only
        r.p[1] = c;
        c.soff += scw * sch; c.doff += ysz >> 2;
        r.p[2] = c;
        r.nplanes = 3;
        break;
    case k420Semi:
        c.es = 2;
        r.p[1] = c;
        r.nplanes = 2;
        break;
    default:
        r.p[0].es = (uint32_t)es;
        r.nplanes = 1;
    }
    for (uint32_t k = 0; k < r.nplanes; ++k) { const uint32_t t = plane_tiles(r.p[k]); if (t > r.max_tiles) r.max_tiles = t; }
    return r;
}

// byte xb of a padded row of elements of es bytes -> the output sample whose taps it takes (past the last column: the last column's)
// and its byte of the element
M2V_SC_HD inline void column(uint32_t xb, uint32_t es, uint32_t w, uint32_t &xo, uint32_t &b)
{
    const uint32_t el = xb / es;
    b = xb - el * es;
    xo = minu(el, w - 1u);
}

// the output row whose taps padded row y takes
M2V_SC_HD inline uint32_t row_of(uint32_t y, uint32_t h) { return minu(y, h - 1u); }

// the source rows rlo .. rhi (clamped to the plane) that the vertical taps of padded rows y0 .. y0 + kTileRows - 1 reach; vt: the plane's
// vertical table.  First and last taps never move backwards from one output row to the next.
M2V_SC_HD inline void tile_span(const Taps *vt, uint32_t y0, uint32_t h, uint32_t srows, int &rlo, int &rhi)
{
    const Taps &a = vt[row_of(y0, h)], &b = vt[row_of(y0 + kTileRows - 1u, h)];
    rlo = clampi(a.first, (int)srows - 1);
    rhi = clampi(b.first + (int)b.n - 1, (int)srows - 1);
}

// horizontal pass, one value: byte b of the elements of source row `row` under the taps t.  0 .. 16320
M2V_SC_HD inline uint32_t hpass(const uint8_t *row, uint32_t es, uint32_t b, const Taps &t, uint32_t scols)
{
    uint32_t acc = 128u;
    auto s = [&](uint32_t k) -> uint32_t { return row[(uint32_t)clampi(t.first + (int)k, (int)scols - 1) * es + b]; };
    for (uint32_t k = 0; k < t.n; k += 4u) {
        const uint32_t s0 = s(k), s1 = s(k + 1u), s2 = s(k + 2u), s3 = s(k + 3u);
        acc = mad24(t.c[k], s0, acc);
        acc = mad24(t.c[k + 1u], s1, acc);
        acc = mad24(t.c[k + 2u], s2, acc);
        acc = mad24(t.c[k + 3u], s3, acc);
    }
    return acc >> 8;
}

// vertical pass, one byte: tcol = the tile's horizontal results of this column, source row rlo first, `stride` values apart
M2V_SC_HD inline uint32_t vpass(const uint16_t *tcol, uint32_t stride, int rlo, const Taps &d, uint32_t srows)
{
    uint32_t acc = 1u << 19;
    // (a tap beyond n has coefficient 0 and reads the row of the last one: clamped to rhi's row at most, which the tile holds)
    const int last = d.first + (int)d.n - 1;
    auto v = [&](uint32_t k) -> uint32_t { const int j = d.first + (int)k; return tcol[(clampi(j < last ? j : last, (int)srows - 1) - rlo) * (int)stride]; };
    for (uint32_t k = 0; k < d.n; k += 4u) {
        const uint32_t v0 = v(k), v1 = v(k + 1u), v2 = v(k + 2u), v3 = v(k + 3u);
        acc = mad24(d.c[k], v0, acc);
        acc = mad24(d.c[k + 1u], v1, acc);
        acc = mad24(d.c[k + 2u], v2, acc);
        acc = mad24(d.c[k + 3u], v3, acc);
    }
    return acc >> 20;
}

}  // namespace scale
}  // namespace m2v
