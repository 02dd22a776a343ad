// m2v_deint_kernels.hpp — the arithmetic of the deinterlacer (m2v_deinterlace_device; include/m2v_mi355x.h has the definition,
// m2v_deint.hip the kernel and its launch): every function that decides a byte or an address, in __host__ __device__ inline form - the
// planes of a frame, the fields of a call and what stands in for an absent one, the rows beside an interpolated row, the three filters on
// samples packed four to a dword, and the walk down a strip of rows.  k_deint is a thin loop over these functions, and the same header
// compiles with a plain C++ compiler (the qualifiers defined empty), so the whole pass can be walked tile by tile on a CPU and held
// against the numpy statement of the definition (deinterlace_frames; tests/test_deint_cases.py).  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define M2V_DI_HD __host__ __device__
#else
#define M2V_DI_HD
#endif

namespace m2v {
namespace deint {

enum { kLine = 0, kAdaptive = 1, kBlend = 2 };      // M2V_DEINT_LINE / ADAPTIVE / BLEND
enum { kFrameRate = 0, kFieldRate = 1 };            // M2V_DEINT_FRAME_RATE / FIELD_RATE
enum { kTff = 0, kBff = 1 };                        // M2V_DEINT_TFF / BFF
constexpr int kMaxSize = 16384;                     // a frame's width and height
// a work item: kTileRows rows of kTileCols bytes of one plane of one frame, walked by kLanes lanes of kVec bytes each - a quarter of a
// wavefront, whose four items lie next to each other along the row where the plane is wide enough
constexpr int kVec = 16, kLanes = 16, kTileCols = kVec * kLanes, kTileRows = 8;
constexpr int kMaxBlocks = 2048, kBlock = 256, kItemsPerBlock = kBlock / kLanes;

M2V_DI_HD inline uint32_t chroma(uint32_t v) { return (v + 1u) / 2u; }

// One plane of a frame: `rows` rows of `rb` bytes at `off` in the frame; tiles: its work items, ctiles of them along a row.
struct Plane { uint32_t off, rb, rows, ctiles, tiles; };
struct Frame { Plane p[3]; uint32_t nplanes, tiles; uint64_t bytes; };

// the planes of a w x h frame of M2V_420_* layout `layout` (0 / 1: three planes, 2 / 3: luma and one plane of pairs).  Every plane is
// processed bytewise, so U and V never need telling apart.
M2V_DI_HD inline Frame make_frame(int layout, uint32_t w, uint32_t h)
{
    Frame f{};
    const uint32_t cw = chroma(w), ch = chroma(h);
    f.p[0] = Plane{0u, w, h, 0u, 0u};
    if (layout < 2) {
        f.p[1] = Plane{w * h, cw, ch, 0u, 0u};
        f.p[2] = Plane{w * h + cw * ch, cw, ch, 0u, 0u};
        f.nplanes = 3;
    } else {
        f.p[1] = Plane{w * h, 2u * cw, ch, 0u, 0u};
        f.nplanes = 2;
    }
    for (uint32_t k = 0; k < f.nplanes; ++k) {
        Plane &p = f.p[k];
        p.ctiles = (p.rb + kTileCols - 1u) / kTileCols;
        p.tiles = p.ctiles * ((p.rows + kTileRows - 1u) / kTileRows);
        f.tiles += p.tiles;
    }
    f.bytes = (uint64_t)w * h + 2ull * cw * ch;
    return f;
}

// work item `t` of a frame (0 .. f.tiles - 1) -> its plane, its first row and its first byte column: the planes one behind the other,
// in a plane the tiles of a strip of rows next to each other.  (Constant indices only: the planes stay in registers.)
M2V_DI_HD inline void tile_of(const Frame &f, uint32_t t, Plane &pl, uint32_t &y0, uint32_t &x0)
{
    pl = f.p[0];
    if (t >= pl.tiles) {
        t -= pl.tiles;
        pl = f.p[1];
        if (t >= pl.tiles) { t -= pl.tiles; pl = f.p[2]; }
    }
    const uint32_t s = t / pl.ctiles;
    y0 = s * kTileRows;
    x0 = (t - s * pl.ctiles) * kTileCols;
}

// The fields of a call: F[k], k = 0 .. nfields - 1 (nfields = 2 * nframes), lies in frame k >> 1 and has parity order ^ (k & 1).
M2V_DI_HD inline uint32_t field_parity(int64_t k, int order) { return (uint32_t)(order ^ (int)(k & 1)); }
// a field index outside the call -> the nearest field of the same parity inside it
M2V_DI_HD inline int64_t field_sub(int64_t k, int64_t nfields) { return k < 0 ? (k & 1) : k >= nfields ? nfields - 2 + (k & 1) : k; }
M2V_DI_HD inline uint64_t field_frame(int64_t k, int64_t nfields) { return (uint64_t)(field_sub(k, nfields) >> 1); }

// the rows beside an interpolated row y of a plane of H >= 2 rows: a row missing at the plane's edge is replaced by the one beside it
M2V_DI_HD inline uint32_t row_c(uint32_t y) { return y > 0u ? y - 1u : y + 1u; }
M2V_DI_HD inline uint32_t row_e(uint32_t y, uint32_t H) { return y + 1u < H ? y + 1u : y - 1u; }

// ---- the filters, on one sample ----
M2V_DI_HD inline uint32_t absd(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
M2V_DI_HD inline uint32_t sp1(uint32_t c, uint32_t e) { return (c + e + 1u) >> 1; }
M2V_DI_HD inline uint32_t blend1(uint32_t up, uint32_t s, uint32_t dn) { return (up + 2u * s + dn + 2u) >> 2; }
// c, e: the rows beside the sample in its own frame; b, a: the sample's row in the frames of F[k - 1] and F[k + 1]; cp, ep / cn, en: the
// rows beside it in the frames of F[k - 2] / F[k + 2]
M2V_DI_HD inline uint32_t adaptive1(uint32_t c, uint32_t e, uint32_t b, uint32_t a, uint32_t cp, uint32_t ep, uint32_t cn, uint32_t en)
{
    const int sp = (int)sp1(c, e), d = (int)((b + a) >> 1);
    const uint32_t t0 = absd(b, a) >> 1, t1 = (absd(cp, c) + absd(ep, e)) >> 1, t2 = (absd(cn, c) + absd(en, e)) >> 1;
    const int m = (int)(t0 > t1 ? (t0 > t2 ? t0 : t2) : (t1 > t2 ? t1 : t2));
    const int lo = d - m, hi = d + m;
    return (uint32_t)(sp < lo ? lo : sp > hi ? hi : sp);
}

// ---- the same on four samples in a dword.  The rounded means need no unpacking; the absolute differences do. ----
M2V_DI_HD inline uint32_t sp4(uint32_t c, uint32_t e) { return (c | e) - (((c ^ e) >> 1) & 0x7F7F7F7Fu); }           // (c + e + 1) >> 1
M2V_DI_HD inline uint32_t floor4(uint32_t b, uint32_t a) { return (b & a) + (((b ^ a) >> 1) & 0x7F7F7F7Fu); }       // (b + a) >> 1
// (up + 2 s + dn + 2) >> 2 = (((up + dn) >> 1) + s + 1) >> 1: the bit the inner shift drops never reaches the result
M2V_DI_HD inline uint32_t blend4(uint32_t up, uint32_t s, uint32_t dn) { return sp4(floor4(up, dn), s); }
M2V_DI_HD inline uint32_t adaptive4(uint32_t c, uint32_t e, uint32_t b, uint32_t a, uint32_t cp, uint32_t ep, uint32_t cn, uint32_t en)
{
    // where neither the other field nor the rows beside the sample move at all, the clamp has no width: the other field is woven in
    if (b == a && cp == c && ep == e && cn == c && en == e) return a;
    uint32_t o = 0;
    for (uint32_t s = 0; s < 32u; s += 8u)
        o |= adaptive1((c >> s) & 255u, (e >> s) & 255u, (b >> s) & 255u, (a >> s) & 255u, (cp >> s) & 255u, (ep >> s) & 255u, (cn >> s) & 255u,
                       (en >> s) & 255u) << s;
    return o;
}

// kVec bytes of a row, as a lane carries them
struct Vec { uint32_t d[kVec / 4]; };
// a row of the walk: the lane's bytes of that row in the frame itself (C) and in the frames before (P) and behind it (N)
struct Rows { Vec C, P, N; };

M2V_DI_HD inline Vec sp_v(const Vec &c, const Vec &e) { Vec o; for (int i = 0; i < kVec / 4; ++i) o.d[i] = sp4(c.d[i], e.d[i]); return o; }
M2V_DI_HD inline Vec blend_v(const Vec &u, const Vec &s, const Vec &d) { Vec o; for (int i = 0; i < kVec / 4; ++i) o.d[i] = blend4(u.d[i], s.d[i], d.d[i]); return o; }
M2V_DI_HD inline Vec adaptive_v(const Vec &c, const Vec &e, const Vec &b, const Vec &a, const Vec &cp, const Vec &ep, const Vec &cn, const Vec &en)
{
    Vec o;
    for (int i = 0; i < kVec / 4; ++i) o.d[i] = adaptive4(c.d[i], e.d[i], b.d[i], a.d[i], cp.d[i], ep.d[i], cn.d[i], en.d[i]);
    return o;
}

// The frames a walk over frame f reads besides f itself.  Output field 2f takes b and c' / e' from the frame of F[2f - 1] and F[2f - 2]
// and c'' / e'' from that of F[2f + 2], output field 2f + 1 takes a and c'' / e'' from the frame of F[2f + 2] and F[2f + 3] and c' / e'
// from that of F[2f - 1]: after the substitution both pairs lie in ONE frame each (fP, fN).
M2V_DI_HD inline void walk_frames(uint64_t f, uint64_t nframes, uint64_t &fP, uint64_t &fN)
{
    const int64_t nf = 2 * (int64_t)nframes, k = 2 * (int64_t)f;
    fP = field_frame(k - 1, nf);        // == field_frame(k - 2, nf)
    fN = field_frame(k + 2, nf);        // == field_frame(k + 3, nf)
}

// which of a row's three vectors the walk over rows y0 .. y1 - 1 needs: bit 0 C, bit 1 P, bit 2 N.  `inside`: y is a row of the strip
// (the rows beside the strip serve as c / e only).  p: the parity of the frame's first field.
template <int MODE, int RATE>
M2V_DI_HD inline uint32_t row_needs(uint32_t y, uint32_t p, bool inside)
{
    if (MODE == kBlend) return 1u;
    const bool kept0 = (y & 1u) == p;                       // a kept row of output field 2f, a source of c / e for it
    if (MODE == kLine) return RATE == kFieldRate || kept0 ? 1u : 0u;
    if (RATE == kFieldRate) return 7u;
    return kept0 ? 7u : inside ? 3u : 0u;                   // the other field's rows: a (C) and b (P) of the row itself
}

// The walk of one lane down rows y0 .. y1 - 1 of a plane of H rows of frame f: io.load(which, y) returns the lane's bytes of row y in frame
// f (which = 0), fP (1) or fN (2); io.store(out, y, v) writes them to row y of output `out` of the frame (0: field 2f or the only one;
// 1: field 2f + 1).  The rows y - 1, y, y + 1 are carried, so no byte of a frame is loaded twice in a strip, and at field rate both
// outputs come from the same loads.
template <int MODE, int RATE, class IO>
M2V_DI_HD inline void walk(IO &io, uint32_t H, uint32_t y0, uint32_t y1, uint32_t p)
{
    auto fetch = [&](uint32_t y, bool inside) {
        Rows r{};
        const uint32_t n = row_needs<MODE, RATE>(y, p, inside);
        if (n & 1u) r.C = io.load(0, y);
        if (n & 2u) r.P = io.load(1, y);
        if (n & 4u) r.N = io.load(2, y);
        return r;
    };
    if (H < 2u) {                                           // a plane with a single row is copied to every output
        for (uint32_t y = y0; y < y1; ++y) {
            const Vec v = io.load(0, y);
            io.store(0, y, v);
            if (RATE == kFieldRate) io.store(1, y, v);
        }
        return;
    }
    // (the loads of row y + 2 are issued before row y is computed: a row's latency is hidden behind the row in front of it)
    Rows m{}, s = fetch(y0, true), n{}, nn{};
    if (y0 > 0u) m = fetch(y0 - 1u, false);
    if (y0 + 1u < H) n = fetch(y0 + 1u, y0 + 1u < y1);
    for (uint32_t y = y0; y < y1; ++y) {
        if (y + 2u < H && y + 1u < y1) nn = fetch(y + 2u, y + 2u < y1);
        if (MODE == kBlend) {
            io.store(0, y, blend_v(y > 0u ? m.C : s.C, s.C, y + 1u < H ? n.C : s.C));
        } else {
            const Rows &c = row_c(y) < y ? m : n, &e = row_e(y, H) > y ? n : m;
            if ((y & 1u) == p) io.store(0, y, s.C);
            else if (MODE == kLine) io.store(0, y, sp_v(c.C, e.C));
            else io.store(0, y, adaptive_v(c.C, e.C, s.P, s.C, c.P, e.P, c.N, e.N));
            if (RATE == kFieldRate) {
                if ((y & 1u) != p) io.store(1, y, s.C);
                else if (MODE == kLine) io.store(1, y, sp_v(c.C, e.C));
                else io.store(1, y, adaptive_v(c.C, e.C, s.C, s.N, c.P, e.P, c.N, e.N));
            }
        }
        m = s;
        s = n;
        n = nn;
    }
}

// where output `out` of frame f lies among a call's output frames
M2V_DI_HD inline uint64_t out_frame(uint64_t f, int rate, uint32_t out) { return rate == kFieldRate ? 2u * f + out : f; }

// bytes a call writes; 0 for arguments outside the definition (or a size no 64-bit count holds)
M2V_DI_HD inline uint64_t bound(int w, int h, uint64_t nframes, int rate)
{
    if (w < 1 || h < 2 || w > kMaxSize || h > kMaxSize || (rate != kFrameRate && rate != kFieldRate)) return 0;
    const uint64_t fb = make_frame(0, (uint32_t)w, (uint32_t)h).bytes;
    if (nframes > (1ull << 62) / fb) return 0;
    return nframes * fb * (rate == kFieldRate ? 2u : 1u);
}

// What the entry answers for its arguments before it looks at the handle's state: kOk, kParam (M2V_E_PARAM) or kOverflow
// (M2V_E_OVERFLOW), and in *why the reason.  src / dst: the two addresses as integers.
enum { kOk = 0, kParam = -1, kOverflow = -6 };
M2V_DI_HD inline int check_args(uint64_t src, uint64_t nframes, int w, int h, int layout, int mode, int rate, int order, uint64_t dst, uint64_t cap,
                                const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (layout < 0 || layout > 3) { *why = "unknown layout"; return kParam; }
    if (mode != kLine && mode != kAdaptive && mode != kBlend) { *why = "unknown mode"; return kParam; }
    if (rate != kFrameRate && rate != kFieldRate) { *why = "unknown rate"; return kParam; }
    if (order != kTff && order != kBff) { *why = "unknown order"; return kParam; }
    if (mode == kBlend && rate == kFieldRate) { *why = "M2V_DEINT_BLEND knows no fields, so it has no field rate"; return kParam; }
    if (w < 1 || h < 2 || w > kMaxSize || h > kMaxSize) { *why = "the size is no frame of two fields (1 ... 16384 by 2 ... 16384)"; return kParam; }
    const uint64_t need = bound(w, h, nframes, rate);
    if (nframes && !need) { *why = "more frames than a 64-bit count of bytes holds"; return kParam; }
    if (nframes && (!src || !dst)) { *why = "a pointer is NULL"; return kParam; }
    const uint64_t in = need / (rate == kFieldRate ? 2u : 1u);
    if (nframes && src < dst + need && dst < src + in) { *why = "the source and the destination overlap (the pass reads neighbouring frames: it cannot work in place)"; return kParam; }
    if (cap < need) { *why = "cap is below m2v_deinterlace_bound"; return kOverflow; }
    *why = "";
    return kOk;
}

}  // namespace deint
}  // namespace m2v
