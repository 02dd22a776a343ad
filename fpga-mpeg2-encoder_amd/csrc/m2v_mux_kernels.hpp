// m2v_mux_kernels.hpp — the arithmetic of the device muxer (m2v_mux.hip tells the whole story): every function that decides a byte of
// the transport or program stream, in __host__ __device__ inline form.  The kernels of m2v_mux.hip are thin loops over these functions,
// and the same header compiles with a plain C++ compiler (the qualifiers defined empty), so the whole algorithm - start-code scan,
// picture table, plan, "16 bytes at container position q" - can be run and checked on a CPU against m2v_container.cpp, which is the
// specification: the output is byte for byte what m2vc_mux_ts / m2vc_mux_ps return.
//
// The rate, pts0, PCR and SCR are double arithmetic in m2v_container.cpp.  They are repeated here operation by operation, in the same
// order, with contraction off (no fused multiply-add) and plain IEEE division, so the device reproduces them bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define M2V_HD __host__ __device__
#else
#define M2V_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace m2v {
namespace mux {

enum { kTs = 1, kPs = 2 };                                   // M2V_MUX_TS / M2V_MUX_PS
enum { kOk = 0, kSyntax = -2, kOverflow = -3, kEvents = -100 };   // kEvents: the event list was too small (m2v_mux_device runs again with a larger one)

constexpr uint32_t kScanTile = 16384;                        // bytes after which k_es_scan hands over to another block
constexpr uint64_t kNone = ~0ull;

// one picture of the plan: where its access unit starts in the elementary stream (picture 0: 0, the sequence headers travel with it),
// where its first byte lands in the container (TS: the PAT in front of it, if one is due), and for TS the PAT / PMT pairs before it
struct Pic { uint64_t es0, out0; uint32_t psi_before, has_psi; uint64_t reserved; };      // 32 bytes; entry [npics] ends the table

// one stream.  The host writes the first group when a call starts (zeros below it); k_es_scan fills the second through atomics; k_mux_plan
// the rest
struct Stream {
    uint64_t es_off, es_bytes;          // where the elementary stream is (the host's, or sampled from the encoder's records by k_mux_plan)
    uint32_t ev_base, ev_cap;           // its part of the event list (a power of two) ...
    uint32_t pic_base, kind;            // ... and of the picture table (ev_cap + 1 entries)
    // k_es_scan: maxima, so that zero is "none" (inv_* = ~position)
    uint64_t inv_first_end, inv_first_bad, inv_first_slice, last_nz;      // first B7, first picture header that is cut short or of a type other than I / P, first slice; one past the last byte != 0
    uint32_t ev_count, pad0;
    // k_mux_plan
    int32_t status; uint32_t npics;
    uint64_t n;                         // bytes up to and including sequence_end_code
    uint64_t out_off, out_bytes, unit0; // the container's place in the caller's buffer; the first of its 16-byte units among all streams'
    uint64_t pts0;
    double rate;
    uint32_t mux_rate50, vbuf_kb, fn, fd;
};

typedef uint64_t u64u __attribute__((aligned(1), may_alias));
M2V_HD inline uint64_t ld8(const uint8_t *p) { return *(const u64u *)p; }

// ---------------------------------------------------------------------------------------------------------------------------
// start-code scan: one call looks at the 16 positions p0 .. p0 + 15
// ---------------------------------------------------------------------------------------------------------------------------
// bit k = byte k of w is zero (exact: no borrow travels between bytes)
M2V_HD inline uint32_t zero_bytes(uint64_t w)
{
    const uint64_t m = 0x7F7F7F7F7F7F7F7Full;
    const uint64_t t = ~(((w & m) + m) | w | m);             // 0x80 in every zero byte
    return (uint32_t)((((t >> 7) * 0x0002040810204081ull) >> 49) & 0xFFu);
}

// bytes p0 .. p0 + 23 of a stream of n bytes as three little-endian words; bytes at or past n read 0xFF (no start code, not zero)
M2V_HD inline void load24(const uint8_t *es, uint64_t p0, uint64_t n, uint64_t &w0, uint64_t &w1, uint64_t &w2)
{
    if (p0 + 24 <= n) { w0 = ld8(es + p0); w1 = ld8(es + p0 + 8); w2 = ld8(es + p0 + 16); return; }
    w0 = w1 = w2 = ~0ull;
    for (uint32_t k = 0; k < 24 && p0 + k < n; ++k) {
        const uint64_t b = (uint64_t)(es[p0 + k] ^ 0xFFu) << (8 * (k & 7));
        if (k < 8) w0 ^= b; else if (k < 16) w1 ^= b; else w2 ^= b;
    }
}

M2V_HD inline uint32_t byte24(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t k)
{
    const uint64_t w = k < 8 ? w0 : k < 16 ? w1 : w2;
    return (uint32_t)(w >> (8 * (k & 7))) & 0xFFu;
}

struct ScanAcc { uint64_t inv_first_end = 0, inv_first_bad = 0, inv_first_slice = 0, last_nz = 0; };
M2V_HD inline uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// What scan() of m2v_container.cpp sees at p0 .. p0 + 15 (p0 < n): 00 00 01 xx with xx inside the stream.  The codes the picture table
// is made of - B3, B8, 00, B7 - go to emit as position << 8 | code; the first end code, the first bad picture header and the first slice
// and the last byte that is not zero go to the accumulator.  (The serial scan steps over a start code that begins at the code byte of a
// picture_start_code; that picture's coding type is then 0, a syntax error there and here.)
template <class Emit>
M2V_HD inline void scan16(uint64_t p0, uint64_t n, uint64_t w0, uint64_t w1, uint64_t w2, ScanAcc &a, Emit emit)
{
    const uint64_t ones = 0x0101010101010101ull;
    const uint32_t z = zero_bytes(w0) | zero_bytes(w1) << 8 | zero_bytes(w2) << 16;
    const uint32_t o = zero_bytes(w0 ^ ones) | zero_bytes(w1 ^ ones) << 8 | zero_bytes(w2 ^ ones) << 16;
    const uint32_t inside = n - p0 >= 16 ? 0xFFFFu : (1u << (uint32_t)(n - p0)) - 1u;
    const uint32_t nz = ~z & inside;
    if (nz) a.last_nz = max64(a.last_nz, p0 + 32u - (uint32_t)__builtin_clz(nz));
    uint32_t cand = z & (z >> 1) & (o >> 2) & 0xFFFFu;
    while (cand) {
        const uint32_t j = (uint32_t)__builtin_ctz(cand);
        cand &= cand - 1u;
        const uint64_t p = p0 + j;
        if (p + 3 >= n) break;
        const uint32_t code = byte24(w0, w1, w2, j + 3);
        if (code == 0x00) {
            const uint32_t type = (byte24(w0, w1, w2, j + 5) >> 3) & 7u;
            if (p + 6 > n || (type != 1 && type != 2)) a.inv_first_bad = max64(a.inv_first_bad, ~p);
        } else if (code <= 0xAF) {
            a.inv_first_slice = max64(a.inv_first_slice, ~p);
            continue;
        } else if (code == 0xB7) {
            a.inv_first_end = max64(a.inv_first_end, ~p);
        } else if (code != 0xB3 && code != 0xB8) {
            continue;
        }
        emit(p << 8 | code);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline void frame_rate(uint32_t code, uint32_t &num, uint32_t &den)
{
    num = code == 1 ? 24000u : code == 2 ? 24u : code == 3 ? 25u : code == 4 ? 30000u : code == 5 ? 30u : code == 6 ? 50u : code == 7 ? 60000u : code == 8 ? 60u : 0u;
    den = code == 1 || code == 4 || code == 7 ? 1001u : 1u;
}

// The picture table from the events in stream order: the state machine of scan() (a GOP header opens its picture's access unit, a
// repeated sequence header in front of it opens it earlier still).  ev = the stream's events sorted by position, nev of them.  Writes
// pics[i].es0 and returns the status; npics, n (the bytes up to and including the end code), maxpic as the CPU's scan leaves them.
// Access units that do not follow each other in the stream (a malformed order of headers) are a syntax error here.
M2V_HD inline int plan_pictures(const uint8_t *es, uint64_t es_bytes, const uint64_t *ev, uint32_t nev, uint32_t pic_cap, const Stream &S,
                                Pic *pics, uint32_t &npics, uint64_t &n, uint64_t &maxpic)
{
    npics = 0; n = es_bytes; maxpic = 0;
    if (es_bytes < 12 || es[0] != 0 || es[1] != 0 || es[2] != 1 || es[3] != 0xB3) return kSyntax;
    const uint64_t first_end = ~S.inv_first_end, first_bad = ~S.inv_first_bad, first_slice = ~S.inv_first_slice;
    if (first_bad < first_end) return kSyntax;
    uint64_t pending_start = kNone, back_off = 0, first_pic = kNone;
    bool gop_pending = false, seq_pending = false, open = false, has_end = false, ordered = true;
    for (uint32_t k = 0; k < nev; ++k) {
        const uint64_t p = ev[k] >> 8;
        const uint32_t code = (uint32_t)ev[k] & 0xFFu;
        if (code == 0xB3 && p == 0) continue;
        if (open) { maxpic = max64(maxpic, p - back_off); open = false; }
        if (code == 0xB3) { seq_pending = true; pending_start = p; }
        else if (code == 0xB8) { gop_pending = true; if (!seq_pending) pending_start = p; seq_pending = false; }
        else if (code == 0x00) {
            const uint64_t off = gop_pending ? pending_start : p;
            if (npics == 0) first_pic = p;
            else if (off <= back_off) ordered = false;
            if (npics < pic_cap) pics[npics].es0 = off;
            ++npics;
            back_off = off; open = true; gop_pending = false;
        } else {                                             // B7
            has_end = true;
            n = p + 4;
            break;
        }
    }
    if (open) maxpic = max64(maxpic, (has_end ? n - 4 : n) - back_off);
    if (first_slice < first_pic && first_slice < first_end) return kSyntax;      // a slice in front of the first picture
    if (has_end && S.last_nz > n) return kSyntax;                                 // only zero padding may follow
    if (!ordered || npics == 0 || npics > pic_cap) return kSyntax;
    uint32_t fn, fd;
    frame_rate(es[7] & 15u, fn, fd);
    if (!fn) return kSyntax;
    return kOk;
}

// video packets of a PES packet of 14 + b bytes: the first carries 176 of them behind the PCR, the others 184
M2V_HD inline uint64_t ts_packets(uint64_t b) { return 14 + b <= 176 ? 1 : 1 + (14 + b - 176 + 183) / 184; }
// packs of a picture of b bytes (the first one, first = the stream's first pack, also carries the system header), and their bytes
M2V_HD inline uint64_t ps_first_payload(bool first) { return first ? 2005 : 2020; }
M2V_HD inline uint64_t ps_packs(uint64_t b, bool first) { const uint64_t c = ps_first_payload(first); return b > c ? 1 + (b - c + 2024) / 2025 : 1; }

// Rate, pts0 and every picture's place (the picture table's es0 are in, npics / n / maxpic from plan_pictures).  TS: the PSI recurrence
// of m2vc_mux_ts - "now" depends on the insertions before it - is serial over the pictures: one division per picture.  Returns the
// container's bytes.
M2V_HD inline uint64_t plan_layout(Stream &S, Pic *pics, const uint8_t *es, uint64_t maxpic)
{
    const uint32_t np = S.npics;
    const uint64_t n = S.n;
    uint32_t fn, fd;
    frame_rate(es[7] & 15u, fn, fd);
    S.fn = fn; S.fd = fd;
    const double seconds = (double)np * fd / fn;
    const uint64_t period = 1ull * 90000ull * fd / fn;       // clk.pts(1, 0)
    pics[0].es0 = 0;                                         // the sequence headers travel with the first picture
    uint64_t v = 0;
    if (S.kind == kTs) {
        double rate = (double)n / seconds * 1.15;
        if (rate < 125000.0) rate = 125000.0;
        S.rate = rate; S.mux_rate50 = 0; S.vbuf_kb = 0;
        S.pts0 = (uint64_t)(2.0 * (double)maxpic / rate * 90000.0) + period + 900;
        double next_psi = 0.0;
        uint32_t psi = 0;
        for (uint32_t i = 0; i < np; ++i) {
            const double now = (double)v / rate;
            const bool has = now >= next_psi;
            if (has) next_psi = now + 0.1;
            pics[i].out0 = v; pics[i].psi_before = psi; pics[i].has_psi = has ? 1u : 0u; pics[i].reserved = 0;
            if (has) { v += 376; ++psi; }
            const uint64_t b = (i + 1 < np ? pics[i + 1].es0 : n) - pics[i].es0;
            v += 188 * ts_packets(b);
        }
        pics[np].es0 = n; pics[np].out0 = v; pics[np].psi_before = psi; pics[np].has_psi = 0; pics[np].reserved = 0;
        return v;
    }
    double bytes_per_s = (double)n / seconds * 1.10;
    if (bytes_per_s < 125000.0) bytes_per_s = 125000.0;
    const uint32_t mux_rate50 = (uint32_t)((bytes_per_s + 49.0) / 50.0);
    const double rate = mux_rate50 * 50.0;
    uint64_t vb = (2 * maxpic + 1023) / 1024 + 16;
    if (vb > 8191) vb = 8191;
    S.rate = rate; S.mux_rate50 = mux_rate50; S.vbuf_kb = (uint32_t)vb;
    S.pts0 = (uint64_t)(2.0 * (double)maxpic / rate * 90000.0) + period + 900;
    for (uint32_t i = 0; i < np; ++i) {
        pics[i].out0 = v; pics[i].psi_before = 0; pics[i].has_psi = 0; pics[i].reserved = 0;
        const uint64_t b = (i + 1 < np ? pics[i + 1].es0 : n) - pics[i].es0;
        v += b + 28 + (i == 0 ? 15 : 0) + 23 * (ps_packs(b, i == 0) - 1);
    }
    pics[np].es0 = n; pics[np].out0 = v; pics[np].psi_before = 0; pics[np].has_psi = 0; pics[np].reserved = 0;
    return v + 4;                                            // MPEG_program_end_code
}

// ---------------------------------------------------------------------------------------------------------------------------
// the bytes
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline uint64_t pts_of(const Stream &S, uint64_t i) { return S.pts0 + i * 90000ull * S.fd / S.fn; }

// byte h (0 .. 4) of a time stamp: prefix '0010', 3 + 15 + 15 bits, a marker behind each group
M2V_HD inline uint32_t stamp_byte(uint64_t t, uint32_t h)
{
    return h == 0 ? 0x21u | (uint32_t)((t >> 30) & 7u) << 1 : h == 1 ? (uint32_t)(t >> 22) & 0xFFu : h == 2 ? ((uint32_t)(t >> 15) & 0x7Fu) << 1 | 1u
         : h == 3 ? (uint32_t)(t >> 7) & 0xFFu : ((uint32_t)t & 0x7Fu) << 1 | 1u;
}

// PAT (which = 0) and PMT (1) packets: header, pointer_field, the section with its CRC (constants: nothing in them varies), 0xFF
M2V_HD inline uint32_t psi_byte(uint32_t which, uint32_t cc, uint32_t k)
{
    static constexpr uint8_t kPat[16] = {0x00, 0xB0, 0x0D, 0x00, 0x01, 0xC1, 0x00, 0x00, 0x00, 0x01, 0xF0, 0x00, 0x2A, 0xB1, 0x04, 0xB2};
    static constexpr uint8_t kPmt[21] = {0x02, 0xB0, 0x12, 0x00, 0x01, 0xC1, 0x00, 0x00, 0xE1, 0x00, 0xF0, 0x00, 0x02, 0xE1, 0x00, 0xF0, 0x00, 0x9E, 0x8B, 0x23, 0xD1};
    if (k < 5) return k == 0 ? 0x47u : k == 1 ? (which ? 0x50u : 0x40u) : k == 2 ? 0x00u : k == 3 ? 0x10u | (cc & 15u) : 0x00u;
    const uint32_t s = k - 5;
    if (which == 0) return s < 16 ? kPat[s] : 0xFFu;
    return s < 21 ? kPmt[s] : 0xFFu;
}

// the bytes in front of the payload of video packet (first = the PES packet's first, with PCR and PES header): k < 4 + af + (first ? 14 : 0)
M2V_HD inline uint32_t ts_head_byte(bool first, uint32_t af, uint32_t cc, uint64_t pcr27, uint64_t pts, uint32_t k)
{
    if (k < 4) return k == 0 ? 0x47u : k == 1 ? (first ? 0x41u : 0x01u) : k == 2 ? 0x00u : (af ? 0x30u : 0x10u) | (cc & 15u);
    if (k < 4 + af) {
        if (k == 4) return af == 1 ? 0u : af - 1;
        if (k == 5) return first ? 0x10u : 0x00u;
        if (first && k < 12) {
            const uint64_t base = (pcr27 / 300) & 0x1FFFFFFFFull, ext = pcr27 % 300;
            return k == 6 ? (uint32_t)(base >> 25) & 0xFFu : k == 7 ? (uint32_t)(base >> 17) & 0xFFu : k == 8 ? (uint32_t)(base >> 9) & 0xFFu
                 : k == 9 ? (uint32_t)(base >> 1) & 0xFFu : k == 10 ? (uint32_t)(((base & 1) << 7) | 0x7E | (ext >> 8)) & 0xFFu : (uint32_t)ext & 0xFFu;
        }
        return 0xFFu;
    }
    const uint32_t h = k - 4 - af;                           // PES header: PES_packet_length 0, data_alignment, PTS only
    return h < 2 ? 0x00u : h == 2 ? 0x01u : h == 3 ? 0xE0u : h < 6 ? 0x00u : h == 6 ? 0x85u : h == 7 ? 0x80u : h == 8 ? 0x05u : stamp_byte(pts, h - 9);
}

// the bytes in front of the payload of a pack: pack header, system header (sys), PES header with (pts) or without a time stamp
M2V_HD inline uint32_t ps_head_byte(const Stream &S, uint64_t scr27, bool sys, bool has_pts, uint64_t payload, uint64_t pts, uint32_t k)
{
    if (k < 14) {
        if (k < 4) return k == 2 ? 0x01u : k == 3 ? 0xBAu : 0x00u;
        if (k < 10) {
            const uint64_t base = (scr27 / 300) & 0x1FFFFFFFFull, ext = scr27 % 300;
            const uint64_t v = 1ull << 46 | ((base >> 30) & 7u) << 43 | 1ull << 42 | ((base >> 15) & 0x7FFFu) << 27 | 1ull << 26 | (base & 0x7FFFu) << 11 | 1ull << 10 | ext << 1 | 1ull;
            return (uint32_t)(v >> (8 * (9 - k))) & 0xFFu;
        }
        if (k < 13) return ((S.mux_rate50 & 0x3FFFFFu) << 2 | 3u) >> (8 * (12 - k)) & 0xFFu;
        return 0xF8u;
    }
    k -= 14;
    if (sys) {
        if (k < 15) {
            if (k < 6) return k == 2 ? 0x01u : k == 3 ? 0xBBu : k == 5 ? 0x09u : 0x00u;
            if (k < 9) return (1u << 23 | (S.mux_rate50 & 0x3FFFFFu) << 1 | 1u) >> (8 * (8 - k)) & 0xFFu;
            return k == 9 ? 0x00u : k == 10 ? 0x61u : k == 11 ? 0x7Fu : k == 12 ? 0xE0u : k == 13 ? 0xE0u | (S.vbuf_kb >> 8 & 0x1Fu) : S.vbuf_kb & 0xFFu;
        }
        k -= 15;
    }
    const uint32_t len = (uint32_t)(3 + (has_pts ? 5 : 0) + payload) & 0xFFFFu;
    return k < 2 ? 0x00u : k == 2 ? 0x01u : k == 3 ? 0xE0u : k == 4 ? len >> 8 : k == 5 ? len & 0xFFu : k == 6 ? (has_pts ? 0x85u : 0x81u)
         : k == 7 ? (has_pts ? 0x80u : 0x00u) : k == 8 ? (has_pts ? 5u : 0u) : stamp_byte(pts, k - 9);
}

// sixteen bytes under construction: byte k of the window is bits 8k .. of lo (k < 8) or hi
struct Win { uint64_t lo = 0, hi = 0; };
M2V_HD inline void win_put(Win &w, uint32_t at, uint32_t b)
{
    if (at < 8) w.lo |= (uint64_t)b << (8 * at); else w.hi |= (uint64_t)b << (8 * (at - 8));
}
// cnt (1 .. 16) bytes of the stream from es + pos to window position at (at + cnt <= 16); never reads at or past es + es_bytes
M2V_HD inline void win_copy(Win &w, uint32_t at, uint32_t cnt, const uint8_t *es, uint64_t pos, uint64_t es_bytes)
{
    uint64_t a, b;
    if (pos + 16 <= es_bytes) { a = ld8(es + pos); b = ld8(es + pos + 8); }
    else {
        a = b = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t v = (uint64_t)es[pos + k] << (8 * (k & 7));
            if (k < 8) a |= v; else b |= v;
        }
    }
    if (cnt < 8) { a &= (1ull << (8 * cnt)) - 1; b = 0; }
    else if (cnt < 16) b &= cnt == 8 ? 0ull : (1ull << (8 * (cnt - 8))) - 1;
    if (at == 0) { w.lo |= a; w.hi |= b; }
    else if (at < 8) { w.lo |= a << (8 * at); w.hi |= b << (8 * at) | a >> (64 - 8 * at); }
    else if (at == 8) w.hi |= a;
    else w.hi |= a << (8 * (at - 8));
}

// the last picture whose first byte is at or in front of container position q (q < out_bytes; entry [npics] is the end of the table)
M2V_HD inline uint32_t pic_at(const Pic *pics, uint32_t npics, uint64_t q)
{
    uint32_t lo = 0, hi = npics;                             // pics[lo].out0 <= q
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (pics[mid].out0 <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The bytes of the container at positions q0 .. q0 + 15, those inside [0, out_bytes) (the others are left zero): unit u of a stream
// whose output starts m bytes past a 16-byte boundary is gen16(.., 16 u - m).  es = the stream's first byte.
M2V_HD inline Win gen16(const Stream &S, const Pic *pics, const uint8_t *es, long long q0)
{
    Win w;
    const uint64_t qa = q0 < 0 ? 0ull : (uint64_t)q0;
    const uint64_t qb = (uint64_t)(q0 + 16) < S.out_bytes ? (uint64_t)(q0 + 16) : S.out_bytes;
    uint64_t q = qa;
    while (q < qb) {
        const uint32_t i = pic_at(pics, S.npics, q);
        const uint64_t out0 = pics[i].out0, es0 = pics[i].es0;
        uint32_t at = (uint32_t)((long long)q - q0);
        if (i == S.npics) {                                  // MPEG_program_end_code (a transport stream ends with its last packet)
            for (; q < qb; ++q, ++at) { const uint32_t k = (uint32_t)(q - out0); win_put(w, at, k == 2 ? 0x01u : k == 3 ? 0xB9u : 0x00u); }
            break;
        }
        const uint64_t b = pics[i + 1].es0 - es0;            // the picture's bytes
        uint64_t start, head, pay_es, pay;                   // this packet: where it starts, the bytes in front of its payload, the payload's place and bytes
        if (S.kind == kTs) {
            const uint64_t pes = out0 + (pics[i].has_psi ? 376u : 0u);
            if (q < pes) {                                   // PAT or PMT
                const uint32_t which = (uint32_t)((q - out0) / 188);
                const uint64_t end = out0 + 188ull * (which + 1) < qb ? out0 + 188ull * (which + 1) : qb;
                for (; q < end; ++q, ++at) win_put(w, at, psi_byte(which, pics[i].psi_before, (uint32_t)(q - out0) - 188u * which));
                continue;
            }
            const uint64_t pk = (q - pes) / 188;
            const bool first = pk == 0;
            const uint64_t before = first ? 0 : 176 + 184 * (pk - 1), left = 14 + b - before;       // PES bytes in earlier packets, and still to go
            uint32_t af = first ? 8u : 0u;
            if (184 - af > left) af = (uint32_t)(184 - left);  // stuffing so that the payload ends with the packet
            start = pes + 188 * pk;
            head = 4 + af + (first ? 14u : 0u);
            pay = 188 - head;
            pay_es = es0 + (first ? 0 : before - 14);
            if (q < start + head) {
                const uint64_t end = start + head < qb ? start + head : qb;
                const uint64_t pcr27 = first ? (uint64_t)((double)pes / S.rate * 27000000.0) : 0ull;
                const uint64_t pts = first ? pts_of(S, i) : 0ull;
                const uint32_t cc = (uint32_t)(out0 / 188 - 2ull * pics[i].psi_before + pk);
                for (; q < end; ++q, ++at) win_put(w, at, ts_head_byte(first, af, cc, pcr27, pts, (uint32_t)(q - start)));
                continue;
            }
        } else {
            const bool sys = i == 0;
            const uint64_t head0 = sys ? 43u : 28u;
            const uint64_t pay0 = b < 2048 - head0 ? b : 2048 - head0;
            bool has_pts = true;
            if (q < out0 + head0 + pay0) { start = out0; head = head0; pay = pay0; pay_es = es0; }
            else {
                const uint64_t j = (q - (out0 + head0 + pay0)) / 2048;
                start = out0 + head0 + pay0 + 2048 * j;
                head = 23;
                const uint64_t before = pay0 + 2025 * j;
                pay = b - before < 2025 ? b - before : 2025;
                pay_es = es0 + before;
                has_pts = false;
            }
            if (q < start + head) {
                const uint64_t end = start + head < qb ? start + head : qb;
                const uint64_t scr27 = (uint64_t)((double)start / S.rate * 27000000.0);
                const uint64_t pts = has_pts ? pts_of(S, i) : 0ull;
                for (; q < end; ++q, ++at) win_put(w, at, ps_head_byte(S, scr27, sys && has_pts, has_pts, pay, pts, (uint32_t)(q - start)));
                continue;
            }
        }
        const uint64_t pend = start + head + pay;
        const uint64_t end = pend < qb ? pend : qb;
        win_copy(w, at, (uint32_t)(end - q), es, pay_es + (q - start - head), S.es_bytes);
        q = end;
    }
    return w;
}

// What always suffices for a stream of es_bytes bytes and `pictures` pictures (include/m2v_mi355x.h states the derivation)
M2V_HD inline uint64_t bound(int kind, uint64_t es_bytes, uint64_t pictures)
{
    const uint64_t np = pictures ? pictures : 1;
    if (kind == kTs) return 188 * (es_bytes / 184 + 4 * np + 1);
    return es_bytes + 23 * (es_bytes / 2025) + 51 * np + 19;
}

}  // namespace mux
}  // namespace m2v
