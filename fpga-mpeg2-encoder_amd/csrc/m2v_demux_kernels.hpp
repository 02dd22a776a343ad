// m2v_demux_kernels.hpp — the arithmetic of the device demultiplexer (m2v_demux.hip tells the whole story): every function that decides a
// byte, an offset or a verdict, in __host__ __device__ inline form.  The kernels of m2v_demux.hip are thin loops and reductions over
// these functions, and the header compiles with a plain C++ compiler, so the whole algorithm - packet classes, PSI, tile sums, the plan,
// the program stream's chain, "16 bytes at stream position q" - runs on a CPU against m2vc_demux_ts / m2vc_demux_ps of m2v_container.cpp,
// which are the specification (include/m2v_container.h states every rule; it is not repeated here).
#pragma once
#include "m2v_mux_kernels.hpp"      // Win, win_copy, ld8

namespace m2v {
namespace demux {

enum { kTs = 1, kPs = 2 };                                            // M2V_MUX_TS / M2V_MUX_PS
enum { kOk = 0, kSyntax = -2, kOverflow = -3, kNoStream = -4 };       // M2V_DEMUX_*

constexpr uint32_t kTilePackets = 1024;                               // transport packets a block of k_ts_tiles / k_demux_table takes at a time
constexpr uint32_t kScanTile = 188 * kTilePackets;
constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kNoPid = ~0u;                                      // matches no packet

// one run of elementary bytes: where it is in the container (<< 16 | the bytes of the PES header in front of it, 0: no PES packet starts
// here) and where it goes in the stream.  Its length is the next entry's `out` minus its own; entry [nseg] ends the table
struct Seg { uint64_t src_hl, out; };

// 1024 transport packets
struct Tile {
    uint32_t bytes, bytes_pre;          // elementary bytes of the video packets; those in front of the tile's first PES start
    uint32_t video, video_pre;          // video packets; ...
    uint32_t pes, disc;                 // PES starts; continuity breaks between two packets of this tile
    uint32_t first, last;               // the first packet with a payload: index in the tile << 8 | discontinuity_indicator << 4 | counter (~0: none); the last one's counter
    uint64_t first_pusi;                // packet index of the first PES start (kNone: none)
    uint64_t out0;                      // ts_plan: elementary bytes in front of this tile
    uint32_t pes0, pad;                 // ts_plan: PES starts in front of it
};

// one container.  The host writes the first group when a call starts; k_ts_find / k_ps_walk and k_ts_tiles the second; k_demux_plan the rest
struct State {
    uint64_t src_off, src_bytes;
    uint64_t seg_base, seg_cap;
    uint32_t tile_base, ntiles;
    int32_t want; uint32_t kind;        // the caller's `stream` (-1: find it)
    uint64_t err;                       // a minimum over packets / units (kNone: no rule broken)
    uint32_t pid; int32_t found;        // TS: the video PID and discovery's verdict; PS: the stream_id and the chain's verdict
    int32_t status; uint32_t pes, packets, disc, skipped, pad;
    uint64_t nseg, first_pusi, out_bytes, out_off, unit0, stamp0;
};

struct Stamp { uint64_t es_offset, pts, dts, src_offset; };

// ---------------------------------------------------------------------------------------------------------------------------
// PES header
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline uint64_t stamp33(const uint8_t *b)
{
    return (uint64_t)((b[0] >> 1) & 7u) << 30 | (uint64_t)b[1] << 22 | (uint64_t)(b[2] >> 1) << 15 | (uint64_t)b[3] << 7 | (uint64_t)(b[4] >> 1);
}

// the PES header at h, of which `avail` bytes may be looked at: false = it breaks a rule; head = 9 + PES_header_data_length
M2V_HD inline bool pes_check(const uint8_t *h, uint64_t avail, uint32_t &head)
{
    head = 0;
    if (avail < 9 || h[0] != 0 || h[1] != 0 || h[2] != 1 || h[3] < 0xE0 || h[3] > 0xEF) return false;
    if ((h[6] & 0xC0) != 0x80 || (h[6] & 0x30) != 0) return false;
    const uint32_t hl = h[8], flags = h[7] >> 6;
    if (9 + hl > avail || flags == 1) return false;
    if (flags >= 2 && (hl < (flags == 3 ? 10u : 5u) || (uint32_t)(h[9] >> 4) != flags || !(h[9] & 1) || !(h[11] & 1) || !(h[13] & 1))) return false;
    if (flags == 3 && ((h[14] >> 4) != 1 || !(h[14] & 1) || !(h[16] & 1) || !(h[18] & 1))) return false;
    head = 9 + hl;
    return true;
}

// the stamps of a header pes_check has accepted
M2V_HD inline void pes_stamps(const uint8_t *h, uint64_t &pts, uint64_t &dts)
{
    const uint32_t flags = h[7] >> 6;
    pts = flags >= 2 ? stamp33(h + 9) : kNone;
    dts = flags == 3 ? stamp33(h + 14) : kNone;
}

// ---------------------------------------------------------------------------------------------------------------------------
// transport stream: one packet
// ---------------------------------------------------------------------------------------------------------------------------
enum { kBadSync = 1, kVideo = 2, kPusi = 4, kPayload = 8, kDi = 16, kViol = 32 };      // Pkt::flags; the counter in bits 8 .. 11

struct Pkt { uint32_t at, len, head, flags; };      // elementary bytes: p[at .. at + len); head: the PES header's bytes in front of them

M2V_HD inline uint32_t ts_pid(const uint8_t *p) { return (uint32_t)(p[1] & 0x1F) << 8 | p[2]; }

M2V_HD inline Pkt classify(const uint8_t *p, uint32_t pid)
{
    Pkt k{188, 0, 0, p[0] != 0x47 ? (uint32_t)kBadSync : 0u};
    if ((p[1] & 0x80) || ts_pid(p) != pid) return k;
    k.flags |= kVideo;
    const uint32_t afc = p[3] >> 4 & 3;
    uint32_t at = 4;
    bool ok = !(p[3] >> 6) && afc != 0;
    if (ok && afc == 2) { ok = p[4] == 183; at = 188; }
    if (ok && afc == 3) { ok = p[4] <= 182; at = 5 + p[4]; }
    const bool pusi = p[1] & 0x40;
    uint32_t head = 0;
    if (ok && pusi) ok = pes_check(p + at, 188 - at, head);
    if (!ok) { k.flags |= kViol; return k; }
    if (afc & 1) {
        k.flags |= kPayload | (uint32_t)(p[3] & 15) << 8;
        if (afc == 3 && p[4] > 0 && (p[5] & 0x80)) k.flags |= kDi;
    }
    if (pusi) k.flags |= kPusi;
    k.head = head; k.at = at + head; k.len = 188 - at - head;
    return k;
}

// the word a tile keeps of its first packet with a payload, and what the packet behind a counter `last` must not be
M2V_HD inline uint32_t cc_word(uint32_t index, const Pkt &k) { return index << 8 | (k.flags & kDi ? 16u : 0u) | (k.flags >> 8 & 15u); }
M2V_HD inline bool cc_breaks(uint32_t last_cc, uint32_t word) { return (word & 15u) != ((last_cc + 1) & 15u) && !(word & 16u); }

// ---------------------------------------------------------------------------------------------------------------------------
// transport stream: PAT and PMT
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline uint32_t crc32_mpeg(const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) {
        c ^= (uint32_t)p[i] << 24;
        for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
    }
    return c;
}

// a packet of `pid` that starts a section and has a payload
M2V_HD inline bool psi_match(const uint8_t *p, uint32_t pid) { return !(p[1] & 0x80) && (p[1] & 0x40) && (p[3] & 0x10) && ts_pid(p) == pid; }

// the section of such a packet: pointer_field, table_id, section_syntax_indicator, wholly inside the packet, CRC 0; len = 3 + section_length
M2V_HD inline bool psi_section(const uint8_t *p, uint32_t table_id, uint32_t min_length, uint32_t &sec, uint32_t &len)
{
    uint32_t at = 4;
    if ((p[3] >> 4 & 3) == 3) {
        if (p[4] > 182) return false;
        at = 5 + p[4];
    }
    at += 1 + p[at];
    if (at + 3 > 188) return false;
    sec = at;
    const uint32_t sl = (uint32_t)(p[at + 1] & 15) << 8 | p[at + 2];
    len = 3 + sl;
    if (p[at] != table_id || !(p[at + 1] & 0x80) || sl < min_length || at + len > 188) return false;
    return crc32_mpeg(p + at, len) == 0;
}

// the PAT packet p: kOk with the first program and its PMT PID, kNoStream, or kSyntax
M2V_HD inline int pat_parse(const uint8_t *p, uint32_t &program, uint32_t &pmt)
{
    uint32_t at, len;
    program = pmt = 0;
    if (!psi_section(p, 0, 9, at, len)) return kSyntax;
    const uint8_t *s = p + at;
    for (uint32_t i = 8; i + 4 <= len - 4 && !program; i += 4) {
        program = (uint32_t)s[i] << 8 | s[i + 1];
        pmt = (uint32_t)(s[i + 2] & 0x1F) << 8 | s[i + 3];
    }
    return program ? kOk : kNoStream;
}

M2V_HD inline int pmt_parse(const uint8_t *p, uint32_t program, uint32_t &video)
{
    uint32_t at, len;
    if (!psi_section(p, 2, 13, at, len)) return kSyntax;
    const uint8_t *s = p + at;
    if (((uint32_t)s[3] << 8 | s[4]) != program) return kSyntax;
    uint32_t i = 12 + ((uint32_t)(s[10] & 15) << 8 | s[11]);
    if (i > len - 4) return kSyntax;
    for (; i + 5 <= len - 4; i += 5 + ((uint32_t)(s[i + 3] & 15) << 8 | s[i + 4]))
        if (s[i] == 1 || s[i] == 2) { video = (uint32_t)(s[i + 1] & 0x1F) << 8 | s[i + 2]; return kOk; }
    return kNoStream;
}

// what the length of a transport stream breaks (a minimum like every other)
M2V_HD inline uint64_t ts_length_err(uint64_t n) { return n == 0 || n % 188 ? 188 * (n / 188) : kNone; }

// ---------------------------------------------------------------------------------------------------------------------------
// transport stream: the plan over the tiles (serial: a few additions per 1024 packets)
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline void tile_clear(Tile &T) { T = Tile{}; T.first = ~0u; T.first_pusi = kNone; }

// one packet into a tile's sums, serially (the kernel reduces the same quantities over its lanes); `index` in the tile, `packet` in the container
M2V_HD inline void tile_add(Tile &T, const Pkt &k, uint32_t index, uint64_t packet, uint32_t &last_cc_state)
{
    if (!(k.flags & kVideo)) return;
    ++T.video;
    T.bytes += k.len;
    if (k.flags & kPusi) { ++T.pes; if (T.first_pusi == kNone) T.first_pusi = packet; }
    if (T.first_pusi == kNone) { ++T.video_pre; T.bytes_pre += k.len; }
    if (k.flags & kPayload) {
        const uint32_t w = cc_word(index, k);
        if (T.first == ~0u) T.first = w;
        else if (cc_breaks(last_cc_state, w)) ++T.disc;
        last_cc_state = T.last = w & 15u;
    }
}

// the verdict of a transport stream and every tile's place, from the tiles' sums; S.err holds the minimum over all packets
M2V_HD inline void ts_plan(State &S, Tile *tiles)
{
    S.pes = S.packets = S.disc = S.skipped = 0;
    S.first_pusi = kNone; S.out_bytes = 0; S.nseg = 0;
    if (S.found != kOk) { S.status = S.found == kSyntax || S.err != kNone ? (int)kSyntax : (int)kNoStream; return; }
    uint64_t out = 0;
    int last = -1;
    for (uint32_t t = 0; t < S.ntiles; ++t) {
        Tile &T = tiles[t];
        T.out0 = out; T.pes0 = S.pes;
        S.packets += T.video; S.disc += T.disc;
        if (T.first != ~0u) {
            if (last >= 0 && cc_breaks((uint32_t)last, T.first)) ++S.disc;
            last = (int)T.last;
        }
        if (S.first_pusi != kNone) out += T.bytes;
        else if (T.first_pusi == kNone) S.skipped += T.video;
        else { S.first_pusi = T.first_pusi; S.skipped += T.video_pre; out += T.bytes - T.bytes_pre; }
        S.pes += T.pes;
    }
    S.out_bytes = out;
    S.nseg = S.src_bytes / 188;
    S.status = S.err != kNone ? (int)kSyntax : S.pes == 0 ? (int)kNoStream : (int)kOk;
}

// the table entry of packet `packet` (elementary bytes in front of it: out): nothing of a packet in front of the first PES start
M2V_HD inline Seg ts_seg(const Pkt &k, uint64_t packet, uint64_t out) { return Seg{(188 * packet + k.at) << 16 | k.head, out}; }
M2V_HD inline uint32_t ts_len(const Pkt &k, uint64_t packet, uint64_t first_pusi) { return (k.flags & kVideo) && packet >= first_pusi ? k.len : 0u; }

// ---------------------------------------------------------------------------------------------------------------------------
// program stream: the chain (serial by definition: one lane per container)
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline void ps_walk(State &S, const uint8_t *src, Seg *segs)
{
    const uint64_t n = S.src_bytes;
    int sel = S.want;
    uint64_t p = 0, out = 0, nseg = 0;
    uint32_t packs = 0, skipped = 0;
    S.err = kNone; S.found = kOk;
    while (p < n) {
        if (n - p < 4 || src[p] != 0 || src[p + 1] != 0 || src[p + 2] != 1) { S.err = p; break; }
        const uint32_t c = src[p + 3];
        if (c == 0xB9) {
            for (uint64_t q = p + 4; q < n; ++q)
                if (src[q]) { S.err = q; break; }
            break;
        }
        if (c == 0xBA) {
            const uint8_t *h = src + p + 4;
            if (n - p < 14 || (h[0] >> 6) != 1 || !(h[0] & 4) || !(h[2] & 4) || !(h[4] & 4) || !(h[5] & 1) || (h[8] & 3) != 3 || n - p < 14u + (h[9] & 7)) { S.err = p; break; }
            ++packs;
            p += 14u + (h[9] & 7);
            continue;
        }
        if ((c != 0xBB && c < 0xBC) || n - p < 6) { S.err = p; break; }
        const uint64_t L = (uint64_t)src[p + 4] << 8 | src[p + 5];
        if (n - p - 6 < L) { S.err = p; break; }
        if (sel < 0 && c >= 0xE0 && c <= 0xEF) sel = (int)c;
        if ((int)c == sel) {
            uint32_t head;
            if (!pes_check(src + p, 6 + L, head)) { S.err = p; break; }
            if (nseg < S.seg_cap) segs[nseg] = Seg{(p + head) << 16 | head, out};
            ++nseg;
            out += 6 + L - head;
        } else {
            ++skipped;
        }
        p += 6 + L;
    }
    if (nseg < S.seg_cap) segs[nseg] = Seg{0, out};
    S.pid = sel < 0 ? 0u : (uint32_t)sel;
    S.pes = (uint32_t)nseg; S.packets = packs; S.skipped = skipped; S.disc = 0;
    S.nseg = nseg; S.out_bytes = out; S.first_pusi = 0;
    S.status = S.found = S.err != kNone ? (int)kSyntax : nseg == 0 ? (int)kNoStream : (int)kOk;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the streams' places, and the bytes
// ---------------------------------------------------------------------------------------------------------------------------
struct Place { uint64_t end = 0, units = 0, stamps = 0; };

// container S behind those before it: on a 32-byte boundary of the buffer, judged against cap; a refused one takes no room and no stamps
M2V_HD inline void place(State &S, Place &P, uint64_t cap, uint64_t dst_addr)
{
    const uint64_t o = (P.end + 31ull) & ~31ull;
    if (S.status == kOk && (o > cap || S.out_bytes > cap - o)) S.status = kOverflow;
    if (S.status != kOk) { S.out_bytes = 0; S.pes = S.packets = S.disc = S.skipped = 0; S.pid = 0; S.nseg = 0; }
    if (S.status != kSyntax) S.err = 0;
    S.out_off = o; S.unit0 = P.units; S.stamp0 = P.stamps;
    if (S.out_bytes) { P.units += (S.out_bytes + ((dst_addr + o) & 15ull) + 15ull) >> 4; P.end = o + S.out_bytes; }
    P.stamps += S.pes;
}

// the stamp of the PES packet that starts at table entry g
M2V_HD inline Stamp stamp_of(const Seg &g, const uint8_t *src)
{
    const uint64_t hdr = (g.src_hl >> 16) - (g.src_hl & 0xFFFFu);
    Stamp s{g.out, 0, 0, hdr};
    pes_stamps(src + hdr, s.pts, s.dts);
    return s;
}

// the last entry that starts at or in front of stream position q (q < out_bytes: it is the one that holds q, empty entries share their successor's start)
M2V_HD inline uint64_t seg_at(const Seg *segs, uint64_t nseg, uint64_t q)
{
    uint64_t lo = 0, hi = nseg;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].out <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The bytes of the stream at positions q0 .. q0 + 15, those inside [0, out_bytes) (the others are left zero).  src = the container's first
// byte, n its length: nothing at or past src + n is read.
M2V_HD inline mux::Win gather16(const Seg *segs, uint64_t nseg, uint64_t out_bytes, const uint8_t *src, uint64_t n, long long q0)
{
    mux::Win w;
    uint64_t q = q0 < 0 ? 0ull : (uint64_t)q0;
    const uint64_t qb = (uint64_t)(q0 + 16) < out_bytes ? (uint64_t)(q0 + 16) : out_bytes;
    if (q >= qb) return w;
    uint64_t i = seg_at(segs, nseg, q);
    while (q < qb) {
        const uint64_t next = segs[i + 1].out;
        if (next > q) {
            const uint64_t end = next < qb ? next : qb;
            mux::win_copy(w, (uint32_t)((long long)q - q0), (uint32_t)(end - q), src, (segs[i].src_hl >> 16) + (q - segs[i].out), n);
            q = end;
        }
        ++i;
    }
    return w;
}

}  // namespace demux
}  // namespace m2v
