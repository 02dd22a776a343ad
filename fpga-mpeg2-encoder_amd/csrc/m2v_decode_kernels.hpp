// m2v_decode_kernels.hpp — the arithmetic of the device decoder (m2v_decode.hip tells the whole story): every function that decides a
// bit or a sample, in __host__ __device__ inline form - bit reader, start-code scan, header parsers, the five VLC tables, the macroblock
// layer, the dequantisers, both Chen-Wang variants, half-pel prediction, and where an output byte comes from.  The kernels of
// m2v_decode.hip are thin loops over these functions, and the same header compiles with a plain C++ compiler (tools/dec_host.hpp runs
// the whole decoder serially on a CPU), so everything can be checked against decoder.py, which is the specification: a stream is
// refused exactly when decoder.decode raises (or holds a start-code prefix it did not read), and the frames are its frames.
//
// The VLC tables are the Annex B tables of decoder.py in look-up form: a code is found by its run of leading zeros (the DC size tables:
// leading ones) and the few bits behind the first one; kXxxZ[z] = offset << 3 | bits, kXxxTab the entries, 0xFFFF = no such code.
#pragma once
#include "m2v_mux_kernels.hpp"

namespace m2v {
namespace dec {

enum { kIso = 0, kModule = 1 };                                   // M2V_DEC_ISO / M2V_DEC_MODULE
enum { kOk = 0, kSyntax = -2, kOverflow = -3, kEvents = -100 };   // kEvents: the event list was too small (the call runs again with the count)

constexpr uint32_t kScanTile = 4096;                              // bytes after which the scan hands over to another block
constexpr uint64_t kNone = ~0ull;
constexpr int kMaxSize = 2048;                                    // pictures up to 2048 x 2048

M2V_HD inline uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------------------
// bit reader: [pos, end) in bits; end is where the next start code begins (or the stream ends).  Bits at or past end read zero, and
// consuming one sets err: no unit is ever read beyond itself
// ---------------------------------------------------------------------------------------------------------------------------
struct Bits { const uint8_t *d; uint64_t pos, end; uint32_t err; };

M2V_HD inline uint64_t be64(const uint8_t *d, uint64_t byte, uint64_t endbyte)
{
    if (byte + 8 <= endbyte) return __builtin_bswap64(mux::ld8(d + byte));
    uint64_t w = 0;
    for (uint32_t k = 0; k < 8; ++k) w = w << 8 | (byte + k < endbyte ? (uint64_t)d[byte + k] : 0ull);
    return w;
}

// the next n bits (1 .. 32), not consumed
M2V_HD inline uint32_t peek(const Bits &b, int n)
{
    const uint64_t w = be64(b.d, b.pos >> 3, b.end >> 3) << (b.pos & 7u);
    return (uint32_t)(w >> (64 - n));
}

M2V_HD inline void skip(Bits &b, int n)
{
    b.pos += (uint32_t)n;
    if (b.pos > b.end) { b.pos = b.end; b.err = 1; }
}

M2V_HD inline uint32_t get(Bits &b, int n)
{
    const uint32_t v = peek(b, n);
    skip(b, n);
    return v;
}

// everything from pos to end is zero (the stuffing in front of the next start code)
M2V_HD inline bool tail_zero(Bits b)
{
    if ((b.pos & 7u) && get(b, 8 - (int)(b.pos & 7u))) return false;     // (end is a whole byte: the rest of this one lies in front of it)
    for (uint64_t k = b.pos >> 3, e = b.end >> 3; k < e; k += 8) if (be64(b.d, k, e)) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// start-code scan: bit j of the answer = 00 00 01 xx begins at p0 + j with xx inside the stream (j = 0 .. 15).  w0 .. w2 = load24
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline uint32_t scan16(uint64_t p0, uint64_t n, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t &last_nz)
{
    const uint64_t ones = 0x0101010101010101ull;
    const uint32_t z = mux::zero_bytes(w0) | mux::zero_bytes(w1) << 8 | mux::zero_bytes(w2) << 16;
    const uint32_t o = mux::zero_bytes(w0 ^ ones) | mux::zero_bytes(w1 ^ ones) << 8 | mux::zero_bytes(w2 ^ ones) << 16;
    const uint32_t inside = n - p0 >= 16 ? 0xFFFFu : (1u << (uint32_t)(n - p0)) - 1u;
    const uint32_t nz = ~z & inside;
    if (nz) last_nz = mux::max64(last_nz, p0 + 32u - (uint32_t)__builtin_clz(nz));     // one past the last byte that is not zero
    uint32_t cand = z & (z >> 1) & (o >> 2) & 0xFFFFu;
    if (n - p0 < 19) {                                       // the code byte of position j is p0 + j + 3 < n
        const uint32_t room = n - p0 > 3 ? (uint32_t)(n - p0) - 3u : 0u;
        cand &= (1u << room) - 1u;
    }
    return cand;
}

// an event: position << 8 | code
M2V_HD inline uint64_t ev_pos(uint64_t e) { return e >> 8; }
M2V_HD inline uint32_t ev_code(uint64_t e) { return (uint32_t)e & 0xFFu; }

// ---------------------------------------------------------------------------------------------------------------------------
// VLC tables
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline uint32_t vlc_find(uint32_t w, const uint16_t *tab, const uint16_t *zd, int nz, bool ones)
{
    if (ones) w = ~w;
    int z = w ? __builtin_clz(w) : 32;
    if (z > nz - 1) z = nz - 1;
    const uint32_t d = zd[z];
    if (d == 0xFFFFu) return 0xFFFFu;
    const uint32_t r = d & 7u;
    const uint32_t idx = r ? (w << (z + 1)) >> (32u - r) : 0u;
    return tab[(d >> 3) + idx];
}

// w = the next 32 bits.  Each answers length | symbol << 8, or 0 where no code of the table begins w
M2V_HD inline uint32_t vlc_motion(uint32_t w)                // Table B-10: symbol = |motion_code| (the sign bit follows)
{
    static constexpr uint16_t kMotionTab[32] = {
        0x0000, 0x0011, 0x0022, 0x0033, 0x0066, 0x0056, 0x0045, 0x0045, 0x00C9, 0x00B9, 0x00A8, 0x00A8, 0x0098, 0x0098, 0x0088, 0x0088, 0x0076,
        0x0076, 0x0076, 0x0076, 0x0076, 0x0076, 0x0076, 0x0076, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0x0109, 0x00F9, 0x00E9, 0x00D9
    };
    static constexpr uint16_t kMotionZ[8] = {
        0x0000, 0x0008, 0x0010, 0x0018, 0x0022, 0x0044, 0x00C3, 0xFFFF
    };
    const uint32_t e = vlc_find(w, kMotionTab, kMotionZ, 8, false);
    return e == 0xFFFFu ? 0u : ((e & 15u) + 1u) | (e >> 4) << 8;
}

M2V_HD inline uint32_t vlc_cbp(uint32_t w)                   // Table B-9 (4:2:0: cbp 0 has no code)
{
    static constexpr uint16_t kCbpTab[74] = {
        0x0284, 0x0144, 0x0304, 0x00C4, 0x0203, 0x0203, 0x0103, 0x0103, 0x0083, 0x0083, 0x0043, 0x0043, 0x03C2, 0x03C2, 0x03C2, 0x03C2, 0x03E4,
        0x0024, 0x03D4, 0x0014, 0x0384, 0x0344, 0x02C4, 0x01C4, 0x0226, 0x0126, 0x00A6, 0x0066, 0x0216, 0x0116, 0x0096, 0x0056, 0x03F5, 0x03F5,
        0x0035, 0x0035, 0x0245, 0x0245, 0x0185, 0x0185, 0x02B7, 0x0177, 0x0337, 0x00F7, 0x02A7, 0x0167, 0x0327, 0x00E7, 0x0297, 0x0157, 0x0317,
        0x00D7, 0x0237, 0x0137, 0x00B7, 0x0077, 0x0397, 0x0357, 0x02D7, 0x01D7, 0x0267, 0x01A7, 0x0257, 0x0197, 0x03A7, 0x0367, 0x02E7, 0x01E7,
        0x03B8, 0x0378, 0x02F8, 0x01F8, 0x0278, 0x01B8
    };
    static constexpr uint16_t kCbpZ[9] = {
        0x0004, 0x0083, 0x00C4, 0x0144, 0x01C3, 0x0202, 0x0222, 0x0241, 0xFFFF
    };
    const uint32_t e = vlc_find(w, kCbpTab, kCbpZ, 9, false);
    return e == 0xFFFFu ? 0u : ((e & 15u) + 1u) | (e >> 4) << 8;
}

M2V_HD inline uint32_t vlc_dc_luma(uint32_t w)               // Table B-12: symbol = dct_dc_size
{
    static constexpr uint16_t kDcYTab[12] = {
        0x0021, 0x0011, 0x0032, 0x0002, 0x0042, 0x0053, 0x0064, 0x0075, 0x0086, 0x0097, 0x00A8, 0x00B8
    };
    static constexpr uint16_t kDcYZ[10] = {
        0x0001, 0x0011, 0x0020, 0x0028, 0x0030, 0x0038, 0x0040, 0x0048, 0x0050, 0x0058
    };
    const uint32_t e = vlc_find(w, kDcYTab, kDcYZ, 10, true);
    return e == 0xFFFFu ? 0u : ((e & 15u) + 1u) | (e >> 4) << 8;
}

M2V_HD inline uint32_t vlc_dc_chroma(uint32_t w)             // Table B-13
{
    static constexpr uint16_t kDcCTab[12] = {
        0x0011, 0x0001, 0x0021, 0x0032, 0x0043, 0x0054, 0x0065, 0x0076, 0x0087, 0x0098, 0x00A9, 0x00B9
    };
    static constexpr uint16_t kDcCZ[11] = {
        0x0001, 0x0010, 0x0018, 0x0020, 0x0028, 0x0030, 0x0038, 0x0040, 0x0048, 0x0050, 0x0058
    };
    const uint32_t e = vlc_find(w, kDcCTab, kDcCZ, 11, true);
    return e == 0xFFFFu ? 0u : ((e & 15u) + 1u) | (e >> 4) << 8;
}

// Table B-14 without the sign bit: length | run << 8 | level << 16; level 0: run 0 = end of block, run 1 = escape.  '11' is run 0
// level 1 (the first-coefficient form '1s' is the block loop's)
M2V_HD inline uint32_t vlc_ac(uint32_t w)
{
    static constexpr uint16_t kAcTab[135] = {
        0x0001, 0x0201, 0x0403, 0x0223, 0x0212, 0x0212, 0x02D7, 0x0C07, 0x02C7, 0x02B7, 0x0437, 0x0617, 0x0A07, 0x02A7, 0x0604, 0x0604, 0x0604,
        0x0604, 0x0604, 0x0604, 0x0604, 0x0604, 0x0244, 0x0244, 0x0244, 0x0244, 0x0244, 0x0244, 0x0244, 0x0244, 0x0234, 0x0234, 0x0234, 0x0234,
        0x0234, 0x0234, 0x0234, 0x0234, 0x0275, 0x0265, 0x0415, 0x0255, 0x0426, 0x0296, 0x0806, 0x0286, 0x0015, 0x0309, 0x0459, 0x0E09, 0x0629,
        0x0819, 0x02F9, 0x02E9, 0x0449, 0x160B, 0x048B, 0x064B, 0x140B, 0x082B, 0x047B, 0x035B, 0x034B, 0x120B, 0x033B, 0x032B, 0x0A1B, 0x063B,
        0x100B, 0x046B, 0x031B, 0x04AC, 0x049C, 0x065C, 0x083C, 0x0A2C, 0x0E1C, 0x0C1C, 0x1E0C, 0x1C0C, 0x1A0C, 0x180C, 0x03AC, 0x039C, 0x038C,
        0x037C, 0x036C, 0x3E0D, 0x3C0D, 0x3A0D, 0x380D, 0x360D, 0x340D, 0x320D, 0x300D, 0x2E0D, 0x2C0D, 0x2A0D, 0x280D, 0x260D, 0x240D, 0x220D,
        0x200D, 0x500E, 0x4E0E, 0x4C0E, 0x4A0E, 0x480E, 0x460E, 0x440E, 0x420E, 0x400E, 0x1C1E, 0x1A1E, 0x181E, 0x161E, 0x141E, 0x121E, 0x101E,
        0x241F, 0x221F, 0x201F, 0x1E1F, 0x066F, 0x050F, 0x04FF, 0x04EF, 0x04DF, 0x04CF, 0x04BF, 0x03FF, 0x03EF, 0x03DF, 0x03CF, 0x03BF
    };
    static constexpr uint16_t kAcZ[13] = {
        0x0001, 0x0012, 0x0035, 0x0132, 0x0152, 0x0170, 0x017B, 0x01BC, 0x023C, 0x02BC, 0x033C, 0x03BC, 0xFFFF
    };
    const uint32_t e = vlc_find(w, kAcTab, kAcZ, 13, false);
    return e == 0xFFFFu ? 0u : ((e & 15u) + 1u) | ((e >> 4) & 31u) << 8 | (e >> 9) << 16;
}

M2V_HD inline uint32_t scan_to_raster(uint32_t k)            // figure 7-2: zig-zag position -> raster index
{
    static constexpr uint8_t kScan[64] = {
        0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50,
        43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
    };
    return kScan[k & 63u];
}

M2V_HD inline int32_t intra_weight(uint32_t i)               // 6.3.11: the default intra matrix, raster
{
    static constexpr uint8_t kIntraW[64] = {
        8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40, 22, 26, 27, 29,
        32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83
    };
    return kIntraW[i & 63u];
}

// ---------------------------------------------------------------------------------------------------------------------------
// headers: each parser takes the unit [start, end) in bytes, start at its 00 00 01 xx, and answers whether decoder.py accepts it -
// the fields it checks, and nothing but zero stuffing behind them
// ---------------------------------------------------------------------------------------------------------------------------
struct SeqHdr {
    uint32_t width, height, aspect, frame_rate_code, bit_rate, vbv, constrained, profile_level, progressive, chroma_format, low_delay,
             video_format, colour, display_w, display_h;      // colour: 0xFFFFFFFF = no colour_description, else the three codes
};

M2V_HD inline bool seq_equal(const SeqHdr &a, const SeqHdr &b)
{
    return a.width == b.width && a.height == b.height && a.aspect == b.aspect && a.frame_rate_code == b.frame_rate_code && a.bit_rate == b.bit_rate &&
           a.vbv == b.vbv && a.constrained == b.constrained && a.profile_level == b.profile_level && a.progressive == b.progressive &&
           a.chroma_format == b.chroma_format && a.low_delay == b.low_delay && a.video_format == b.video_format && a.colour == b.colour &&
           a.display_w == b.display_w && a.display_h == b.display_h;
}

M2V_HD inline Bits unit_bits(const uint8_t *es, uint64_t start, uint64_t end) { return Bits{es, 8 * start + 32, 8 * end, 0}; }

M2V_HD inline bool parse_sequence_header(const uint8_t *es, uint64_t start, uint64_t end, SeqHdr &h)
{
    Bits b = unit_bits(es, start, end);
    h.width = get(b, 12); h.height = get(b, 12); h.aspect = get(b, 4); h.frame_rate_code = get(b, 4); h.bit_rate = get(b, 18);
    bool ok = get(b, 1) == 1;
    h.vbv = get(b, 10); h.constrained = get(b, 1);
    ok = ok && get(b, 1) == 0;                               // load_intra_quantiser_matrix
    ok = ok && get(b, 1) == 0;                               // load_non_intra_quantiser_matrix
    return ok && !b.err && tail_zero(b);
}

M2V_HD inline bool parse_sequence_extension(const uint8_t *es, uint64_t start, uint64_t end, SeqHdr &h)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 1;
    h.profile_level = get(b, 8); h.progressive = get(b, 1); h.chroma_format = get(b, 2);
    ok = ok && get(b, 2) == 0;
    ok = ok && get(b, 2) == 0;                               // horizontal / vertical size extension
    h.bit_rate |= get(b, 12) << 18;
    ok = ok && get(b, 1) == 1;
    h.vbv |= get(b, 8) << 10;
    h.low_delay = get(b, 1);
    skip(b, 7);
    ok = ok && h.chroma_format == 1 && h.aspect >= 1 && h.aspect <= 4 && h.frame_rate_code >= 1 && h.frame_rate_code <= 8 && h.bit_rate != 0;
    return ok && !b.err && tail_zero(b);
}

M2V_HD inline bool parse_display_extension(const uint8_t *es, uint64_t start, uint64_t end, SeqHdr &h)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 2;
    h.video_format = get(b, 3);
    h.colour = 0xFFFFFFFFu;
    if (get(b, 1)) {
        h.colour = get(b, 24);
        ok = ok && (h.colour >> 16) != 0 && ((h.colour >> 8) & 255u) != 0 && (h.colour & 255u) != 0;
    }
    h.display_w = get(b, 14);
    ok = ok && get(b, 1) == 1;
    h.display_h = get(b, 14);
    return ok && !b.err && tail_zero(b);
}

M2V_HD inline bool parse_gop_header(const uint8_t *es, uint64_t start, uint64_t end)
{
    Bits b = unit_bits(es, start, end);
    skip(b, 12);                                             // drop_frame_flag, hours, minutes
    const bool ok = get(b, 1) == 1;
    skip(b, 14);                                             // seconds, pictures, closed_gop, broken_link
    return ok && !b.err && tail_zero(b);
}

M2V_HD inline bool parse_picture_header(const uint8_t *es, uint64_t start, uint64_t end, uint32_t &type)
{
    Bits b = unit_bits(es, start, end);
    skip(b, 10);
    type = get(b, 3);
    skip(b, 16);
    bool ok = type == 1 || type == 2;
    if (type == 2) { ok = ok && get(b, 1) == 0; skip(b, 3); }     // full_pel_forward_vector, forward_f_code
    ok = ok && get(b, 1) == 0;                               // extra_bit_picture
    return ok && !b.err && tail_zero(b);
}

M2V_HD inline bool parse_picture_coding_extension(const uint8_t *es, uint64_t start, uint64_t end)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    ok = ok && get(b, 4) == 1;
    ok = ok && get(b, 4) == 1;                               // f_code[0][0], [0][1]
    skip(b, 8);                                              // the backward ones
    ok = ok && get(b, 2) == 2;                               // intra_dc_precision: 10 bits
    ok = ok && get(b, 2) == 3;                               // frame picture
    skip(b, 1);                                              // top_field_first
    ok = ok && get(b, 1) == 1;                               // frame_pred_frame_dct
    ok = ok && get(b, 1) == 0;                               // concealment_motion_vectors
    ok = ok && get(b, 1) == 0;                               // q_scale_type
    ok = ok && get(b, 1) == 0;                               // intra_vlc_format
    ok = ok && get(b, 1) == 0;                               // alternate_scan
    skip(b, 4);                                              // repeat_first_field, chroma_420_type, progressive_frame, composite_display_flag
    return ok && !b.err && tail_zero(b);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the plan: the grammar of decoder.decode over the ordered start codes.  Every rule looks at an event and the three in front of it,
// so the events are judged independently; what a rule needs of the sequence header (mbh, the first header's fields) comes from event 0
// ---------------------------------------------------------------------------------------------------------------------------
enum { rBad = 0, rSeq, rSeqExt, rDisp, rGop, rPic, rPicExt, rSlice, rEnd };

M2V_HD inline int ev_role(const uint64_t *ev, uint32_t i)
{
    const uint32_t c = ev_code(ev[i]);
    if (c == 0xB3) return rSeq;
    if (c == 0xB8) return rGop;
    if (c == 0xB7) return rEnd;
    if (c == 0x00) return rPic;
    if (c <= 0xAF) return rSlice;
    if (c != 0xB5 || i == 0) return rBad;
    const uint32_t p = ev_code(ev[i - 1]);
    if (p == 0xB3) return rSeqExt;
    if (p == 0x00) return rPicExt;
    if (p == 0xB5 && i >= 2 && ev_code(ev[i - 2]) == 0xB3) return rDisp;
    return rBad;
}

// the three units of a sequence header at events i .. i + 2: kNone, or the start of the first unit that is wrong
M2V_HD inline uint64_t plan_sequence(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, SeqHdr &h)
{
    const uint64_t p0 = ev_pos(ev[i]);
    if (i + 2 >= nev || ev_code(ev[i]) != 0xB3) return p0;
    const uint64_t p1 = ev_pos(ev[i + 1]), p2 = ev_pos(ev[i + 2]), p3 = i + 3 < nev ? ev_pos(ev[i + 3]) : n;
    if (!parse_sequence_header(es, p0, p1, h)) return p0;
    if (ev_code(ev[i + 1]) != 0xB5 || !parse_sequence_extension(es, p1, p2, h)) return p1;
    if (ev_code(ev[i + 2]) != 0xB5 || !parse_display_extension(es, p2, p3, h)) return p2;
    return kNone;
}

struct Plan { SeqHdr seq; uint32_t mbw, mbh; };

// event 0 and what lies in front of it: kNone and the plan, or the error's offset
M2V_HD inline uint64_t plan_first(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, Plan &P)
{
    if (!nev) return 0;
    for (uint64_t k = 0, p0 = ev_pos(ev[0]); k < p0; k += 8) if (be64(es, k, p0)) return 0;      // (a stream of this encoder starts with the code)
    const uint64_t bad = plan_sequence(es, n, ev, nev, 0, P.seq);
    if (bad != kNone) return bad;
    if (!P.seq.width || !P.seq.height || P.seq.width > (uint32_t)kMaxSize || P.seq.height > (uint32_t)kMaxSize) return ev_pos(ev[0]);
    P.mbw = (P.seq.width + 15u) / 16u; P.mbh = (P.seq.height + 15u) / 16u;
    return kNone;
}

struct EvInfo { uint64_t bad; uint32_t pic, type, gop, rep; };      // bad: kNone, or the offset this event's rule reports

M2V_HD inline EvInfo plan_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const Plan &P, uint64_t last_nz)
{
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    const int role = ev_role(ev, i);
    if (role == rBad) { r.bad = pos; return r; }
    // what may stand in front of it
    const int prev = i ? ev_role(ev, i - 1) : rBad;
    const bool after_first = prev == rDisp && i == 3, after_repeat = prev == rDisp && i > 3;
    const bool after_picture = prev == rSlice && ev_code(ev[i - (i ? 1 : 0)]) == P.mbh;
    const bool top = after_first || after_picture;
    bool ok = true;
    switch (role) {
    case rSeq:
        if (i) {
            SeqHdr h;
            ok = top;
            const uint64_t bad = plan_sequence(es, n, ev, nev, i, h);
            if (bad != kNone) { r.bad = bad; return r; }
            ok = ok && seq_equal(h, P.seq);
            r.rep = 1;
        }
        break;
    case rSeqExt: case rDisp: break;                           // (judged with their sequence header)
    case rGop: ok = (top || after_repeat) && parse_gop_header(es, pos, end); r.gop = 1; break;
    case rPic: ok = (top || prev == rGop) && parse_picture_header(es, pos, end, r.type); r.pic = 1; break;
    case rPicExt: ok = parse_picture_coding_extension(es, pos, end); break;
    case rSlice: {
        const uint32_t c = ev_code(ev[i]);
        ok = c <= P.mbh && (c == 1 ? prev == rPicExt : prev == rSlice && ev_code(ev[i - 1]) == c - 1);
        break;
    }
    default:                                                   // rEnd: the last code, zeros behind it, the length a multiple of 32
        ok = top && i + 1 == nev && last_nz <= pos + 4 && (n & 31u) == 0;
        break;
    }
    if (i + 1 == nev && role != rEnd) ok = false;              // sequence_end_code is missing
    if (!ok) r.bad = pos;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// macroblock layer
// ---------------------------------------------------------------------------------------------------------------------------
struct MbRec { uint8_t intra, mc, cbp, qcode; int8_t mvx, mvy; uint8_t reserved[10]; };      // 16 bytes
struct SliceState { int32_t dc_pred[3]; int32_t pmv[2]; };

M2V_HD inline int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }

// 7.6.3.1 for f_code 1: the new vector component from its prediction and the decoded delta
M2V_HD inline int32_t vector_wrap(int32_t pmv, int32_t delta)
{
    int32_t v = pmv + delta;
    if (v < -16) v += 32; else if (v > 15) v -= 32;
    return v;
}

// 7.6.3.7: the chroma vector - /2 toward zero, or the module's floor
M2V_HD inline int32_t chroma_vector(int32_t mv, int mode) { return mode == kModule ? mv >> 1 : mv / 2; }

// an n x n block at (x0, y0) of a plane of pw x ph moved by (mvx, mvy) half samples reads inside the plane
M2V_HD inline bool block_inside(int x0, int y0, int mvx, int mvy, int n, int pw, int ph)
{
    const int ix = mvx >> 1, iy = mvy >> 1, hx = mvx & 1, hy = mvy & 1;
    return x0 + ix >= 0 && y0 + iy >= 0 && x0 + ix + n - 1 + hx < pw && y0 + iy + n - 1 + hy < ph;
}

M2V_HD inline bool vector_inside(int col, int row, int mvx, int mvy, int mbw, int mbh, int mode)
{
    return block_inside(16 * col, 16 * row, mvx, mvy, 16, 16 * mbw, 16 * mbh) &&
           block_inside(8 * col, 8 * row, chroma_vector(mvx, mode), chroma_vector(mvy, mode), 8, 8 * mbw, 8 * mbh);
}

// one coded block: the levels through put(raster index, level) - an intra block's DC goes to dc instead -; false = refused
template <class Put>
M2V_HD inline bool parse_block(Bits &b, bool intra, int comp, SliceState &s, int32_t &dc, Put put)
{
    uint32_t k = 0;
    if (intra) {
        const uint32_t e = comp ? vlc_dc_chroma(peek(b, 32)) : vlc_dc_luma(peek(b, 32));
        if (!e) return false;
        skip(b, (int)(e & 255u));
        const int size = (int)(e >> 8);
        int32_t diff = 0;
        if (size) {
            const int32_t d = (int32_t)get(b, size);
            diff = (d >> (size - 1)) ? d : d - (1 << size) + 1;
        }
        s.dc_pred[comp] = wrap_add(s.dc_pred[comp], diff);
        dc = s.dc_pred[comp];
        k = 1;
    }
    bool first = !intra;
    for (;;) {                                               // at most 64 coefficients: k grows with every one
        if (b.err) return false;
        const uint32_t w = peek(b, 32);
        uint32_t run = 0;
        int32_t lvl = 1;
        if (first && (w >> 31)) {                            // '1s': run 0, level +-1 as the first coefficient
            skip(b, 1);
            if (get(b, 1)) lvl = -1;
        } else {
            const uint32_t e = vlc_ac(w);
            if (!e) return false;
            skip(b, (int)(e & 255u));
            run = (e >> 8) & 255u;
            lvl = (int32_t)(e >> 16);
            if (!lvl) {
                if (!run) break;                             // end of block
                run = get(b, 6);                             // escape
                lvl = (int32_t)get(b, 12);
                if (lvl & 0x800) lvl -= 4096;
                if (lvl == 0 || lvl == -2048) return false;
            } else if (get(b, 1)) {
                lvl = -lvl;
            }
        }
        first = false;
        k += run;
        if (k >= 64 || b.err) return false;
        put(scan_to_raster(k), lvl);
        ++k;
    }
    return !b.err;
}

// one macroblock of a picture of type ptype (1 = I, 2 = P): its record, the DC of its intra blocks, its levels through
// put(block, raster index, level); false = refused
template <class Put>
M2V_HD inline bool parse_macroblock(Bits &b, uint32_t ptype, SliceState &s, MbRec &m, int32_t (&dc)[6], Put put)
{
    if (get(b, 1) != 1) return false;                        // macroblock_address_increment 1: nothing is skipped
    bool intra = false, mc = false, pattern = false;
    if (ptype == 1) {
        if (get(b, 1) != 1) return false;
        intra = true;
    } else if (get(b, 1)) {
        mc = pattern = true;                                 // '1'     MC, coded
    } else if (get(b, 1)) {
        return false;                                        // '01'    No-MC coded: never emitted
    } else if (get(b, 1)) {
        mc = true;                                           // '001'   MC, not coded
    } else {
        if (get(b, 2) != 3) return false;                    // '00011' intra
        intra = true;
    }
    int32_t mv[2] = {0, 0};
    if (mc) {
        for (int t = 0; t < 2; ++t) {
            const uint32_t e = vlc_motion(peek(b, 32));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            int32_t code = (int32_t)(e >> 8);
            if (code && get(b, 1)) code = -code;
            s.pmv[t] = mv[t] = vector_wrap(s.pmv[t], code);
        }
    } else {
        s.pmv[0] = s.pmv[1] = 0;                             // 7.6.3.4
    }
    uint32_t cbp = intra ? 63u : 0u;
    if (pattern) {
        const uint32_t e = vlc_cbp(peek(b, 32));
        if (!e) return false;
        skip(b, (int)(e & 255u));
        cbp = e >> 8;
    }
    if (!intra) s.dc_pred[0] = s.dc_pred[1] = s.dc_pred[2] = 0;     // 7.2.1
    m = MbRec{};
    m.intra = intra; m.mc = mc; m.cbp = (uint8_t)cbp; m.mvx = (int8_t)mv[0]; m.mvy = (int8_t)mv[1];
    for (int blk = 0; blk < 6; ++blk) {
        dc[blk] = 0;
        if (!((cbp >> (5 - blk)) & 1u)) continue;
        if (!parse_block(b, intra, blk < 4 ? 0 : blk - 3, s, dc[blk], [&](uint32_t i, int32_t l) { put(blk, i, l); })) return false;
    }
    return !b.err;
}

// the slice of macroblock row `row` in the unit [start, end): mbw macroblocks through sink.mb(col, record, dc) and
// sink.level(col, block, raster index, level), then nothing but zero stuffing; false = refused
template <class Sink>
M2V_HD inline bool parse_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, int mbw, int mbh, int row, int mode, Sink &sink)
{
    Bits b = unit_bits(es, start, end);
    const uint32_t qcode = get(b, 5);
    if (get(b, 1) != 0) return false;                        // extra_bit_slice
    SliceState s{{0, 0, 0}, {0, 0}};
    for (int col = 0; col < mbw; ++col) {
        MbRec m;
        int32_t dc[6];
        if (!parse_macroblock(b, ptype, s, m, dc, [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); })) return false;
        if (m.mc && !vector_inside(col, row, m.mvx, m.mvy, mbw, mbh, mode)) return false;
        m.qcode = (uint8_t)qcode;
        sink.mb(col, m, dc);
    }
    return !b.err && tail_zero(b);
}

// ---------------------------------------------------------------------------------------------------------------------------
// reconstruction
// ---------------------------------------------------------------------------------------------------------------------------
// 7.4.2: coefficient i (raster) of level q, saturated; the intra DC and mismatch control are the caller's (dequant_dc, mismatch)
M2V_HD inline int32_t dequant(int32_t q, uint32_t i, bool intra, int32_t qscale, int mode)
{
    int32_t v;
    if (intra) {
        v = 2 * q * intra_weight(i) * qscale;
        v = mode == kModule ? v >> 5 : v / 32;                // the module floors, ISO truncates toward zero
    } else {
        v = (2 * q + (q > 0 ? 1 : q < 0 ? -1 : 0)) * 16 * qscale / 32;
    }
    const int32_t lo = mode == kModule ? -2047 : -2048;
    return v < lo ? lo : v > 2047 ? 2047 : v;
}

// the intra DC: times 2 for 10-bit precision (the 1024 offset is the prediction's 128); the module does not saturate it
M2V_HD inline int32_t dequant_dc(int32_t dc, int mode)
{
    const int32_t v = (int32_t)((uint32_t)dc << 1);
    if (mode == kModule) return v;
    return v < -2048 ? -2048 : v > 2047 ? 2047 : v;
}

// 7.4.4: coefficient 63 once the sum of all 64 is known to be even (ISO only)
M2V_HD inline int32_t mismatch(int32_t f63) { return f63 + ((f63 & 1) ? -1 : 1); }

// Chen-Wang in 32-bit arithmetic, eight values in place: a row (11-bit scaling, >> 8; the module keeps 18 bits) or a column
// (>> 14, clipped to -256 .. 255; the module to -255 .. 255)
M2V_HD inline void idct_1d(int32_t (&a)[8], bool row, int mode)
{
    typedef uint32_t U;
    const U W1 = 2841, W2 = 2676, W3 = 2408, W5 = 1609, W6 = 1108, W7 = 565;
    const int sh = row ? 0 : 3;
    const U r = row ? 0u : 4u;
    auto sr = [](U v, int s) { return (U)((int32_t)v >> s); };
    U x0, x1, x2 = (U)a[6], x3 = (U)a[2], x4 = (U)a[1], x5 = (U)a[7], x6 = (U)a[5], x7 = (U)a[3], x8;
    if (row) { x0 = ((U)a[0] << 11) + 128u; x1 = (U)a[4] << 11; }
    else { x0 = ((U)a[0] << 8) + 8192u; x1 = (U)a[4] << 8; }
    x8 = W7 * (x4 + x5) + r;
    x4 = sr(x8 + (W1 - W7) * x4, sh);
    x5 = sr(x8 - (W1 + W7) * x5, sh);
    x8 = W3 * (x6 + x7) + r;
    x6 = sr(x8 - (W3 - W5) * x6, sh);
    x7 = sr(x8 - (W3 + W5) * x7, sh);
    x8 = x0 + x1;
    x0 = x0 - x1;
    x1 = W6 * (x3 + x2) + r;
    x2 = sr(x1 - (W2 + W6) * x2, sh);
    x3 = sr(x1 + (W2 - W6) * x3, sh);
    x1 = x4 + x6;
    x4 = x4 - x6;
    x6 = x5 + x7;
    x5 = x5 - x7;
    x7 = x8 + x3;
    x8 = x8 - x3;
    x3 = x0 + x2;
    x0 = x0 - x2;
    x2 = sr(181u * (x4 + x5) + 128u, 8);
    x4 = sr(181u * (x4 - x5) + 128u, 8);
    const U o[8] = {x7 + x1, x3 + x2, x0 + x4, x8 + x6, x8 - x6, x0 - x4, x3 - x2, x7 - x1};
    for (int k = 0; k < 8; ++k) {
        int32_t v = (int32_t)o[k] >> (row ? 8 : 14);
        if (row) {
            if (mode == kModule) v = (int32_t)((U)v << 14) >> 14;        // the 18-bit row store
        } else {
            const int32_t lo = mode == kModule ? -255 : -256;
            v = v < lo ? lo : v > 255 ? 255 : v;
        }
        a[k] = v;
    }
}

// 7.6.4: the sample at (x, y) of a reference plane moved by half samples (hx, hy); the module rounds the four-sample mean with + 1
M2V_HD inline int32_t predict(const uint8_t *plane, int stride, int x, int y, int hx, int hy, int mode)
{
    const uint8_t *p = plane + (size_t)y * stride + x;
    const int32_t a = p[0];
    if (hx && hy) return (a + p[1] + p[stride] + p[stride + 1] + (mode == kModule ? 1 : 2)) >> 2;
    if (hx) return (a + p[1] + 1) >> 1;
    if (hy) return (a + p[stride] + 1) >> 1;
    return a;
}

M2V_HD inline uint8_t clip255(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// ---------------------------------------------------------------------------------------------------------------------------
// output: byte q of a frame of w x h in layout (M2V_420_*: bit 1 = interleaved chroma, bit 0 = V first) is sample (x, y) of plane
// 0 = Y, 1 = U, 2 = V; run = the bytes from q to the end of its row (out_step walks them)
// ---------------------------------------------------------------------------------------------------------------------------
struct OutAt { uint32_t plane, x, y, run; };

M2V_HD inline OutAt out_locate(uint32_t q, uint32_t w, uint32_t h, int layout)
{
    const uint32_t cw = (w + 1u) / 2u, ch = (h + 1u) / 2u, ysz = w * h;
    const bool semi = (layout & 2) != 0, vfirst = (layout & 1) != 0;
    OutAt o;
    if (q < ysz) { o.plane = 0; o.y = q / w; o.x = q - o.y * w; o.run = w - o.x; return o; }
    q -= ysz;
    uint32_t second;
    if (semi) {
        o.y = q / (2u * cw);
        const uint32_t xx = q - o.y * 2u * cw;
        o.x = xx >> 1; second = xx & 1u; o.run = 2u * cw - xx;
    } else {
        second = q >= cw * ch;
        if (second) q -= cw * ch;
        o.y = q / cw; o.x = q - o.y * cw; o.run = cw - o.x;
    }
    o.plane = 1u + (second ^ (vfirst ? 1u : 0u));
    return o;
}

// the byte behind o, while o.run > 1: the next sample of the row, or - interleaved chroma - the other plane's sample first
M2V_HD inline void out_step(OutAt &o, int layout)
{
    --o.run;
    if (o.plane && (layout & 2)) {
        const uint32_t first = (layout & 1) ? 2u : 1u;
        if (o.plane == first) { o.plane = 3u - first; return; }
        o.plane = first;
    }
    ++o.x;
}

M2V_HD inline uint64_t frame_bytes(uint32_t w, uint32_t h) { return (uint64_t)w * h + 2ull * ((w + 1u) / 2u) * ((h + 1u) / 2u); }

// sample (x, y) of a plane of a decoded picture: planar Y, U, V of W x H = whole macroblocks
M2V_HD inline uint8_t pic_sample(const uint8_t *pic, uint32_t W, uint32_t H, const OutAt &o)
{
    if (!o.plane) return pic[(size_t)o.y * W + o.x];
    return pic[(size_t)W * H + (size_t)(o.plane - 1u) * (W / 2u) * (H / 2u) + (size_t)o.y * (W / 2u) + o.x];
}

// ---------------------------------------------------------------------------------------------------------------------------
// several streams per call (m2v_decode_streams_device): a chunk is a run of whole pictures in batch order, and its table holds one
// entry per picture - everything a slice, a macroblock or an output byte needs of the stream its picture belongs to (the sizes differ
// from stream to stream).  plan_streams (m2v_decode_streams.hpp) fills the tables
// ---------------------------------------------------------------------------------------------------------------------------
struct ChunkPic {
    uint64_t out_off, fb;                                    // the frame's first byte in the output, and its bytes
    uint64_t buf_off, ref_off;                               // the picture's planar slot in the chunk's buffer; the slot of the picture in front of it in ITS stream (0: the carried one)
    uint64_t mb_base;                                        // its first macroblock in the chunk's records
    uint32_t stream, pic, slice0, type, mbw, mbh, w, h;      // slice0: its first slice among the chunk's slices
};

// the picture slice g of a chunk belongs to: the last entry whose slice0 is not behind g (every picture has a slice: slice0 grows)
M2V_HD inline uint32_t chunk_slice_pic(const ChunkPic *t, uint32_t n, uint32_t g)
{
    uint32_t a = 0, b = n;
    while (b - a > 1u) { const uint32_t m = (a + b) / 2u; if (t[m].slice0 <= g) a = m; else b = m; }
    return a;
}

// which picture, byte of its frame and sample output byte o is; o lies inside the chunk's range (the frames of a chunk follow each
// other without a gap: out_off grows by fb)
struct OutByte { uint32_t pic, q; OutAt at; };

M2V_HD inline OutByte streams_out_locate(const ChunkPic *t, uint32_t n, uint64_t o, int layout)
{
    uint32_t a = 0, b = n;
    while (b - a > 1u) { const uint32_t m = (a + b) / 2u; if (t[m].out_off <= o) a = m; else b = m; }
    OutByte r;
    r.pic = a; r.q = (uint32_t)(o - t[a].out_off);
    r.at = out_locate(r.q, t[a].w, t[a].h, layout);
    return r;
}

}  // namespace dec
}  // namespace m2v
