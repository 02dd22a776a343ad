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

// ---------------------------------------------------------------------------------------------------------------------------
// the main syntax (option "decode_syntax" = M2V_SYNTAX_MAIN; decoder.decode_main is the definition): Main-Profile streams of
// progressive frame pictures, I and P, from any encoder.  The functions above keep the module's syntax; these stand beside them and
// use what is syntax-blind of them (bit reader, the five VLC tables, parse_block, vector_inside, the transform, the prediction).
// The arithmetic is M2V_DEC_ISO's.
//
// The grammar stays a set of local rules although user_data, copyright_extension and picture_display_extension may stand between
// the units that matter: every start code is significant or transparent by what it is (main_role: its code, and an extension's
// identifier), a significant one is judged against the significant one in front of it (`prev`: the caller's prefix scan), a
// transparent one by which significant one it stands behind.  A transparent unit still ends where the next start code begins.
// ---------------------------------------------------------------------------------------------------------------------------
enum { rUser = 9, rSkipExt = 10 };                               // behind rEnd: the transparent roles

M2V_HD inline int main_role(const uint8_t *es, uint64_t n, uint64_t e)
{
    const uint32_t c = ev_code(e);
    if (c == 0xB3) return rSeq;
    if (c == 0xB8) return rGop;
    if (c == 0xB7) return rEnd;
    if (c == 0x00) return rPic;
    if (c <= 0xAF) return rSlice;
    if (c == 0xB2) return rUser;
    if (c != 0xB5 || ev_pos(e) + 4 >= n) return rBad;
    switch (es[ev_pos(e) + 4] >> 4) {                            // extension_start_code_identifier
    case 1: return rSeqExt;
    case 2: return rDisp;
    case 8: return rPicExt;
    case 4: case 7: return rSkipExt;                             // copyright_extension, picture_display_extension
    default: return rBad;                                        // quant_matrix_extension and the scalable ones
    }
}

M2V_HD inline bool main_significant(int role) { return role >= rSeq && role <= rEnd; }

M2V_HD inline uint32_t zigzag_position(uint32_t i)               // figure 7-2 the other way: raster index -> zig-zag position
{
    static constexpr uint8_t kPos[64] = {
        0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45,
        52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63
    };
    return kPos[i & 63u];
}

M2V_HD inline uint32_t alternate_to_raster(uint32_t k)           // figure 7-3: alternate scan position -> raster index
{
    static constexpr uint8_t kAlt[64] = {
        0, 8, 16, 24, 1, 9, 2, 10, 17, 25, 32, 40, 48, 56, 57, 49, 41, 33, 26, 18, 3, 11, 4, 12, 19, 27, 34, 42, 50, 58, 35, 43, 51, 59, 20, 28, 5, 13,
        6, 14, 21, 29, 36, 44, 52, 60, 37, 45, 53, 61, 22, 30, 7, 15, 23, 31, 38, 46, 54, 62, 39, 47, 55, 63
    };
    return kAlt[k & 63u];
}

M2V_HD inline int32_t main_scale(uint32_t qcode, uint32_t q_scale_type)      // table 7-6 (code 0 has no scale: 0 in both columns)
{
    static constexpr uint8_t kNonLinear[32] = {
        0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112
    };
    return q_scale_type ? (int32_t)kNonLinear[qcode & 31u] : 2 * (int32_t)(qcode & 31u);
}

// Table B-1 over the next 11 bits: length | increment << 8, increment 34 = macroblock_escape; 0 where no code begins the window
M2V_HD inline uint32_t vlc_increment(uint32_t w11)
{
    if (w11 >> 10) return 1u | 1u << 8;
    static constexpr uint16_t kCode[33] = {
        0b011, 0b010, 0b0011, 0b0010, 0b00011, 0b00010, 0b0000111, 0b0000110, 0b00001011, 0b00001010, 0b00001001, 0b00001000, 0b00000111, 0b00000110,
        0b0000010111, 0b0000010110, 0b0000010101, 0b0000010100, 0b0000010011, 0b0000010010, 0b00000100011, 0b00000100010, 0b00000100001,
        0b00000100000, 0b00000011111, 0b00000011110, 0b00000011101, 0b00000011100, 0b00000011011, 0b00000011010, 0b00000011001, 0b00000011000,
        0b00000001000
    };
    static constexpr uint8_t kLen[33] = {3, 3, 4, 4, 5, 5, 7, 7, 8, 8, 8, 8, 8, 8, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11};
    for (uint32_t k = 0; k < 33u; ++k)
        if ((w11 >> (11u - kLen[k])) == kCode[k]) return kLen[k] | (k + 2u) << 8;
    return 0u;
}

// sequence_header with its matrices (raster order; the defaults where none is loaded), and whether a display extension stood behind
struct MainSeq { SeqHdr h; uint32_t display; uint8_t wi[64], wn[64]; };

// the header's fields into h; every weight of both matrices through weight(matrix 0 = intra / 1 = non-intra, raster index, value) -
// the first header stores them, a repeated one compares them with the first's where they lie, without a copy of its own
template <class Weight>
M2V_HD inline bool main_sequence_header(const uint8_t *es, uint64_t start, uint64_t end, SeqHdr &h, Weight weight)
{
    Bits b = unit_bits(es, start, end);
    h.width = get(b, 12); h.height = get(b, 12); h.aspect = get(b, 4); h.frame_rate_code = get(b, 4); h.bit_rate = get(b, 18);
    bool ok = get(b, 1) == 1;
    h.vbv = get(b, 10); h.constrained = get(b, 1);
    for (int m = 0; m < 2; ++m) {                                // load_intra_quantiser_matrix, load_non_intra_quantiser_matrix
        if (!get(b, 1)) {                                        // the default matrix
            for (uint32_t i = 0; i < 64u; ++i) weight(m, i, m ? 16u : (uint32_t)intra_weight(i));
            continue;
        }
        for (uint32_t k = 0; k < 64u; ++k) {                     // 64 bytes in zig-zag order, 0 forbidden
            const uint32_t v = get(b, 8);
            ok = ok && v != 0;
            weight(m, scan_to_raster(k), v);
        }
    }
    return ok && !b.err && tail_zero(b);
}

// the picture's parameters: what differs from picture to picture in the main syntax
struct PicParams { uint32_t fh, fv, prec, qst, alt; };           // f_code[0][0], [0][1], intra_dc_precision, q_scale_type, alternate_scan

M2V_HD inline uint32_t params_pack(const PicParams &p) { return p.fh | p.fv << 4 | p.prec << 8 | p.qst << 10 | p.alt << 11; }
M2V_HD inline PicParams params_unpack(uint32_t v) { return PicParams{v & 15u, (v >> 4) & 15u, (v >> 8) & 3u, (v >> 10) & 1u, (v >> 11) & 1u}; }

M2V_HD inline bool main_fcode_ok(uint32_t f, uint32_t ptype) { return (f >= 1 && f <= 9) || (ptype == 1 && f == 15); }      // 15: "not used" in an I picture

M2V_HD inline bool main_picture_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, PicParams &p)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    p.fh = get(b, 4); p.fv = get(b, 4);
    skip(b, 8);                                              // the backward ones
    p.prec = get(b, 2);
    ok = ok && get(b, 2) == 3;                               // frame picture
    skip(b, 1);                                              // top_field_first
    ok = ok && get(b, 1) == 1;                               // frame_pred_frame_dct
    ok = ok && get(b, 1) == 0;                               // concealment_motion_vectors
    p.qst = get(b, 1);
    ok = ok && get(b, 1) == 0;                               // intra_vlc_format
    p.alt = get(b, 1);
    skip(b, 4);                                              // repeat_first_field, chroma_420_type, progressive_frame, composite_display_flag
    ok = ok && main_fcode_ok(p.fh, ptype) && main_fcode_ok(p.fv, ptype);
    return ok && !b.err && tail_zero(b);
}

// sequence_header at event i, sequence_extension at i + 1, then user_data and at most one sequence_display_extension: kNone, or the
// start of the first unit that is wrong
template <class Weight>
M2V_HD inline uint64_t main_group(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, SeqHdr &h, uint32_t &display, Weight weight)
{
    const uint64_t p0 = ev_pos(ev[i]);
    if (main_role(es, n, ev[i]) != rSeq || i + 1 >= nev) return p0;
    const uint64_t p1 = ev_pos(ev[i + 1]), p2 = i + 2 < nev ? ev_pos(ev[i + 2]) : n;
    h = SeqHdr{};
    display = 0;
    if (!main_sequence_header(es, p0, p1, h, weight)) return p0;
    if (main_role(es, n, ev[i + 1]) != rSeqExt || !parse_sequence_extension(es, p1, p2, h)) return p1;
    uint32_t j = i + 2;
    while (j < nev && main_role(es, n, ev[j]) == rUser) ++j;     // (bounded by the events)
    if (j < nev && main_role(es, n, ev[j]) == rDisp) {
        if (!parse_display_extension(es, ev_pos(ev[j]), j + 1 < nev ? ev_pos(ev[j + 1]) : n, h)) return ev_pos(ev[j]);
        display = 1;
    }
    return kNone;
}

struct MainPlan { MainSeq seq; uint32_t mbw, mbh; };

M2V_HD inline uint64_t main_first(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, MainPlan &P)
{
    if (!nev) return 0;
    for (uint64_t k = 0, p0 = ev_pos(ev[0]); k < p0; k += 8) if (be64(es, k, p0)) return 0;
    MainSeq &q = P.seq;
    const uint64_t bad = main_group(es, n, ev, nev, 0, q.h, q.display, [&](int m, uint32_t i, uint32_t v) { (m ? q.wn : q.wi)[i & 63u] = (uint8_t)v; });
    if (bad != kNone) return bad;
    const SeqHdr &h = P.seq.h;
    if (!h.width || !h.height || h.width > (uint32_t)kMaxSize || h.height > (uint32_t)kMaxSize) return ev_pos(ev[0]);
    P.mbw = (h.width + 15u) / 16u; P.mbh = (h.height + 15u) / 16u;
    return kNone;
}

// a picture may end here: behind the sequence headers, or behind the slice of the last macroblock row
M2V_HD inline bool main_top(const uint8_t *es, uint64_t n, const uint64_t *ev, int prev, uint32_t mbh)
{
    if (prev < 0) return false;
    const int role = main_role(es, n, ev[prev]);
    return role == rSeqExt || role == rDisp || (role == rSlice && ev_code(ev[prev]) == mbh);
}

// event i by its own rule; prev: the significant event in front of it, -1: none
M2V_HD inline EvInfo main_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, uint64_t last_nz, int prev)
{
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    const int role = main_role(es, n, ev[i]);
    const int prole = prev >= 0 ? main_role(es, n, ev[prev]) : rBad;
    const int before = i ? main_role(es, n, ev[i - 1]) : rBad;      // the event right in front, transparent or not
    const bool top = main_top(es, n, ev, prev, P.mbh);
    bool ok = true;
    switch (role) {
    case rBad: ok = false; break;
    case rSeq:
        if (i) {
            SeqHdr h;                                              // 6.1.1.6: it says what the first one said, matrices included
            uint32_t display;
            bool same = true;
            const uint64_t bad = main_group(es, n, ev, nev, i, h, display,
                                            [&](int m, uint32_t k, uint32_t v) { same = same && (m ? P.seq.wn : P.seq.wi)[k & 63u] == v; });
            if (bad != kNone) r.bad = bad;
            else { ok = top && same && seq_equal(h, P.seq.h) && display == P.seq.display; r.rep = 1; }
        }
        break;
    case rSeqExt: ok = before == rSeq; break;                      // (read with its sequence header)
    case rDisp: { SeqHdr h; ok = prole == rSeqExt && parse_display_extension(es, pos, end, h); break; }
    case rUser: ok = prole == rSeqExt || prole == rDisp || prole == rGop || prole == rPicExt; break;
    case rSkipExt: ok = prole == rPicExt; break;
    case rGop: { const bool good = parse_gop_header(es, pos, end); ok = top && good; r.gop = good; break; }
    case rPic: { const bool good = parse_picture_header(es, pos, end, r.type); ok = (top || prole == rGop) && good; r.pic = good; break; }
    case rPicExt: {
        PicParams p;
        const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
        const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
        ok = before == rPic && main_picture_extension(es, pos, end, ptype, p);
        break;
    }
    case rSlice: {
        const uint32_t c = ev_code(ev[i]);
        ok = c <= P.mbh && (c == 1 ? prole == rPicExt : prole == rSlice && ev_code(ev[prev]) == c - 1);
        break;
    }
    default:                                                       // rEnd: the last code, zeros behind it
        ok = top && i + 1 == nev && last_nz <= pos + 4;
        break;
    }
    if (i + 1 == nev && role != rEnd && ok)                        // no sequence_end_code: the stream ends where a picture may end
        ok = main_top(es, n, ev, main_significant(role) ? (int)i : prev, P.mbh);
    if (!ok) r.bad = min64(r.bad, pos);
    return r;
}

// the parameters of the picture whose header is event i of an accepted stream, and its first slice's event
M2V_HD inline uint32_t main_picture_params(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, uint32_t &slice0)
{
    PicParams p{1, 1, 0, 0, 0};
    uint32_t j = i + 2;
    if (i + 1 < nev) {
        const uint64_t pos = ev_pos(ev[i]);
        (void)main_picture_extension(es, ev_pos(ev[i + 1]), i + 2 < nev ? ev_pos(ev[i + 2]) : n, pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u, p);
    }
    while (j < nev && !main_significant(main_role(es, n, ev[j]))) ++j;
    slice0 = j;
    return params_pack(p);
}

// ---- macroblock layer ----
struct MainMb { uint8_t intra, mc, cbp, qcode; int16_t mvx, mvy; uint8_t skipped, reserved[7]; };      // MbRec with the vectors in 16 bits; mc 0: the zero vector

// 7.6.3.1: the component from its prediction, the motion code, the residual and r_size = f_code - 1
M2V_HD inline int32_t main_vector(int32_t pmv, int32_t code, int32_t residual, int r_size)
{
    const int32_t f = 1 << r_size;
    int32_t delta = code;
    if (f != 1 && code != 0) {
        delta = ((code < 0 ? -code : code) - 1) * f + residual + 1;
        if (code < 0) delta = -delta;
    }
    int32_t v = pmv + delta;
    if (v < -16 * f) v += 32 * f; else if (v > 16 * f - 1) v -= 32 * f;
    return v;
}

// one macroblock behind its address increment: tables B-2 / B-3, the quantiser, the vector, the pattern, the blocks.  qcode: the
// slice's quantiser_scale_code, which a macroblock quantiser replaces.  false = refused
template <class Put>
M2V_HD inline bool main_macroblock(Bits &b, uint32_t ptype, const PicParams &pp, SliceState &s, uint32_t &qcode, MainMb &m, int32_t (&dc)[6], Put put)
{
    bool quant = false, mc = false, pattern = false, intra = false;
    const uint32_t w = peek(b, 6);
    int len;
    if (ptype == 1) {
        if (w >> 5) { len = 1; intra = true; }                                   // '1'      intra
        else if (w >> 4) { len = 2; intra = quant = true; }                      // '01'     intra, quant
        else return false;
    }
    else if (w >> 5) { len = 1; mc = pattern = true; }                           // '1'      MC, coded
    else if (w >> 4) { len = 2; pattern = true; }                                // '01'     No MC, coded
    else if (w >> 3) { len = 3; mc = true; }                                     // '001'    MC, not coded
    else if ((w >> 1) == 3u) { len = 5; intra = true; }                          // '00011'  intra
    else if ((w >> 1) == 2u) { len = 5; quant = mc = pattern = true; }           // '00010'  MC, coded, quant
    else if ((w >> 1) == 1u) { len = 5; quant = pattern = true; }                // '00001'  No MC, coded, quant
    else if (w == 1u) { len = 6; quant = intra = true; }                         // '000001' intra, quant
    else return false;
    skip(b, len);
    if (quant) {
        qcode = get(b, 5);
        if (!qcode) return false;
    }
    int32_t mv[2] = {0, 0};
    if (mc) {
        for (int t = 0; t < 2; ++t) {
            const int r_size = (int)(t ? pp.fv : pp.fh) - 1;
            const uint32_t e = vlc_motion(peek(b, 32));
            if (!e || r_size < 0 || r_size > 8) return false;
            skip(b, (int)(e & 255u));
            int32_t code = (int32_t)(e >> 8);
            if (code && get(b, 1)) code = -code;
            const int32_t residual = code && r_size ? (int32_t)get(b, r_size) : 0;
            s.pmv[t] = mv[t] = main_vector(s.pmv[t], code, residual, r_size);
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
    if (!intra) { for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0; }    // 7.2.1: a macroblock that is not intra resets the DC predictors
    m = MainMb{};
    m.intra = intra; m.mc = mc; m.cbp = (uint8_t)cbp; m.mvx = (int16_t)mv[0]; m.mvy = (int16_t)mv[1];
    for (int blk = 0; blk < 6; ++blk) {
        dc[blk] = 0;
        if (!((cbp >> (5 - blk)) & 1u)) continue;
        // parse_block places through the zig-zag scan: with alternate_scan the same position through figure 7-3
        if (!parse_block(b, intra, blk < 4 ? 0 : blk - 3, s, dc[blk],
                         [&](uint32_t i, int32_t l) { put(blk, pp.alt ? alternate_to_raster(zigzag_position(i)) : i, l); })) return false;
    }
    return !b.err;
}

// the slice of macroblock row `row`: address increments with escapes, skipped macroblocks (P pictures, never the row's first or
// last), mbw macroblocks in all through sink.mb(col, record, dc) and sink.level(col, block, raster index, level), then nothing but
// zero stuffing.  Every pass of the loop moves col forward, an escape by 33: mbw passes at most
template <class Sink>
M2V_HD inline bool main_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, const PicParams &pp, int mbw, int mbh, int row, Sink &sink)
{
    Bits b = unit_bits(es, start, end);
    uint32_t qcode = get(b, 5);
    if (get(b, 1) != 0) return false;                        // extra_bit_slice
    SliceState s{{0, 0, 0}, {0, 0}};
    int col = -1;
    while (col < mbw - 1) {
        int incr = 0;
        uint32_t e;
        for (;;) {
            e = vlc_increment(peek(b, 11));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            if ((e >> 8) != 34u) break;
            incr += 33;                                      // macroblock_escape
            if (col + incr >= mbw) return false;
        }
        incr += (int)(e >> 8);
        if ((col < 0 && incr != 1) || col + incr >= mbw || b.err) return false;
        if (incr > 1) {                                      // 7.6.6: skipped - the zero vector, the predictors reset
            if (ptype != 2) return false;
            MainMb z{};
            z.skipped = 1; z.qcode = (uint8_t)qcode;
            const int32_t none[6] = {0, 0, 0, 0, 0, 0};
            for (int k = 1; k < incr; ++k) sink.mb(col + k, z, none);
            s = SliceState{{0, 0, 0}, {0, 0}};
        }
        col += incr;
        MainMb m;
        int32_t dc[6];
        if (!main_macroblock(b, ptype, pp, s, qcode, m, dc, [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); })) return false;
        if (m.mc && !vector_inside(col, row, m.mvx, m.mvy, mbw, mbh, kIso)) return false;
        m.qcode = (uint8_t)qcode;
        sink.mb(col, m, dc);
    }
    return !b.err && tail_zero(b);
}

// ---- reconstruction ----
M2V_HD inline int32_t main_saturate(int32_t v) { return v > 2047 ? 2047 : v < -2048 ? -2048 : v; }      // 7.4.3

// 7.4.2 with the stream's weight w for the coefficient and the picture's scale, saturated; the intra DC and mismatch control are
// the caller's (main_dequant_dc, mismatch)
M2V_HD inline int32_t main_dequant(int32_t q, int32_t w, bool intra, int32_t qscale)
{
    const int32_t v = (intra ? 2 * q : 2 * q + (q > 0 ? 1 : q < 0 ? -1 : 0)) * w * qscale / 32;
    return main_saturate(v);
}

// the intra DC relative to its reset value, times intra_dc_mult = 8 >> precision (the offset of 1024 is the prediction's 128)
M2V_HD inline int32_t main_dequant_dc(int32_t dc, uint32_t prec)
{
    return main_saturate((int32_t)((uint32_t)dc << (3u - (prec & 3u))));
}

// ---------------------------------------------------------------------------------------------------------------------------
// B pictures (option "decode_b_pictures" on top of the main syntax; decoder.decode_main(b_pictures=True) is the definition).  The
// main_ functions above keep their signatures and their meaning; these stand beside them: a picture header and coding extension that
// know picture_coding_type 3, Table B-4, two vector predictors, a record with both vectors and the directions, the mean of two
// predictions.  An I or P picture goes through main_slice as before and leaves the same kind of record (directions: forward).
// ---------------------------------------------------------------------------------------------------------------------------
enum { kFwd = 1, kBwd = 2 };                                     // the directions of a macroblock's prediction

M2V_HD inline bool bp_picture_header(const uint8_t *es, uint64_t start, uint64_t end, uint32_t &type)
{
    Bits b = unit_bits(es, start, end);
    skip(b, 10);
    type = get(b, 3);
    skip(b, 16);
    bool ok = type >= 1 && type <= 3;                        // D pictures stay refused
    if (type == 2 || type == 3) { ok = ok && get(b, 1) == 0; skip(b, 3); }     // full_pel_forward_vector, forward_f_code
    if (type == 3) { ok = ok && get(b, 1) == 0; skip(b, 3); }                  // full_pel_backward_vector, backward_f_code
    ok = ok && get(b, 1) == 0;                               // extra_bit_picture
    return ok && !b.err && tail_zero(b);
}

// the picture's parameters with the backward f_codes, f_code[1][0] and [1][1]; packed above params_pack's twelve bits
struct BPicParams { PicParams p; uint32_t bh, bv; };

M2V_HD inline uint32_t bp_params_pack(const BPicParams &q) { return params_pack(q.p) | q.bh << 12 | q.bv << 16; }
M2V_HD inline BPicParams bp_params_unpack(uint32_t v) { return BPicParams{params_unpack(v), (v >> 12) & 15u, (v >> 16) & 15u}; }

M2V_HD inline bool bp_picture_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, BPicParams &q)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    q.p.fh = get(b, 4); q.p.fv = get(b, 4);
    q.bh = get(b, 4); q.bv = get(b, 4);
    q.p.prec = get(b, 2);
    ok = ok && get(b, 2) == 3;                               // frame picture
    skip(b, 1);                                              // top_field_first
    ok = ok && get(b, 1) == 1;                               // frame_pred_frame_dct
    ok = ok && get(b, 1) == 0;                               // concealment_motion_vectors
    q.p.qst = get(b, 1);
    ok = ok && get(b, 1) == 0;                               // intra_vlc_format
    q.p.alt = get(b, 1);
    skip(b, 4);                                              // repeat_first_field, chroma_420_type, progressive_frame, composite_display_flag
    ok = ok && main_fcode_ok(q.p.fh, ptype) && main_fcode_ok(q.p.fv, ptype);
    if (ptype == 3) ok = ok && q.bh >= 1 && q.bh <= 9 && q.bv >= 1 && q.bv <= 9;      // (an I or P picture's backward pair is not judged)
    return ok && !b.err && tail_zero(b);
}

// event i by its own rule, as main_event: a picture header may be a B picture's, and its coding extension is judged as one
M2V_HD inline EvInfo bp_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, uint64_t last_nz, int prev)
{
    const int role = main_role(es, n, ev[i]);
    if (role != rPic && role != rPicExt) return main_event(es, n, ev, nev, i, P, last_nz, prev);
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    bool ok;
    if (role == rPic) {
        const int prole = prev >= 0 ? main_role(es, n, ev[prev]) : rBad;
        const bool good = bp_picture_header(es, pos, end, r.type);
        ok = (main_top(es, n, ev, prev, P.mbh) || prole == rGop) && good;
        r.pic = good;
    } else {
        BPicParams q;
        const int before = i ? main_role(es, n, ev[i - 1]) : rBad;
        const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
        const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
        ok = before == rPic && bp_picture_extension(es, pos, end, ptype, q);
    }
    if (i + 1 == nev) ok = false;                            // no stream ends behind a picture header or its extension
    if (!ok) r.bad = pos;
    return r;
}

M2V_HD inline uint32_t bp_picture_params(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, uint32_t &slice0)
{
    BPicParams q{PicParams{1, 1, 0, 0, 0}, 1, 1};
    uint32_t j = i + 2;
    if (i + 1 < nev) {
        const uint64_t pos = ev_pos(ev[i]);
        (void)bp_picture_extension(es, ev_pos(ev[i + 1]), i + 2 < nev ? ev_pos(ev[i + 2]) : n, pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u, q);
    }
    while (j < nev && !main_significant(main_role(es, n, ev[j]))) ++j;
    slice0 = j;
    return bp_params_pack(q);
}

// the display index of an anchor at coded index p whose next anchor is at coded index next (the number of pictures where there is
// none), and of a B picture at p
M2V_HD inline uint32_t bp_display_anchor(uint32_t next) { return next - 1u; }
M2V_HD inline uint32_t bp_display_b(uint32_t p) { return p - 1u; }

// ---- macroblock layer ----
// MainMb with the backward vector and the directions in its reserved bytes; mc = the forward direction, as there
struct BMb { uint8_t intra, mc, cbp, qcode; int16_t mvx, mvy; uint8_t skipped, dirs; int16_t bvx, bvy; uint8_t reserved[2]; };

// Table B-4 over the next 6 bits: length | flags << 8, flags = quant << 4 | forward << 3 | backward << 2 | pattern << 1 | intra; 0 where
// no code begins the window
M2V_HD inline uint32_t vlc_type_b(uint32_t w6)
{
    if ((w6 >> 4) == 2u) return 2u | 0x0Cu << 8;             // '10'     forward, backward
    if ((w6 >> 4) == 3u) return 2u | 0x0Eu << 8;             // '11'     forward, backward, coded
    if ((w6 >> 3) == 2u) return 3u | 0x04u << 8;             // '010'    backward
    if ((w6 >> 3) == 3u) return 3u | 0x06u << 8;             // '011'    backward, coded
    if ((w6 >> 2) == 2u) return 4u | 0x08u << 8;             // '0010'   forward
    if ((w6 >> 2) == 3u) return 4u | 0x0Au << 8;             // '0011'   forward, coded
    if ((w6 >> 1) == 3u) return 5u | 0x01u << 8;             // '00011'  intra
    if ((w6 >> 1) == 2u) return 5u | 0x1Eu << 8;             // '00010'  forward, backward, coded, quant
    if (w6 == 3u) return 6u | 0x1Au << 8;                    // '000011' forward, coded, quant
    if (w6 == 2u) return 6u | 0x16u << 8;                    // '000010' backward, coded, quant
    if (w6 == 1u) return 6u | 0x11u << 8;                    // '000001' intra, quant
    return 0u;
}

// one vector component behind its predictor (7.6.3.1): motion_code, sign, motion_residual of r_size bits; false = refused
M2V_HD inline bool bp_component(Bits &b, int32_t &pmv, int r_size)
{
    const uint32_t e = vlc_motion(peek(b, 32));
    if (!e || r_size < 0 || r_size > 8) return false;
    skip(b, (int)(e & 255u));
    int32_t code = (int32_t)(e >> 8);
    if (code && get(b, 1)) code = -code;
    const int32_t residual = code && r_size ? (int32_t)get(b, r_size) : 0;
    pmv = main_vector(pmv, code, residual, r_size);
    return true;
}

// the vectors a record uses read inside the picture
M2V_HD inline bool bp_inside(int col, int row, const BMb &m, int mbw, int mbh)
{
    return (!(m.dirs & kFwd) || vector_inside(col, row, m.mvx, m.mvy, mbw, mbh, kIso)) &&
           (!(m.dirs & kBwd) || vector_inside(col, row, m.bvx, m.bvy, mbw, mbh, kIso));
}

// a record's vectors from the predictors of the directions it uses: s.pmv is PMV[0][0] (forward), bpmv PMV[0][1] (backward)
M2V_HD inline void bp_vectors(BMb &m, uint32_t dirs, const SliceState &s, const int32_t (&bpmv)[2])
{
    m.dirs = (uint8_t)dirs; m.mc = (dirs & kFwd) != 0;
    if (dirs & kFwd) { m.mvx = (int16_t)s.pmv[0]; m.mvy = (int16_t)s.pmv[1]; }
    if (dirs & kBwd) { m.bvx = (int16_t)bpmv[0]; m.bvy = (int16_t)bpmv[1]; }
}

// one macroblock of a B picture behind its address increment; false = refused
template <class Put>
M2V_HD inline bool bp_macroblock(Bits &b, const BPicParams &pp, SliceState &s, int32_t (&bpmv)[2], uint32_t &qcode, BMb &m, int32_t (&dc)[6], Put put)
{
    const uint32_t e = vlc_type_b(peek(b, 6));
    if (!e) return false;
    skip(b, (int)(e & 255u));
    const uint32_t flags = e >> 8;
    const bool intra = (flags & 1u) != 0, pattern = ((flags >> 1) & 1u) != 0;
    const uint32_t dirs = (((flags >> 3) & 1u) ? (uint32_t)kFwd : 0u) | (((flags >> 2) & 1u) ? (uint32_t)kBwd : 0u);
    if (flags >> 4) {
        qcode = get(b, 5);
        if (!qcode) return false;
    }
    if (dirs & kFwd) { if (!bp_component(b, s.pmv[0], (int)pp.p.fh - 1) || !bp_component(b, s.pmv[1], (int)pp.p.fv - 1)) return false; }
    if (dirs & kBwd) { if (!bp_component(b, bpmv[0], (int)pp.bh - 1) || !bp_component(b, bpmv[1], (int)pp.bv - 1)) return false; }
    if (intra) { s.pmv[0] = s.pmv[1] = 0; bpmv[0] = bpmv[1] = 0; }      // 7.6.3.4; a direction that is not used keeps its predictor
    uint32_t cbp = intra ? 63u : 0u;
    if (pattern) {
        const uint32_t c = vlc_cbp(peek(b, 32));
        if (!c) return false;
        skip(b, (int)(c & 255u));
        cbp = c >> 8;
    }
    if (!intra) { for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0; }       // 7.2.1
    m = BMb{};
    m.intra = intra; m.cbp = (uint8_t)cbp;
    bp_vectors(m, dirs, s, bpmv);
    for (int blk = 0; blk < 6; ++blk) {
        dc[blk] = 0;
        if (!((cbp >> (5 - blk)) & 1u)) continue;
        if (!parse_block(b, intra, blk < 4 ? 0 : blk - 3, s, dc[blk],
                         [&](uint32_t i, int32_t l) { put(blk, pp.p.alt ? alternate_to_raster(zigzag_position(i)) : i, l); })) return false;
    }
    return !b.err;
}

// main_slice's records as BMb: what is not intra predicts forward (a skipped or No-MC macroblock with the zero vector)
template <class Sink>
struct BpAnchorSink {
    Sink &s;
    M2V_HD void mb(int col, const MainMb &m, const int32_t (&dc)[6])
    {
        BMb r{};
        r.intra = m.intra; r.mc = m.mc; r.cbp = m.cbp; r.qcode = m.qcode; r.mvx = m.mvx; r.mvy = m.mvy; r.skipped = m.skipped;
        r.dirs = m.intra ? 0 : (uint8_t)kFwd;
        s.mb(col, r, dc);
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { s.level(col, blk, i, l); }
};

// the slice of macroblock row `row` of a picture of any type through sink.mb(col, BMb, dc) and sink.level: an I or P picture's by
// main_slice, a B picture's here - Table B-4, two predictors, skipped macroblocks that take the directions and vectors in front of
// them (never behind an intra macroblock), every vector of either direction inside the picture.  Bounded as main_slice is
template <class Sink>
M2V_HD inline bool bp_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, const BPicParams &pp, int mbw, int mbh, int row, Sink &sink)
{
    if (ptype != 3) {
        BpAnchorSink<Sink> a{sink};
        return main_slice(es, start, end, ptype, pp.p, mbw, mbh, row, a);
    }
    Bits b = unit_bits(es, start, end);
    uint32_t qcode = get(b, 5);
    if (get(b, 1) != 0) return false;                        // extra_bit_slice
    SliceState s{{0, 0, 0}, {0, 0}};
    int32_t bpmv[2] = {0, 0};
    uint32_t dirs = 0;                                       // of the macroblock in front; 0: intra
    int col = -1;
    while (col < mbw - 1) {
        int incr = 0;
        uint32_t e;
        for (;;) {
            e = vlc_increment(peek(b, 11));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            if ((e >> 8) != 34u) break;
            incr += 33;                                      // macroblock_escape
            if (col + incr >= mbw) return false;
        }
        incr += (int)(e >> 8);
        if ((col < 0 && incr != 1) || col + incr >= mbw || b.err) return false;
        if (incr > 1) {                                      // 7.6.6: skipped - the directions in front, the predictors as vectors, no residual
            if (!dirs) return false;
            BMb z{};
            z.skipped = 1; z.qcode = (uint8_t)qcode;
            bp_vectors(z, dirs, s, bpmv);
            const int32_t none[6] = {0, 0, 0, 0, 0, 0};
            for (int k = 1; k < incr; ++k) {
                if (!bp_inside(col + k, row, z, mbw, mbh)) return false;
                sink.mb(col + k, z, none);
            }
            for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0;
        }
        col += incr;
        BMb m;
        int32_t dc[6];
        if (!bp_macroblock(b, pp, s, bpmv, qcode, m, dc, [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); })) return false;
        if (!bp_inside(col, row, m, mbw, mbh)) return false;
        m.qcode = (uint8_t)qcode;
        dirs = m.dirs;
        sink.mb(col, m, dc);
    }
    return !b.err && tail_zero(b);
}

// 7.6.7.1: the mean of the forward and the backward prediction, each rounded on its own before
M2V_HD inline int32_t bp_mean(int32_t a, int32_t b) { return (a + b + 1) >> 1; }

// the prediction of the sample at (x, y) of a plane for a record: lx, ly the sample's place, (fx, fy) / (bx, by) the plane's vectors
M2V_HD inline int32_t bp_predict(const uint8_t *fwd, const uint8_t *bwd, int stride, int x, int y, uint32_t dirs, int fx, int fy, int bx, int by)
{
    int32_t a = 0, c = 0;
    if (dirs & kFwd) a = predict(fwd, stride, x + (fx >> 1), y + (fy >> 1), fx & 1, fy & 1, kIso);
    if (dirs & kBwd) c = predict(bwd, stride, x + (bx >> 1), y + (by >> 1), bx & 1, by & 1, kIso);
    return dirs == (uint32_t)(kFwd | kBwd) ? bp_mean(a, c) : (dirs & kFwd) ? a : c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Interlaced frame pictures (option "decode_interlaced" on top of the main syntax, "decode_b_pictures" either way;
// decoder.decode_main(interlaced=True) is the definition).  The main_ and bp_ functions above keep their text; these stand beside
// them: the macroblock rows of a sequence that is not progressive, a coding extension that knows frame_pred_frame_dct 0,
// macroblock_modes(), two predictors per direction, field vectors and field prediction, the field-DCT row map, a record of 32 bytes.
// A picture with frame_pred_frame_dct 1 goes through bp_slice / main_slice as before and leaves the same kind of record.
// ---------------------------------------------------------------------------------------------------------------------------
// 6.3.3: the macroblock rows of a frame picture
M2V_HD inline uint32_t il_mbh(uint32_t height, uint32_t progressive_sequence)
{
    return progressive_sequence ? (height + 15u) / 16u : 2u * ((height + 31u) / 32u);
}

// main_first with that rule
M2V_HD inline uint64_t il_first(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, MainPlan &P)
{
    const uint64_t bad = main_first(es, n, ev, nev, P);
    if (bad == kNone) P.mbh = il_mbh(P.seq.h.height, P.seq.h.progressive);
    return bad;
}

// the picture's parameters with `field`: frame_pred_frame_dct 0; packed above bp_params_pack's twenty bits
struct IPicParams { BPicParams b; uint32_t field; };

M2V_HD inline uint32_t il_params_pack(const IPicParams &q) { return bp_params_pack(q.b) | q.field << 20; }
M2V_HD inline IPicParams il_params_unpack(uint32_t v) { return IPicParams{bp_params_unpack(v), (v >> 20) & 1u}; }

// 6.3.10: frame_pred_frame_dct 0 only where neither the sequence nor the frame is progressive
M2V_HD inline bool il_field_allowed(uint32_t progressive_sequence, uint32_t progressive_frame) { return !progressive_sequence && !progressive_frame; }

// b_pictures: whether the backward f_codes of a B picture are judged, as bp_picture_extension does (off, its header is refused)
M2V_HD inline bool il_picture_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, bool b_pictures, uint32_t progressive_sequence,
                                        IPicParams &q)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    q.b.p.fh = get(b, 4); q.b.p.fv = get(b, 4);
    q.b.bh = get(b, 4); q.b.bv = get(b, 4);
    q.b.p.prec = get(b, 2);
    ok = ok && get(b, 2) == 3;                               // frame picture
    skip(b, 1);                                              // top_field_first: read, not acted on
    q.field = get(b, 1) ^ 1u;                                // frame_pred_frame_dct
    ok = ok && get(b, 1) == 0;                               // concealment_motion_vectors
    q.b.p.qst = get(b, 1);
    ok = ok && get(b, 1) == 0;                               // intra_vlc_format
    q.b.p.alt = get(b, 1);
    skip(b, 2);                                              // repeat_first_field, chroma_420_type: read, not acted on
    const uint32_t progressive_frame = get(b, 1);
    skip(b, 1);                                              // composite_display_flag
    ok = ok && (!q.field || il_field_allowed(progressive_sequence, progressive_frame));
    ok = ok && main_fcode_ok(q.b.p.fh, ptype) && main_fcode_ok(q.b.p.fv, ptype);
    if (b_pictures && ptype == 3) ok = ok && q.b.bh >= 1 && q.b.bh <= 9 && q.b.bv >= 1 && q.b.bv <= 9;
    return ok && !b.err && tail_zero(b);
}

// event i by its own rule: bp_event or main_event (P.mbh is il_first's), but a coding extension is judged by il_picture_extension
M2V_HD inline EvInfo il_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, uint64_t last_nz, int prev,
                              bool b_pictures)
{
    if (main_role(es, n, ev[i]) != rPicExt)
        return b_pictures ? bp_event(es, n, ev, nev, i, P, last_nz, prev) : main_event(es, n, ev, nev, i, P, last_nz, prev);
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    IPicParams q;
    const int before = i ? main_role(es, n, ev[i - 1]) : rBad;
    const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
    const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
    bool ok = before == rPic && il_picture_extension(es, pos, end, ptype, b_pictures, P.seq.h.progressive, q);
    if (i + 1 == nev) ok = false;                            // no stream ends behind a picture coding extension
    if (!ok) r.bad = pos;
    return r;
}

M2V_HD inline uint32_t il_picture_params(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, bool b_pictures,
                                         uint32_t progressive_sequence, uint32_t &slice0)
{
    IPicParams q{BPicParams{PicParams{1, 1, 0, 0, 0}, 1, 1}, 0};
    uint32_t j = i + 2;
    if (i + 1 < nev) {
        const uint64_t pos = ev_pos(ev[i]);
        (void)il_picture_extension(es, ev_pos(ev[i + 1]), i + 2 < nev ? ev_pos(ev[i + 2]) : n, pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u, b_pictures,
                                   progressive_sequence, q);
    }
    while (j < nev && !main_significant(main_role(es, n, ev[j]))) ++j;
    slice0 = j;
    return il_params_pack(q);
}

// ---- macroblock layer ----
// BMb with its two reserved bytes given meaning, and sixteen more: the second vector of either direction (a field-based macroblock's
// bottom-field lines; a frame-based one repeats the first) and the field selects, sel[2 * s + r]
struct IMb {
    uint8_t intra, mc, cbp, qcode; int16_t mvx, mvy; uint8_t skipped, dirs; int16_t bvx, bvy; uint8_t motion_type, dct_type;
    int16_t mvx1, mvy1, bvx1, bvy1; uint8_t sel[4]; uint8_t reserved[4];
};
enum { kFieldBased = 1, kFrameBased = 2 };                   // frame_motion_type (0 reserved, 3 dual prime)

// tables B-2 and B-3 over the next 6 bits in vlc_type_b's form: length | flags << 8; 0 where no code begins the window
M2V_HD inline uint32_t il_type_ip(uint32_t w6, uint32_t ptype)
{
    if (ptype == 1) return (w6 >> 5) ? 1u | 0x01u << 8 : (w6 >> 4) ? 2u | 0x11u << 8 : 0u;      // '1' intra; '01' intra, quant
    if (w6 >> 5) return 1u | 0x0Au << 8;                     // '1'      MC, coded
    if (w6 >> 4) return 2u | 0x02u << 8;                     // '01'     No MC, coded
    if (w6 >> 3) return 3u | 0x08u << 8;                     // '001'    MC, not coded
    if ((w6 >> 1) == 3u) return 5u | 0x01u << 8;             // '00011'  intra
    if ((w6 >> 1) == 2u) return 5u | 0x1Au << 8;             // '00010'  MC, coded, quant
    if ((w6 >> 1) == 1u) return 5u | 0x12u << 8;             // '00001'  No MC, coded, quant
    if (w6 == 1u) return 6u | 0x11u << 8;                    // '000001' intra, quant
    return 0u;
}

// macroblock_modes() behind macroblock_type in a picture with frame_pred_frame_dct 0: frame_motion_type where the macroblock has a
// vector, dct_type where it has blocks; false = refused (the reserved motion type, or dual prime)
M2V_HD inline bool il_modes(Bits &b, bool has_vector, bool has_blocks, uint32_t &motion_type, uint32_t &dct_type)
{
    motion_type = kFrameBased; dct_type = 0;
    if (has_vector) {
        motion_type = get(b, 2);
        if (motion_type != (uint32_t)kFieldBased && motion_type != (uint32_t)kFrameBased) return false;
    }
    if (has_blocks) dct_type = get(b, 1);
    return !b.err;
}

// a field vector behind its select (7.6.3.1): the horizontal component as ever; the vertical one predicted from the predictor DIV 2,
// the predictor twice the vector afterwards.  pmv: PMV[r][s]; false = refused
M2V_HD inline bool il_field_vector(Bits &b, int32_t (&pmv)[2], int r_h, int r_v, int32_t &vx, int32_t &vy)
{
    if (!bp_component(b, pmv[0], r_h)) return false;
    int32_t half = pmv[1] >> 1;
    if (!bp_component(b, half, r_v)) return false;
    pmv[1] = 2 * half;
    vx = pmv[0]; vy = half;
    return true;
}

// block_inside for a w x h block: a field prediction's 16 x 8 and 8 x 4
M2V_HD inline bool il_block_inside(int x0, int y0, int mvx, int mvy, int w, int h, int pw, int ph)
{
    const int ix = mvx >> 1, iy = mvy >> 1, hx = mvx & 1, hy = mvy & 1;
    return x0 + ix >= 0 && y0 + iy >= 0 && x0 + ix + w - 1 + hx < pw && y0 + iy + h - 1 + hy < ph;
}

// a field vector reads inside its field: luma 16 x 8 at (16 col, 8 row) of 16 mbw x 8 mbh, chroma 8 x 4 with the halved vector
M2V_HD inline bool il_field_inside(int col, int row, int mvx, int mvy, int mbw, int mbh)
{
    return il_block_inside(16 * col, 8 * row, mvx, mvy, 16, 8, 16 * mbw, 8 * mbh) &&
           il_block_inside(8 * col, 4 * row, chroma_vector(mvx, kIso), chroma_vector(mvy, kIso), 8, 4, 8 * mbw, 4 * mbh);
}

// the vectors a record uses read inside the picture: a frame-based one's as bp_inside, a field-based one's per field
M2V_HD inline bool il_inside(int col, int row, const IMb &m, int mbw, int mbh)
{
    if (m.motion_type != kFieldBased)
        return (!(m.dirs & kFwd) || vector_inside(col, row, m.mvx, m.mvy, mbw, mbh, kIso)) &&
               (!(m.dirs & kBwd) || vector_inside(col, row, m.bvx, m.bvy, mbw, mbh, kIso));
    return (!(m.dirs & kFwd) || (il_field_inside(col, row, m.mvx, m.mvy, mbw, mbh) && il_field_inside(col, row, m.mvx1, m.mvy1, mbw, mbh))) &&
           (!(m.dirs & kBwd) || (il_field_inside(col, row, m.bvx, m.bvy, mbw, mbh) && il_field_inside(col, row, m.bvx1, m.bvy1, mbw, mbh)));
}

// a frame-based record's vectors of direction s from PMV[0][s]: both halves the same
M2V_HD inline void il_frame_vectors(IMb &m, int s, const int32_t (&pmv)[2])
{
    if (s == 0) { m.mvx = m.mvx1 = (int16_t)pmv[0]; m.mvy = m.mvy1 = (int16_t)pmv[1]; }
    else { m.bvx = m.bvx1 = (int16_t)pmv[0]; m.bvy = m.bvy1 = (int16_t)pmv[1]; }
}

// one macroblock of a picture with frame_pred_frame_dct 0 behind its address increment; pmv: PMV[r][s][t]; false = refused
template <class Put>
M2V_HD inline bool il_macroblock(Bits &b, uint32_t ptype, const IPicParams &pp, SliceState &s, int32_t (&pmv)[2][2][2], uint32_t &qcode, IMb &m, int32_t (&dc)[6],
                                 Put put)
{
    const uint32_t e = ptype == 3 ? vlc_type_b(peek(b, 6)) : il_type_ip(peek(b, 6), ptype);
    if (!e) return false;
    skip(b, (int)(e & 255u));
    const uint32_t flags = e >> 8;
    const bool intra = (flags & 1u) != 0, pattern = ((flags >> 1) & 1u) != 0;
    const uint32_t dirs = (((flags >> 3) & 1u) ? (uint32_t)kFwd : 0u) | (((flags >> 2) & 1u) ? (uint32_t)kBwd : 0u);
    uint32_t motion_type, dct_type;
    if (!il_modes(b, dirs != 0, intra || pattern, motion_type, dct_type)) return false;
    if (flags >> 4) {
        qcode = get(b, 5);
        if (!qcode) return false;
    }
    m = IMb{};
    for (int d = 0; d < 2; ++d) {
        if (!(dirs & (d ? (uint32_t)kBwd : (uint32_t)kFwd))) continue;
        const int r_h = (int)(d ? pp.b.bh : pp.b.p.fh) - 1, r_v = (int)(d ? pp.b.bv : pp.b.p.fv) - 1;
        if (motion_type == (uint32_t)kFrameBased) {          // 7.6.3.3: both predictors of the direction follow a frame vector
            if (!bp_component(b, pmv[0][d][0], r_h) || !bp_component(b, pmv[0][d][1], r_v)) return false;
            pmv[1][d][0] = pmv[0][d][0]; pmv[1][d][1] = pmv[0][d][1];
            il_frame_vectors(m, d, pmv[0][d]);
            continue;
        }
        for (int r = 0; r < 2; ++r) {
            int32_t vx, vy;
            m.sel[2 * d + r] = (uint8_t)get(b, 1);           // motion_vertical_field_select[r][s]
            if (!il_field_vector(b, pmv[r][d], r_h, r_v, vx, vy)) return false;
            if (d == 0) { if (r == 0) { m.mvx = (int16_t)vx; m.mvy = (int16_t)vy; } else { m.mvx1 = (int16_t)vx; m.mvy1 = (int16_t)vy; } }
            else { if (r == 0) { m.bvx = (int16_t)vx; m.bvy = (int16_t)vy; } else { m.bvx1 = (int16_t)vx; m.bvy1 = (int16_t)vy; } }
        }
    }
    if (intra || (ptype == 2 && !(dirs & kFwd))) {           // 7.6.3.4: both r, both directions
        for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
    }
    uint32_t cbp = intra ? 63u : 0u;
    if (pattern) {
        const uint32_t c = vlc_cbp(peek(b, 32));
        if (!c) return false;
        skip(b, (int)(c & 255u));
        cbp = c >> 8;
    }
    if (!intra) { for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0; }       // 7.2.1
    m.intra = intra; m.cbp = (uint8_t)cbp; m.mc = (dirs & kFwd) != 0;
    m.dirs = (uint8_t)(intra ? 0u : ptype == 2 ? (uint32_t)kFwd : dirs);      // a P picture's macroblock without a vector: forward, the zero vector
    m.motion_type = (uint8_t)motion_type; m.dct_type = (uint8_t)dct_type;
    for (int blk = 0; blk < 6; ++blk) {
        dc[blk] = 0;
        if (!((cbp >> (5 - blk)) & 1u)) continue;
        if (!parse_block(b, intra, blk < 4 ? 0 : blk - 3, s, dc[blk],
                         [&](uint32_t i, int32_t l) { put(blk, pp.b.p.alt ? alternate_to_raster(zigzag_position(i)) : i, l); })) return false;
    }
    return !b.err;
}

// bp_slice's records as IMb: frame-based, frame DCT
template <class Sink>
struct IlFrameSink {
    Sink &s;
    M2V_HD void mb(int col, const BMb &m, const int32_t (&dc)[6])
    {
        IMb r{};
        r.intra = m.intra; r.mc = m.mc; r.cbp = m.cbp; r.qcode = m.qcode; r.skipped = m.skipped; r.dirs = m.dirs;
        r.mvx = r.mvx1 = m.mvx; r.mvy = r.mvy1 = m.mvy; r.bvx = r.bvx1 = m.bvx; r.bvy = r.bvy1 = m.bvy;
        r.motion_type = (uint8_t)kFrameBased;
        s.mb(col, r, dc);
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { s.level(col, blk, i, l); }
};

// the slice of macroblock row `row` of a picture of any type through sink.mb(col, IMb, dc) and sink.level: a picture with
// frame_pred_frame_dct 1 by bp_slice (an I or P picture's by main_slice behind it); one with 0 here - macroblock_modes, two predictors
// per direction, skipped macroblocks frame-predicted (a P picture's with the zero vector, a B picture's with PMV[0][s]), every vector
// inside the picture or its field.  Bounded as main_slice is
template <class Sink>
M2V_HD inline bool il_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, const IPicParams &pp, int mbw, int mbh, int row, Sink &sink)
{
    if (!pp.field) {
        IlFrameSink<Sink> a{sink};
        return bp_slice(es, start, end, ptype, pp.b, mbw, mbh, row, a);
    }
    Bits b = unit_bits(es, start, end);
    uint32_t qcode = get(b, 5);
    if (get(b, 1) != 0) return false;                        // extra_bit_slice
    SliceState s{{0, 0, 0}, {0, 0}};
    int32_t pmv[2][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};
    uint32_t dirs = 0;                                       // of the macroblock in front; 0: intra
    int col = -1;
    while (col < mbw - 1) {
        int incr = 0;
        uint32_t e;
        for (;;) {
            e = vlc_increment(peek(b, 11));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            if ((e >> 8) != 34u) break;
            incr += 33;                                      // macroblock_escape
            if (col + incr >= mbw) return false;
        }
        incr += (int)(e >> 8);
        if ((col < 0 && incr != 1) || col + incr >= mbw || b.err) return false;
        if (incr > 1) {                                      // 7.6.6: skipped - frame prediction, no residual
            if (ptype == 1) return false;
            IMb z{};
            z.skipped = 1; z.qcode = (uint8_t)qcode; z.motion_type = (uint8_t)kFrameBased;
            if (ptype == 2) {                                // the zero vector, the predictors reset
                z.dirs = (uint8_t)kFwd;
                for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
            } else {                                         // the directions in front, PMV[0][s] as frame vectors
                if (!dirs) return false;
                z.dirs = (uint8_t)dirs; z.mc = (dirs & kFwd) != 0;
                if (dirs & kFwd) il_frame_vectors(z, 0, pmv[0][0]);
                if (dirs & kBwd) il_frame_vectors(z, 1, pmv[0][1]);
            }
            const int32_t none[6] = {0, 0, 0, 0, 0, 0};
            for (int k = 1; k < incr; ++k) {
                if (!il_inside(col + k, row, z, mbw, mbh)) return false;
                sink.mb(col + k, z, none);
            }
            for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0;
        }
        col += incr;
        IMb m;
        int32_t dc[6];
        if (!il_macroblock(b, ptype, pp, s, pmv, qcode, m, dc, [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); })) return false;
        if (!il_inside(col, row, m, mbw, mbh)) return false;
        m.qcode = (uint8_t)qcode;
        dirs = m.dirs;
        sink.mb(col, m, dc);
    }
    return !b.err && tail_zero(b);
}

// the field-DCT row map: the luma block that holds sample (x, y) of a macroblock, and the row inside it
M2V_HD inline uint32_t il_luma_block(uint32_t x, uint32_t y, uint32_t dct_type) { return (dct_type ? (y & 1u) : (y >> 3)) * 2u + (x >> 3); }
M2V_HD inline uint32_t il_luma_row(uint32_t y, uint32_t dct_type) { return dct_type ? y >> 1 : y & 7u; }

// the prediction of the sample at (x, y) of a plane for a record; chroma: the plane is a chroma plane, the vectors are halved toward
// zero.  Frame-based: bp_predict.  Field-based (7.6.4): row y is a line of the field of its parity, predicted by the vector of that
// parity from the field its select names - rows of one parity, twice the stride apart -, at field line y >> 1
M2V_HD inline int32_t il_predict(const uint8_t *fwd, const uint8_t *bwd, int stride, int x, int y, const IMb &m, bool chroma)
{
    const int r = m.motion_type == kFieldBased ? (y & 1) : 0;
    int fx = r ? m.mvx1 : m.mvx, fy = r ? m.mvy1 : m.mvy, bx = r ? m.bvx1 : m.bvx, by = r ? m.bvy1 : m.bvy;
    if (chroma) { fx = chroma_vector(fx, kIso); fy = chroma_vector(fy, kIso); bx = chroma_vector(bx, kIso); by = chroma_vector(by, kIso); }
    if (m.motion_type != kFieldBased) return bp_predict(fwd, bwd, stride, x, y, m.dirs, fx, fy, bx, by);
    const int line = y >> 1;
    const int sf = r ? m.sel[1] : m.sel[0], sb = r ? m.sel[3] : m.sel[2];      // (no index into the record: it stays in registers)
    int32_t a = 0, c = 0;
    if (m.dirs & kFwd) a = predict(fwd + (size_t)sf * stride, 2 * stride, x + (fx >> 1), line + (fy >> 1), fx & 1, fy & 1, kIso);
    if (m.dirs & kBwd) c = predict(bwd + (size_t)sb * stride, 2 * stride, x + (bx >> 1), line + (by >> 1), bx & 1, by & 1, kIso);
    return m.dirs == (kFwd | kBwd) ? bp_mean(a, c) : (m.dirs & kFwd) ? a : c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Several slices a row (option "decode_extended" on top of the main syntax, "decode_b_pictures" and "decode_interlaced" either way;
// decoder.decode_main(extended=True) is the definition).  The functions above keep their text; these stand beside them:
//   slices      a picture is any number of slices, 1 <= code <= mbh: the first behind the picture's extensions has code 1, every
//               further one its predecessor's code or that + 1, and a picture ends only behind code mbh (x_event).  The first
//               macroblock_address_increment of a slice, escapes included, places it: column increment - 1, nothing skipped in front.
//               The macroblock loop runs while anything but zero bits is left in the unit; a slice without a macroblock or one whose
//               column passes mbw - 1 is refused.  All predictors reset at a slice's start (x_slice).
//   continuity  judged behind the walk from what every slice leaves (x_span_pack): a row's first slice starts at column 0 and the row
//               in front of it is full; a slice with its predecessor's code starts one column behind the predecessor's last; the
//               picture's last slice ends at mbw - 1.  A slice that breaks one of these is refused at its own start code (x_continuous).
//   header      behind quantiser_scale_code a bit 1 is intra_slice_flag: intra_slice and reserved_bits (8 bits, not judged), then
//               extra_information_slice bytes, each behind an extra_bit_slice 1, then the closing 0.
//   matrices    quant_matrix_extension (identifier 3) is a transparent unit behind a picture_coding_extension, one a picture at most:
//               the two load flags with 64 bytes each in zig-zag order (a weight of 0 refuses it), the two chroma load flags 0, zero
//               stuffing.  A loaded matrix is in force from its picture on, in coded order, each matrix on its own; every sequence
//               header puts both back to the sequence's (x_mats_*).
//   composite   composite_display_flag 1: the 20 bits behind it are read and not acted on (x_picture_extension).
// ---------------------------------------------------------------------------------------------------------------------------
enum { rQuant = 11 };                                            // quant_matrix_extension: transparent, as rUser and rSkipExt
constexpr uint32_t kNoEvent = 0xFFFFFFFFu;

M2V_HD inline int x_role(const uint8_t *es, uint64_t n, uint64_t e)
{
    const int r = main_role(es, n, e);
    if (r == rBad && ev_code(e) == 0xB5 && ev_pos(e) + 4 < n && (es[ev_pos(e) + 4] >> 4) == 3u) return rQuant;
    return r;
}

// quant_matrix_extension: loads = load_intra | load_non_intra << 1; every loaded weight through weight(matrix, raster index, value)
template <class Weight>
M2V_HD inline bool x_quant_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t &loads, Weight weight)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 3;
    loads = 0;
    for (int m = 0; m < 2; ++m) {
        if (!get(b, 1)) continue;
        loads |= 1u << m;
        for (uint32_t k = 0; k < 64u; ++k) {                     // 64 bytes in zig-zag order, 0 forbidden
            const uint32_t v = get(b, 8);
            ok = ok && v != 0;
            weight(m, scan_to_raster(k), v);
        }
    }
    ok = ok && get(b, 2) == 0;                                   // the chroma load flags: 4:2:0 has no chroma matrices
    return ok && !b.err && tail_zero(b);
}

// the load flags of an extension the plan accepted, and the weight at zig-zag position k of its matrix m
M2V_HD inline uint32_t x_quant_loads(const uint8_t *es, uint64_t start, uint64_t end)
{
    Bits b = unit_bits(es, start, end);
    skip(b, 4);
    const uint32_t li = get(b, 1);
    if (li) skip(b, 512);
    return li | get(b, 1) << 1;
}

M2V_HD inline uint32_t x_quant_weight(const uint8_t *es, uint64_t start, uint64_t end, int m, uint32_t k)
{
    Bits b = unit_bits(es, start, end);
    skip(b, 4);
    const uint32_t li = get(b, 1);
    if (m) { if (li) skip(b, 512); skip(b, 1); }
    skip(b, 8 * (int)(k & 63u));
    return get(b, 8);
}

// the matrices in force, as the events that loaded them (kNoEvent: the sequence's): a sequence header puts both back, an accepted
// quant_matrix_extension replaces what it loads
struct XMats { uint32_t mi, mn; };

M2V_HD inline void x_mats_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, XMats &s)
{
    const int role = x_role(es, n, ev[i]);
    if (role == rSeq) { s.mi = s.mn = kNoEvent; return; }
    if (role != rQuant) return;
    const uint32_t loads = x_quant_loads(es, ev_pos(ev[i]), i + 1 < nev ? ev_pos(ev[i + 1]) : n);
    if (loads & 1u) s.mi = i;
    if (loads & 2u) s.mn = i;
}

// a picture's matrices: what is in force in front of its header, then its own extension (quant: x_picture_params')
M2V_HD inline XMats x_mats_picture(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, XMats s, uint32_t quant)
{
    if (quant != kNoEvent) x_mats_event(es, n, ev, nev, quant, s);
    return s;
}

// the weight at raster index t of matrix m (0 intra, 1 non-intra) whose source is event src: a row of the matrix table
M2V_HD inline uint32_t x_matrix_weight(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t src, int m, uint32_t t, const uint8_t *seq_w)
{
    if (src == kNoEvent || src >= nev) return seq_w[t & 63u];
    return x_quant_weight(es, ev_pos(ev[src]), src + 1 < nev ? ev_pos(ev[src + 1]) : n, m, zigzag_position(t));
}

// il_picture_extension with composite_display_flag 1: v_axis, field_sequence, sub_carrier, burst_amplitude, sub_carrier_phase follow
M2V_HD inline bool x_picture_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, bool b_pictures, bool interlaced,
                                       uint32_t progressive_sequence, IPicParams &q)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    q.b.p.fh = get(b, 4); q.b.p.fv = get(b, 4);
    q.b.bh = get(b, 4); q.b.bv = get(b, 4);
    q.b.p.prec = get(b, 2);
    ok = ok && get(b, 2) == 3;                               // frame picture
    skip(b, 1);                                              // top_field_first
    q.field = get(b, 1) ^ 1u;                                // frame_pred_frame_dct
    ok = ok && get(b, 1) == 0;                               // concealment_motion_vectors
    q.b.p.qst = get(b, 1);
    ok = ok && get(b, 1) == 0;                               // intra_vlc_format
    q.b.p.alt = get(b, 1);
    skip(b, 2);                                              // repeat_first_field, chroma_420_type
    const uint32_t progressive_frame = get(b, 1);
    if (get(b, 1)) skip(b, 20);                              // composite_display_flag and what it announces: read, not acted on
    ok = ok && (!q.field || (interlaced && il_field_allowed(progressive_sequence, progressive_frame)));
    ok = ok && main_fcode_ok(q.b.p.fh, ptype) && main_fcode_ok(q.b.p.fv, ptype);
    if (b_pictures && ptype == 3) ok = ok && q.b.bh >= 1 && q.b.bh <= 9 && q.b.bv >= 1 && q.b.bv <= 9;
    return ok && !b.err && tail_zero(b);
}

// event i by its own rule: il_event / bp_event / main_event as the other two options say (P.mbh is theirs), but a coding extension
// by x_picture_extension, a slice by the grammar above, a quant_matrix_extension behind its picture's coding extension, once
M2V_HD inline EvInfo x_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, uint64_t last_nz, int prev,
                             bool b_pictures, bool interlaced)
{
    const int role = x_role(es, n, ev[i]);
    if (role != rPicExt && role != rSlice && role != rQuant) {
        if (interlaced) return il_event(es, n, ev, nev, i, P, last_nz, prev, b_pictures);
        return b_pictures ? bp_event(es, n, ev, nev, i, P, last_nz, prev) : main_event(es, n, ev, nev, i, P, last_nz, prev);
    }
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    const int prole = prev >= 0 ? main_role(es, n, ev[prev]) : rBad;
    bool ok;
    if (role == rPicExt) {
        IPicParams q;
        const int before = i ? main_role(es, n, ev[i - 1]) : rBad;
        const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
        const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
        ok = before == rPic && x_picture_extension(es, pos, end, ptype, b_pictures, interlaced, P.seq.h.progressive, q) && i + 1 != nev;
    } else if (role == rQuant) {
        ok = prole == rPicExt && i + 1 != nev;
        for (uint32_t j = i; ok && j > (uint32_t)(prev + 1); --j) ok = x_role(es, n, ev[j - 1]) != rQuant;      // (the units between are transparent; ends at the first one found)
        uint32_t loads;
        ok = x_quant_extension(es, pos, end, loads, [](int, uint32_t, uint32_t) {}) && ok;
    } else {
        const uint32_t c = ev_code(ev[i]), pc = prole == rSlice ? ev_code(ev[prev]) : 0u;
        ok = c <= P.mbh && ((c == 1u && prole == rPicExt) || (prole == rSlice && (pc == c || pc + 1u == c)));
        if (i + 1 == nev && ok) ok = main_top(es, n, ev, (int)i, P.mbh);      // no sequence_end_code: the stream ends where a picture may end
    }
    if (!ok) r.bad = pos;
    return r;
}

// the parameters of the picture whose header is event i of an accepted stream, its first slice's event, its number of slices and
// its quant_matrix_extension's event (kNoEvent: none)
M2V_HD inline uint32_t x_picture_params(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, bool b_pictures, bool interlaced,
                                        uint32_t progressive_sequence, uint32_t &slice0, uint32_t &nslices, uint32_t &quant)
{
    IPicParams q{BPicParams{PicParams{1, 1, 0, 0, 0}, 1, 1}, 0};
    uint32_t j = i + 2;
    if (i + 1 < nev) {
        const uint64_t pos = ev_pos(ev[i]);
        (void)x_picture_extension(es, ev_pos(ev[i + 1]), i + 2 < nev ? ev_pos(ev[i + 2]) : n, pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u, b_pictures, interlaced,
                                  progressive_sequence, q);
    }
    quant = kNoEvent;
    for (; j < nev && !main_significant(main_role(es, n, ev[j])); ++j)
        if (quant == kNoEvent && x_role(es, n, ev[j]) == rQuant) quant = j;
    slice0 = j;
    for (; j < nev && main_role(es, n, ev[j]) == rSlice; ++j) {}
    nslices = j - slice0;
    return il_params_pack(q);
}

// the picture of slice g of a chunk whose pictures' entries are t[0 .. n) and the slice's number k inside it: the last entry whose
// sbase (the slices in front of the picture) is not behind g, as chunk_slice_pic above.  sbase never falls; where every picture has a
// slice it grows, and with "decode_conceal" pictures without a slice share theirs with the picture behind them: the LAST such entry
// is the one that owns slice g, so the search passes them (g is below the chunk's slices, so it never ends on a trailing one)
template <class Pic>
M2V_HD inline uint32_t x_slice_pic(const Pic *t, uint32_t n, uint32_t g, uint32_t &k)
{
    const uint32_t base = t[0].sbase;
    uint32_t a = 0, b = n;
    while (b - a > 1u) { const uint32_t m = (a + b) / 2u; if (t[m].sbase - base <= g) a = m; else b = m; }
    k = g - (t[a].sbase - base);
    return a;
}

// what a slice's walk leaves for the judge: ok << 31 | code << 16 | first column << 8 | last column (mbw <= 128, code <= 175)
M2V_HD inline uint32_t x_span_pack(bool ok, uint32_t code, int first, int last)
{
    return (ok ? 1u << 31 : 0u) | (code & 255u) << 16 | ((uint32_t)first & 255u) << 8 | ((uint32_t)last & 255u);
}

// continuity of a readable slice `cur`, slice k of nslices of its picture, behind `front` (k > 0: the span of slice k - 1)
M2V_HD inline bool x_continuous(uint32_t cur, uint32_t front, uint32_t k, uint32_t nslices, uint32_t mbw)
{
    const uint32_t code = (cur >> 16) & 255u, first = (cur >> 8) & 255u, last = cur & 255u;
    const uint32_t fcode = (front >> 16) & 255u, flast = front & 255u;
    bool ok;
    if (k && fcode == code) ok = first == flast + 1u;
    else ok = first == 0u && (!k || flast == mbw - 1u);
    return ok && (k + 1u != nslices || last == mbw - 1u);
}

// main_slice's and bp_slice's records as IMb: frame-based, frame DCT (what BpAnchorSink and IlFrameSink make of them)
M2V_HD inline IMb x_record(const BMb &m)
{
    IMb r{};
    r.intra = m.intra; r.mc = m.mc; r.cbp = m.cbp; r.qcode = m.qcode; r.skipped = m.skipped; r.dirs = m.dirs;
    r.mvx = r.mvx1 = m.mvx; r.mvy = r.mvy1 = m.mvy; r.bvx = r.bvx1 = m.bvx; r.bvy = r.bvy1 = m.bvy;
    r.motion_type = (uint8_t)kFrameBased;
    return r;
}

M2V_HD inline IMb x_record(const MainMb &m)
{
    BMb r{};
    r.intra = m.intra; r.mc = m.mc; r.cbp = m.cbp; r.qcode = m.qcode; r.mvx = m.mvx; r.mvy = m.mvy; r.skipped = m.skipped;
    r.dirs = m.intra ? 0 : (uint8_t)kFwd;
    return x_record(r);
}

// one past the last bit that is 1 in bytes [from, end) of the stream, in bits; 8 * from where all are zero
M2V_HD inline uint64_t x_last_one(const uint8_t *es, uint64_t from, uint64_t end)
{
    uint64_t k = end;
    while (k >= from + 8 && !be64(es, k - 8, end)) k -= 8;   // (the stream's last slice may carry any number of trailing zero bytes)
    while (k > from && !es[k - 1]) --k;
    if (k == from) return 8 * from;
    uint32_t v = es[k - 1], z = 0;
    while (!(v & 1u)) { v >>= 1; ++z; }
    return 8 * k - z;
}

// one slice of a picture of any type, anywhere in macroblock row `row`, through sink.mb(col, IMb, dc) and sink.level: the header with
// its extras, the first increment as the slice's column, then macroblocks - main_macroblock, bp_macroblock or il_macroblock as the
// picture says - while anything but zero bits is left.  first / last: the columns of its first and last macroblock.  Every pass moves
// col forward and col stays below mbw: mbw passes at most
template <class Sink>
M2V_HD inline bool x_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, const IPicParams &pp, int mbw, int mbh, int row, Sink &sink,
                           int &first, int &last)
{
    first = last = -1;
    if (end < start + 4) return false;
    Bits b = unit_bits(es, start, end);
    const uint64_t lim = x_last_one(es, start + 4, end);
    uint32_t qcode = get(b, 5);
    if (get(b, 1)) {                                         // intra_slice_flag
        skip(b, 8);                                          // intra_slice, reserved_bits
        while (get(b, 1)) skip(b, 8);                        // extra_bit_slice, extra_information_slice (a read past the unit is 0)
    }
    if (b.err) return false;
    SliceState s{{0, 0, 0}, {0, 0}};                         // s.pmv: PMV[0][0] of a picture with frame_pred_frame_dct 1
    int32_t pmv[2][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};      // PMV[r][s]; with frame_pred_frame_dct 1 only PMV[0][1] of it
    uint32_t dirs = 0;                                       // of the macroblock in front; 0: intra
    int col = -1;
    const int32_t none[6] = {0, 0, 0, 0, 0, 0};
    while (b.pos < lim) {
        int incr = 0;
        uint32_t e;
        for (;;) {
            e = vlc_increment(peek(b, 11));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            if ((e >> 8) != 34u) break;
            incr += 33;                                      // macroblock_escape
            if (col + incr >= mbw) return false;
        }
        incr += (int)(e >> 8);
        if (col + incr >= mbw || b.err) return false;
        if (col < 0) {                                       // the slice's place: nothing is skipped in front of it
            first = incr - 1;
        } else if (incr > 1) {                               // 7.6.6: skipped - frame prediction, no residual
            if (ptype == 1) return false;
            IMb z{};
            z.skipped = 1; z.qcode = (uint8_t)qcode; z.motion_type = (uint8_t)kFrameBased;
            if (ptype == 2) {                                // the zero vector, the predictors reset
                z.dirs = (uint8_t)kFwd;
                s.pmv[0] = s.pmv[1] = 0;
                for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
            } else {                                         // the directions in front, PMV[0][s] as frame vectors
                if (!dirs) return false;
                z.dirs = (uint8_t)dirs; z.mc = (dirs & kFwd) != 0;
                if (dirs & kFwd) il_frame_vectors(z, 0, pp.field ? pmv[0][0] : s.pmv);
                if (dirs & kBwd) il_frame_vectors(z, 1, pmv[0][1]);
            }
            for (int k = 1; k < incr; ++k) {
                if (!il_inside(col + k, row, z, mbw, mbh)) return false;
                sink.mb(col + k, z, none);
            }
            for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0;
        }
        col += incr;
        IMb m;
        int32_t dc[6];
        auto put = [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); };
        if (pp.field) {
            if (!il_macroblock(b, ptype, pp, s, pmv, qcode, m, dc, put)) return false;
        } else if (ptype == 3) {
            BMb bm;
            if (!bp_macroblock(b, pp.b, s, pmv[0][1], qcode, bm, dc, put)) return false;
            m = x_record(bm);
        } else {
            MainMb mm;
            if (!main_macroblock(b, ptype, pp.b.p, s, qcode, mm, dc, put)) return false;
            m = x_record(mm);
        }
        if (!il_inside(col, row, m, mbw, mbh)) return false;
        m.qcode = (uint8_t)qcode;
        dirs = m.dirs;
        sink.mb(col, m, dc);
    }
    last = col;
    return !b.err && col >= 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The macroblock tools (option "decode_mb_tools" on top of "decode_extended", "decode_b_pictures" and "decode_interlaced" either way;
// decoder.decode_main(extended=True, mb_tools=True) is the definition).  The functions above keep their text; these stand beside them:
//   Table B-15  with the picture's intra_vlc_format 1 the AC coefficients of intra blocks are read with vlc_ac15 (end of block '0110');
//               non-intra blocks keep vlc_ac and the '1s' form (t_block).
//   concealment with concealment_motion_vectors 1 an intra macroblock carries a forward frame vector with f_code[0][*] and a marker bit
//               1 behind its quantiser: it sets PMV[0][0] and PMV[1][0], is not used and not judged against the edges, and such a
//               macroblock does not reset the predictors.  An I picture with the flag carries f_codes 1 .. 9 (t_picture_extension).
//   dual prime  frame_motion_type 3 in a P picture with frame_pred_frame_dct 0: one field vector without a select and a dmvector
//               behind each component.  Its record is a field-based one with both directions whose "backward" picture is the forward
//               reference: selects {0, 1} forward with the vector itself, {1, 0} backward with the derived vectors (t_dual_prime);
//               il_inside judges all four reads, il_predict forms the means.
// One macroblock function reads every picture kind (t_macroblock): a picture with frame_pred_frame_dct 1 has no macroblock_modes(),
// and leaves the records main_macroblock and bp_macroblock leave through x_record.
// ---------------------------------------------------------------------------------------------------------------------------
struct TPicParams { IPicParams i; uint32_t ivf, cmv, tff; };     // intra_vlc_format, concealment_motion_vectors, top_field_first

M2V_HD inline uint32_t t_params_pack(const TPicParams &q) { return il_params_pack(q.i) | q.ivf << 21 | q.cmv << 22 | q.tff << 23; }
M2V_HD inline TPicParams t_params_unpack(uint32_t v) { return TPicParams{il_params_unpack(v), (v >> 21) & 1u, (v >> 22) & 1u, (v >> 23) & 1u}; }

// x_picture_extension with the three flags kept, not refused
M2V_HD inline bool t_picture_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, bool b_pictures, bool interlaced,
                                       uint32_t progressive_sequence, TPicParams &q)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    q.i.b.p.fh = get(b, 4); q.i.b.p.fv = get(b, 4);
    q.i.b.bh = get(b, 4); q.i.b.bv = get(b, 4);
    q.i.b.p.prec = get(b, 2);
    ok = ok && get(b, 2) == 3;                               // frame picture
    q.tff = get(b, 1);                                       // top_field_first: the order of a dual-prime macroblock's derived vectors
    q.i.field = get(b, 1) ^ 1u;                              // frame_pred_frame_dct
    q.cmv = get(b, 1);                                       // concealment_motion_vectors
    q.i.b.p.qst = get(b, 1);
    q.ivf = get(b, 1);                                       // intra_vlc_format
    q.i.b.p.alt = get(b, 1);
    skip(b, 2);                                              // repeat_first_field, chroma_420_type
    const uint32_t progressive_frame = get(b, 1);
    if (get(b, 1)) skip(b, 20);                              // composite_display_flag and what it announces: read, not acted on
    ok = ok && (!q.i.field || (interlaced && il_field_allowed(progressive_sequence, progressive_frame)));
    const uint32_t ftype = q.cmv ? 0u : ptype;               // with concealment vectors an I picture's f_codes are used: 15 is not legal
    ok = ok && main_fcode_ok(q.i.b.p.fh, ftype) && main_fcode_ok(q.i.b.p.fv, ftype);
    if (b_pictures && ptype == 3) ok = ok && q.i.b.bh >= 1 && q.i.b.bh <= 9 && q.i.b.bv >= 1 && q.i.b.bv <= 9;
    return ok && !b.err && tail_zero(b);
}

// Table B-15 without the sign bit, in vlc_ac's form: length | run << 8 | level << 16; level 0: run 0 = end of block, run 1 = escape.
// A window that starts with 1 is classed by its leading ones (five at most, no terminator behind five), any other by its leading
// zeros; behind seven zeros the entries are B-14's, but for the ten pairs whose codes moved: one path for every lane, and two
// dependent table loads a code, as vlc_ac
M2V_HD inline uint32_t vlc_ac15(uint32_t w)
{
    static constexpr uint16_t kAc15Tab[149] = {
        0x0212, 0x0212, 0x0003, 0x0603, 0x0A17, 0x02B7, 0x1607, 0x1407, 0x02D7, 0x02C7, 0x0437, 0x0817, 0x0224, 0x0224, 0x0224, 0x0224, 0x0224,
        0x0224, 0x0224, 0x0224, 0x0414, 0x0414, 0x0414, 0x0414, 0x0414, 0x0414, 0x0414, 0x0414, 0x0234, 0x0234, 0x0234, 0x0234, 0x0234, 0x0234,
        0x0234, 0x0234, 0x0E05, 0x0C05, 0x0245, 0x0255, 0x0276, 0x0286, 0x0266, 0x0426, 0x0015, 0x0458, 0x0458, 0x02E8, 0x02E8, 0x0829, 0x0309,
        0x02F8, 0x02F8, 0xFFFF, 0x048B, 0x064B, 0xFFFF, 0xFFFF, 0x047B, 0x035B, 0x034B, 0xFFFF, 0x033B, 0x032B, 0xFFFF, 0x063B, 0xFFFF, 0x046B,
        0x031B, 0x04AC, 0x049C, 0x065C, 0x083C, 0x0A2C, 0x0E1C, 0x0C1C, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0x03AC, 0x039C, 0x038C, 0x037C, 0x036C,
        0x3E0D, 0x3C0D, 0x3A0D, 0x380D, 0x360D, 0x340D, 0x320D, 0x300D, 0x2E0D, 0x2C0D, 0x2A0D, 0x280D, 0x260D, 0x240D, 0x220D, 0x200D, 0x500E,
        0x4E0E, 0x4C0E, 0x4A0E, 0x480E, 0x460E, 0x440E, 0x420E, 0x400E, 0x1C1E, 0x1A1E, 0x181E, 0x161E, 0x141E, 0x121E, 0x101E, 0x241F, 0x221F,
        0x201F, 0x1E1F, 0x066F, 0x050F, 0x04FF, 0x04EF, 0x04DF, 0x04CF, 0x04BF, 0x03FF, 0x03EF, 0x03DF, 0x03CF, 0x03BF, 0x0201, 0x0402, 0x0804,
        0x0A04, 0x0296, 0x0616, 0x02A6, 0x1006, 0x1206, 0x1206, 0x1807, 0x1A07, 0x0627, 0x0447, 0x1C07, 0x1E07
    };
    static constexpr uint16_t kAc15Z[17] = {                 // leading zeros 1 .. 11, twelve and more, then leading ones 1 .. 5: first entry << 3 | index bits
        0x0002, 0x0025, 0x0122, 0x0142, 0x0160, 0x016B, 0x01AC, 0x022C, 0x02AC, 0x032C, 0x03AC, 0xFFFF, 0x0428, 0x0430, 0x0439, 0x044A, 0x046B
    };
    const bool ones = (w >> 31) != 0;
    const uint32_t v = ones ? ~w : w;
    int z = v ? __builtin_clz(v) : 32;
    if (z > (ones ? 5 : 12)) z = ones ? 5 : 12;
    const int used = ones && z == 5 ? 5 : z + 1;             // the run and the bit that ends it
    const uint32_t d = kAc15Z[ones ? 11 + z : z - 1];
    if (d == 0xFFFFu) return 0u;
    const uint32_t r = d & 7u;
    const uint32_t idx = r ? (w << used) >> (32u - r) : 0u;
    const uint32_t e = kAc15Tab[(d >> 3) + idx];
    return e == 0xFFFFu ? 0u : ((e & 15u) + 1u) | ((e >> 4) & 31u) << 8 | (e >> 9) << 16;
}

// one coefficient of a block behind its DC, by Table B-15 where b15 says so, else by Table B-14 with its '1s' form for a first one:
// 1 = (run, lvl) read, 0 = end of block, -1 = refused
M2V_HD inline int t_coefficient(Bits &b, bool first, bool b15, uint32_t &run, int32_t &lvl)
{
    const uint32_t w = peek(b, 32);
    if (first && !b15 && (int32_t)w < 0) {                   // '1s': run 0, level +-1
        skip(b, 1);
        run = 0;
        lvl = get(b, 1) ? -1 : 1;
        return 1;
    }
    const uint32_t e = b15 ? vlc_ac15(w) : vlc_ac(w);
    if (!e) return -1;
    skip(b, (int)(e & 255u));
    run = (e >> 8) & 255u;
    lvl = (int32_t)(e >> 16);
    if (lvl) {
        if (get(b, 1)) lvl = -lvl;
        return 1;
    }
    if (!run) return 0;                                      // end of block
    run = get(b, 6);                                         // escape: 6 bits of run, 12 of level, 0 and -2048 forbidden
    lvl = (int32_t)(get(b, 12) ^ 0x800u) - 0x800;
    return lvl && lvl != -2048 ? 1 : -1;
}

// parse_block over t_coefficient: Table B-15 for an intra block's AC coefficients where the picture says so (b15)
template <class Put>
M2V_HD inline bool t_block(Bits &b, bool intra, bool b15, int comp, SliceState &s, int32_t &dc, Put put)
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
    for (bool first = !intra; !b.err; first = false) {       // at most 64 coefficients: k grows with every one
        uint32_t run;
        int32_t lvl;
        const int got = t_coefficient(b, first, intra && b15, run, lvl);
        if (got < 0) return false;
        if (!got) return !b.err;
        k += run;
        if (k > 63u || b.err) return false;
        put(scan_to_raster(k), lvl);
        ++k;
    }
    return false;
}

// division by 2 to the nearest integer, halves away from zero
M2V_HD inline int32_t t_half(int32_t a) { return (a + (a > 0 ? 1 : 0)) >> 1; }

// a dual-prime macroblock's record from its vector (vx, vy) and dmvector (d0, d1): field-based, both directions; forward the vector
// itself from the field of the same parity, "backward" the derived vectors from the field of the opposite parity - T for the
// top-field lines, B for the bottom-field lines, the factors 1 and 3 by top_field_first
M2V_HD inline void t_dual_prime(IMb &m, int32_t vx, int32_t vy, int32_t d0, int32_t d1, uint32_t tff)
{
    const int32_t ft = tff ? 1 : 3, fb = tff ? 3 : 1;
    m.mvx = m.mvx1 = (int16_t)vx; m.mvy = m.mvy1 = (int16_t)vy;
    m.bvx = (int16_t)(t_half(ft * vx) + d0); m.bvy = (int16_t)(t_half(ft * vy) + d1 - 1);
    m.bvx1 = (int16_t)(t_half(fb * vx) + d0); m.bvy1 = (int16_t)(t_half(fb * vy) + d1 + 1);
    m.sel[0] = 0; m.sel[1] = 1; m.sel[2] = 1; m.sel[3] = 0;
}

// dmvector: '0' 0, '10' +1, '11' -1
M2V_HD inline int32_t t_dmvector(Bits &b) { return get(b, 1) ? (get(b, 1) ? -1 : 1) : 0; }

// one macroblock of a picture of any kind behind its address increment; pmv: PMV[r][s][t] (a picture with frame_pred_frame_dct 1 uses
// PMV[0][s] only); false = refused
template <class Put>
M2V_HD inline bool t_macroblock(Bits &b, uint32_t ptype, const TPicParams &pp, SliceState &s, int32_t (&pmv)[2][2][2], uint32_t &qcode, IMb &m, int32_t (&dc)[6],
                                Put put)
{
    const uint32_t e = ptype == 3 ? vlc_type_b(peek(b, 6)) : il_type_ip(peek(b, 6), ptype);
    if (!e) return false;
    skip(b, (int)(e & 255u));
    const uint32_t flags = e >> 8;
    const bool intra = (flags & 1u) != 0, pattern = ((flags >> 1) & 1u) != 0;
    const uint32_t dirs = (((flags >> 3) & 1u) ? (uint32_t)kFwd : 0u) | (((flags >> 2) & 1u) ? (uint32_t)kBwd : 0u);
    uint32_t motion_type = kFrameBased, dct_type = 0;
    if (pp.i.field) {                                        // macroblock_modes(): 3 is dual prime, in a P picture only
        if (dirs) {
            motion_type = get(b, 2);
            if (motion_type == 0u || (motion_type == 3u && ptype != 2)) return false;
        }
        if (intra || pattern) dct_type = get(b, 1);
    }
    if (flags >> 4) {
        qcode = get(b, 5);
        if (!qcode) return false;
    }
    m = IMb{};
    bool dual = false;
    if (motion_type == 3u) {                                 // dual prime (a P picture: forward only): component, dmvector, component, dmvector
        if (!bp_component(b, pmv[0][0][0], (int)pp.i.b.p.fh - 1)) return false;
        const int32_t d0 = t_dmvector(b);
        int32_t half = pmv[0][0][1] >> 1;
        if (!bp_component(b, half, (int)pp.i.b.p.fv - 1)) return false;
        const int32_t d1 = t_dmvector(b);
        pmv[0][0][1] = 2 * half;
        pmv[1][0][0] = pmv[0][0][0]; pmv[1][0][1] = pmv[0][0][1];
        t_dual_prime(m, pmv[0][0][0], half, d0, d1, pp.tff);
        dual = true;
    }
    for (int d = 0; d < 2 && !dual; ++d) {
        if (!(dirs & (d ? (uint32_t)kBwd : (uint32_t)kFwd))) continue;
        const int r_h = (int)(d ? pp.i.b.bh : pp.i.b.p.fh) - 1, r_v = (int)(d ? pp.i.b.bv : pp.i.b.p.fv) - 1;
        if (motion_type == (uint32_t)kFrameBased) {          // 7.6.3.3: both predictors of the direction follow a frame vector
            if (!bp_component(b, pmv[0][d][0], r_h) || !bp_component(b, pmv[0][d][1], r_v)) return false;
            pmv[1][d][0] = pmv[0][d][0]; pmv[1][d][1] = pmv[0][d][1];
            il_frame_vectors(m, d, pmv[0][d]);
            continue;
        }
        for (int r = 0; r < 2; ++r) {
            int32_t vx, vy;
            m.sel[2 * d + r] = (uint8_t)get(b, 1);           // motion_vertical_field_select[r][s]
            if (!il_field_vector(b, pmv[r][d], r_h, r_v, vx, vy)) return false;
            if (d == 0) { if (r == 0) { m.mvx = (int16_t)vx; m.mvy = (int16_t)vy; } else { m.mvx1 = (int16_t)vx; m.mvy1 = (int16_t)vy; } }
            else { if (r == 0) { m.bvx = (int16_t)vx; m.bvy = (int16_t)vy; } else { m.bvx1 = (int16_t)vx; m.bvy1 = (int16_t)vy; } }
        }
    }
    if (intra && pp.cmv) {                                   // a concealment vector: kept in the predictors, not used, not judged
        if (!bp_component(b, pmv[0][0][0], (int)pp.i.b.p.fh - 1) || !bp_component(b, pmv[0][0][1], (int)pp.i.b.p.fv - 1)) return false;
        pmv[1][0][0] = pmv[0][0][0]; pmv[1][0][1] = pmv[0][0][1];
        if (!get(b, 1)) return false;                        // marker_bit
    } else if (intra || (ptype == 2 && !(dirs & kFwd))) {    // 7.6.3.4: both r, both directions
        for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
    }
    uint32_t cbp = intra ? 63u : 0u;
    if (pattern) {
        const uint32_t c = vlc_cbp(peek(b, 32));
        if (!c) return false;
        skip(b, (int)(c & 255u));
        cbp = c >> 8;
    }
    if (!intra) { for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0; }       // 7.2.1
    m.intra = intra; m.cbp = (uint8_t)cbp; m.mc = (dirs & kFwd) != 0;
    m.dirs = (uint8_t)(intra ? 0u : dual ? (uint32_t)(kFwd | kBwd) : ptype == 2 ? (uint32_t)kFwd : dirs);
    m.motion_type = (uint8_t)(dual ? (uint32_t)kFieldBased : motion_type); m.dct_type = (uint8_t)dct_type;
    for (int blk = 0; blk < 6; ++blk) {
        dc[blk] = 0;
        if (!((cbp >> (5 - blk)) & 1u)) continue;
        if (!t_block(b, intra, pp.ivf != 0, blk < 4 ? 0 : blk - 3, s, dc[blk],
                     [&](uint32_t i, int32_t l) { put(blk, pp.i.b.p.alt ? alternate_to_raster(zigzag_position(i)) : i, l); })) return false;
    }
    return !b.err;
}

// x_slice over t_macroblock: every picture kind in one walk, the forward predictor PMV[0][0] for all of them
template <class Sink>
M2V_HD inline bool t_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, const TPicParams &pp, int mbw, int mbh, int row, Sink &sink,
                           int &first, int &last)
{
    first = last = -1;
    if (end < start + 4) return false;
    Bits b = unit_bits(es, start, end);
    const uint64_t lim = x_last_one(es, start + 4, end);
    uint32_t qcode = get(b, 5);
    if (get(b, 1)) {                                         // intra_slice_flag
        skip(b, 8);                                          // intra_slice, reserved_bits
        while (get(b, 1)) skip(b, 8);                        // extra_bit_slice, extra_information_slice (a read past the unit is 0)
    }
    if (b.err) return false;
    SliceState s{{0, 0, 0}, {0, 0}};
    int32_t pmv[2][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};      // PMV[r][s]
    uint32_t dirs = 0;                                       // of the macroblock in front; 0: intra
    int col = -1;
    const int32_t none[6] = {0, 0, 0, 0, 0, 0};
    while (b.pos < lim) {
        int incr = 0;
        uint32_t e;
        for (;;) {
            e = vlc_increment(peek(b, 11));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            if ((e >> 8) != 34u) break;
            incr += 33;                                      // macroblock_escape
            if (col + incr >= mbw) return false;
        }
        incr += (int)(e >> 8);
        if (col + incr >= mbw || b.err) return false;
        if (col < 0) {                                       // the slice's place: nothing is skipped in front of it
            first = incr - 1;
        } else if (incr > 1) {                               // 7.6.6: skipped - frame prediction, no residual
            if (ptype == 1) return false;
            IMb z{};
            z.skipped = 1; z.qcode = (uint8_t)qcode; z.motion_type = (uint8_t)kFrameBased;
            if (ptype == 2) {                                // the zero vector, the predictors reset
                z.dirs = (uint8_t)kFwd;
                for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
            } else {                                         // the directions in front, PMV[0][s] as frame vectors
                if (!dirs) return false;
                z.dirs = (uint8_t)dirs; z.mc = (dirs & kFwd) != 0;
                if (dirs & kFwd) il_frame_vectors(z, 0, pmv[0][0]);
                if (dirs & kBwd) il_frame_vectors(z, 1, pmv[0][1]);
            }
            for (int k = 1; k < incr; ++k) {
                if (!il_inside(col + k, row, z, mbw, mbh)) return false;
                sink.mb(col + k, z, none);
            }
            for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0;
        }
        col += incr;
        IMb m;
        int32_t dc[6];
        if (!t_macroblock(b, ptype, pp, s, pmv, qcode, m, dc, [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); })) return false;
        if (!il_inside(col, row, m, mbw, mbh)) return false;
        m.qcode = (uint8_t)qcode;
        dirs = m.dirs;
        sink.mb(col, m, dc);
    }
    last = col;
    return !b.err && col >= 0;
}

// x_event, but a coding extension is judged by t_picture_extension
M2V_HD inline EvInfo t_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, uint64_t last_nz, int prev,
                             bool b_pictures, bool interlaced)
{
    if (x_role(es, n, ev[i]) != rPicExt) return x_event(es, n, ev, nev, i, P, last_nz, prev, b_pictures, interlaced);
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    TPicParams q;
    const int before = i ? main_role(es, n, ev[i - 1]) : rBad;
    const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
    const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
    const bool ok = before == rPic && t_picture_extension(es, pos, end, ptype, b_pictures, interlaced, P.seq.h.progressive, q) && i + 1 != nev;
    if (!ok) r.bad = pos;
    return r;
}

// x_picture_params with t_picture_extension's parameters (t_params_pack)
M2V_HD inline uint32_t t_picture_params(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, bool b_pictures, bool interlaced,
                                        uint32_t progressive_sequence, uint32_t &slice0, uint32_t &nslices, uint32_t &quant)
{
    TPicParams q{IPicParams{BPicParams{PicParams{1, 1, 0, 0, 0}, 1, 1}, 0}, 0, 0, 0};
    uint32_t j = i + 2;
    if (i + 1 < nev) {
        const uint64_t pos = ev_pos(ev[i]);
        (void)t_picture_extension(es, ev_pos(ev[i + 1]), i + 2 < nev ? ev_pos(ev[i + 2]) : n, pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u, b_pictures, interlaced,
                                  progressive_sequence, q);
    }
    quant = kNoEvent;
    for (; j < nev && !main_significant(main_role(es, n, ev[j])); ++j)
        if (quant == kNoEvent && x_role(es, n, ev[j]) == rQuant) quant = j;
    slice0 = j;
    for (; j < nev && main_role(es, n, ev[j]) == rSlice; ++j) {}
    nslices = j - slice0;
    return t_params_pack(q);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Field pictures (option "decode_field_pictures" on top of "decode_interlaced", "decode_extended" and "decode_mb_tools",
// "decode_b_pictures" either way; decoder.decode_main(..., field_pictures=True) is the definition).  The functions above keep their
// text; these stand beside them:
//   extension   picture_structure 1 / 2 where progressive_sequence, progressive_frame, frame_pred_frame_dct, top_field_first and
//               repeat_first_field are 0 (fp_picture_extension); the structure, "second field of its frame" and "no field of the same
//               parity in front" ride in bits 24 .. 27 of the packed parameters.
//   rows        a field has mbh / 2 macroblock rows: a slice's code and the place where a picture may end are judged with the rows of
//               the picture whose coding extension is the nearest in front (fp_field_at, fp_event with the two plans).
//   pairs       a picture is a picture header that reads (fp_is_picture), its structure that of the coding extension right behind
//               it.  A field no first field waits for is a first field; the next picture is its partner, whatever it is (fp_feed),
//               refused unless fp_partner_ok.  The state that crosses a range of events is FpRange: a range is summed twice, once for
//               either state in front of it (fp_range), and the sums are joined in order (fp_join) - a pair parted by a range's edge
//               plans as one inside a range does.
//   macroblocks field_motion_type 1 field-based, 2 16 x 8, 3 dual prime; a select in front of every vector of the first two kinds and
//               of a concealment vector; no component halved; no dct_type (fp_macroblock).  A record is an IMb whose two vectors of a
//               direction are those of the upper and the lower 16 x 8 (a 16 x 16 prediction says the same twice) and whose selects name
//               the parity; dual prime is both directions, "backward" the other parity with the derived vector.
//   prediction  fp_predict: a sample of a field from the field of parity sel[.] of the frame that direction and parity name (fp_ref).
// ---------------------------------------------------------------------------------------------------------------------------
struct FPicParams { TPicParams t; uint32_t ps, second, noref; }; // picture_structure; the second field of its frame; no field of its own parity in front

M2V_HD inline uint32_t fp_params_pack(const FPicParams &q) { return t_params_pack(q.t) | q.ps << 24 | q.second << 26 | q.noref << 27; }
M2V_HD inline FPicParams fp_params_unpack(uint32_t v) { return FPicParams{t_params_unpack(v), (v >> 24) & 3u, (v >> 26) & 1u, (v >> 27) & 1u}; }
M2V_HD inline bool fp_is_field(uint32_t ps) { return ps == 1u || ps == 2u; }

// t_picture_extension that knows picture_structure 1 and 2
M2V_HD inline bool fp_picture_extension(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, bool b_pictures, uint32_t progressive_sequence, FPicParams &q)
{
    Bits b = unit_bits(es, start, end);
    bool ok = get(b, 4) == 8;
    TPicParams &t = q.t;
    t.i.b.p.fh = get(b, 4); t.i.b.p.fv = get(b, 4);
    t.i.b.bh = get(b, 4); t.i.b.bv = get(b, 4);
    t.i.b.p.prec = get(b, 2);
    q.ps = get(b, 2);
    t.tff = get(b, 1);
    t.i.field = get(b, 1) ^ 1u;                              // frame_pred_frame_dct
    t.cmv = get(b, 1);
    t.i.b.p.qst = get(b, 1);
    t.ivf = get(b, 1);
    t.i.b.p.alt = get(b, 1);
    const uint32_t repeat_first_field = get(b, 1);
    skip(b, 1);                                              // chroma_420_type
    const uint32_t progressive_frame = get(b, 1);
    if (get(b, 1)) skip(b, 20);                              // composite_display_flag and what it announces
    if (fp_is_field(q.ps)) ok = ok && !progressive_sequence && !progressive_frame && t.i.field && !t.tff && !repeat_first_field;
    else ok = ok && q.ps == 3u;
    ok = ok && (!t.i.field || il_field_allowed(progressive_sequence, progressive_frame));
    const uint32_t ftype = t.cmv ? 0u : ptype;
    ok = ok && main_fcode_ok(t.i.b.p.fh, ftype) && main_fcode_ok(t.i.b.p.fv, ftype);
    if (b_pictures && ptype == 3) ok = ok && t.i.b.bh >= 1 && t.i.b.bh <= 9 && t.i.b.bv >= 1 && t.i.b.bv <= 9;
    return ok && !b.err && tail_zero(b);
}

// the picture_structure bits of the coding extension at event j (3 where they are not there)
M2V_HD inline uint32_t fp_structure_bits(const uint8_t *es, uint64_t n, uint64_t e) { return ev_pos(e) + 6 < n ? es[ev_pos(e) + 6] & 3u : 3u; }

// whether the slice at event j belongs to a field picture: the coding extension nearest in front says so (bounded by j)
M2V_HD inline bool fp_field_at(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t j)
{
    for (uint32_t k = j; k > 0; --k)
        if (main_role(es, n, ev[k - 1]) == rPicExt && ev_pos(ev[k - 1]) + 6 < n) return fp_is_field(fp_structure_bits(es, n, ev[k - 1]));
    return false;
}

// event i by its own rule: t_event with the rows of the picture the event is judged against - its own where it is a slice, else that of
// the slice in front (Pf: P with mbh / 2) -, a coding extension by fp_picture_extension
M2V_HD inline EvInfo fp_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, const MainPlan &Pf, uint64_t last_nz,
                              int prev, bool b_pictures)
{
    const int role = x_role(es, n, ev[i]);
    if (role == rPicExt) {
        EvInfo r{kNone, 0, 0, 0, 0};
        const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
        FPicParams q;
        const int before = i ? main_role(es, n, ev[i - 1]) : rBad;
        const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
        const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
        const bool ok = before == rPic && fp_picture_extension(es, pos, end, ptype, b_pictures, P.seq.h.progressive, q) && i + 1 != nev;
        if (!ok) r.bad = pos;
        return r;
    }
    const int j = role == rSlice ? (int)i : prev >= 0 && main_role(es, n, ev[prev]) == rSlice ? prev : -1;
    const bool field = j >= 0 && fp_field_at(es, n, ev, (uint32_t)j);
    return t_event(es, n, ev, nev, i, field ? Pf : P, last_nz, prev, b_pictures, true);
}

// whether event i is a picture: its header reads (what t_event's EvInfo::pic says); its type, temporal_reference and the structure of
// the coding extension right behind it (3: a frame picture, or none there)
M2V_HD inline bool fp_is_picture(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, bool b_pictures, uint32_t &type, uint32_t &tref, uint32_t &ps)
{
    if (ev_code(ev[i]) != 0x00u) return false;
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    if (!(b_pictures ? bp_picture_header(es, pos, end, type) : parse_picture_header(es, pos, end, type))) return false;
    tref = (uint32_t)es[pos + 4] << 2 | es[pos + 5] >> 6;    // (the header read: its bytes are there)
    ps = 3u;
    if (i + 1 < nev && main_role(es, n, ev[i + 1]) == rPicExt) ps = fp_structure_bits(es, n, ev[i + 1]);
    if (!ps) ps = 3u;
    return true;
}

// a first field that waits for its partner: 0 none, else 1 << 31 | temporal_reference << 5 | type << 2 | structure
M2V_HD inline uint32_t fp_open_pack(uint32_t ps, uint32_t type, uint32_t tref) { return 1u << 31 | tref << 5 | type << 2 | ps; }

// the partner of the first field `open`: the other parity, the same temporal_reference, the same type or P behind I
M2V_HD inline bool fp_partner_ok(uint32_t open, uint32_t ps, uint32_t type, uint32_t tref)
{
    const uint32_t ops = open & 3u, otype = (open >> 2) & 7u, otref = (open >> 5) & 1023u;
    return fp_is_field(ps) && ps != ops && tref == otref && (type == otype || (otype == 1u && type == 2u));
}

// what a run of pictures leaves: frames begun, I frames, anchor frames; the last I frame, the last two anchor frames and the coded
// index of the last one's first picture (-1: none; counted from the run's first frame / picture); the first field that waits, its frame
struct FpRange { uint32_t frames, ni, na; int32_t last, a1, a2, a1cp; uint32_t open, openf; };

M2V_HD inline FpRange fp_range_none() { return FpRange{0, 0, 0, -1, -1, -1, -1, 0, 0}; }

// one picture, the cp-th of the run, into the run's sums: true = it begins a frame, false = it is the partner of the field that waited
M2V_HD inline bool fp_feed(FpRange &r, uint32_t cp, uint32_t ps, uint32_t type, uint32_t tref)
{
    if (r.open) { r.open = 0; return false; }
    const int32_t f = (int32_t)r.frames++;
    if (type == 1u) { r.last = f; ++r.ni; }
    if (type != 3u) { r.a2 = r.a1; r.a1 = f; r.a1cp = (int32_t)cp; ++r.na; }
    if (fp_is_field(ps)) { r.open = fp_open_pack(ps, type, tref); r.openf = (uint32_t)f; }
    return true;
}

// the pictures of events [a, b) summed twice: A with nothing waiting in front, B with a first field waiting (the first picture is its
// partner); m: the pictures
M2V_HD inline void fp_range(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t a, uint32_t b, bool b_pictures, FpRange &A, FpRange &B, uint32_t &m)
{
    A = B = fp_range_none();
    m = 0;
    for (uint32_t i = a; i < b; ++i) {
        uint32_t type, tref, ps;
        if (!fp_is_picture(es, n, ev, nev, i, b_pictures, type, tref, ps)) continue;
        (void)fp_feed(A, m, ps, type, tref);
        if (m) (void)fp_feed(B, m, ps, type, tref);
        ++m;
    }
}

// `in`: the sums of everything in front (absolute), cp pictures; a range of m pictures follows - its sums A or B as `in` says
M2V_HD inline void fp_join(FpRange &in, uint32_t &cp, const FpRange &A, const FpRange &B, uint32_t m)
{
    if (!m) return;                                          // (a field that waits goes on waiting)
    const FpRange &r = in.open ? B : A;
    const int32_t base = (int32_t)in.frames;
    if (r.last >= 0) in.last = base + r.last;
    if (r.na >= 2u) { in.a2 = base + r.a2; in.a1 = base + r.a1; }
    else if (r.na == 1u) { in.a2 = in.a1; in.a1 = base + r.a1; }
    if (r.na) in.a1cp = (int32_t)cp + r.a1cp;
    in.frames += r.frames; in.ni += r.ni; in.na += r.na;
    in.open = r.open; in.openf = (uint32_t)base + r.openf;
    cp += m;
}

// what the plan knows of a coded picture beyond its parameters
struct FpPlace { uint32_t frame, second, fwd, bwd; bool bad; };  // fwd / bwd: frames (0xFFFFFFFF: none)

// picture (ps, type, tref) at coded index cp behind the sums `s` (absolute): its place, and s moved on.  bad: refused at its header - not
// a legal partner, no I frame so far, a B picture without two anchor frames
M2V_HD inline FpPlace fp_place(FpRange &s, uint32_t cp, uint32_t ps, uint32_t type, uint32_t tref)
{
    FpPlace q{0, 0, kNoEvent, kNoEvent, false};
    const uint32_t open = s.open, openf = s.openf;
    const int32_t a1 = s.a1, a2 = s.a2;                      // the anchor frames in front of this picture's frame, if it begins one
    if (fp_feed(s, cp, ps, type, tref)) {
        q.frame = s.frames - 1u;
        if (type == 2u) q.fwd = q.bwd = (uint32_t)a1;        // (a dual-prime macroblock's second prediction reads the same frame)
        if (type == 3u) { q.fwd = (uint32_t)a2; q.bwd = (uint32_t)a1; }
    } else {
        q.frame = openf; q.second = 1;
        q.bad = !fp_partner_ok(open, ps, type, tref);
        // the field of its own parity: in the anchor frame in front of its own frame (its own frame is s.a1 where it is an anchor)
        if (type == 2u) q.fwd = q.bwd = (uint32_t)(s.a1 == (int32_t)openf ? s.a2 : s.a1);
        if (type == 3u) { q.fwd = (uint32_t)s.a2; q.bwd = (uint32_t)s.a1; }
    }
    q.bad = q.bad || s.last < 0 || (type == 3u && s.na < 2u);
    return q;
}

// fp_picture_params: t_picture_params with fp_picture_extension's parameters (the place's bits are the caller's)
M2V_HD inline FPicParams fp_picture_params(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, bool b_pictures, uint32_t progressive_sequence,
                                           uint32_t &slice0, uint32_t &nslices, uint32_t &quant)
{
    FPicParams q{TPicParams{IPicParams{BPicParams{PicParams{1, 1, 0, 0, 0}, 1, 1}, 0}, 0, 0, 0}, 3, 0, 0};
    uint32_t j = i + 2;
    if (i + 1 < nev) {
        const uint64_t pos = ev_pos(ev[i]);
        (void)fp_picture_extension(es, ev_pos(ev[i + 1]), i + 2 < nev ? ev_pos(ev[i + 2]) : n, pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u, b_pictures, progressive_sequence, q);
    }
    quant = kNoEvent;
    for (; j < nev && !main_significant(main_role(es, n, ev[j])); ++j)
        if (quant == kNoEvent && x_role(es, n, ev[j]) == rQuant) quant = j;
    slice0 = j;
    for (; j < nev && main_role(es, n, ev[j]) == rSlice; ++j) {}
    nslices = j - slice0;
    return q;
}

// ---- macroblock layer of a field picture ----
// the two vectors of direction d (the upper and the lower 16 x 8) and their selects
M2V_HD inline void fp_set_vector(IMb &m, int d, int r, int32_t vx, int32_t vy, uint32_t sel)
{
    if (d == 0) { if (r == 0) { m.mvx = (int16_t)vx; m.mvy = (int16_t)vy; } else { m.mvx1 = (int16_t)vx; m.mvy1 = (int16_t)vy; } }
    else { if (r == 0) { m.bvx = (int16_t)vx; m.bvy = (int16_t)vy; } else { m.bvx1 = (int16_t)vx; m.bvy1 = (int16_t)vy; } }
    m.sel[2 * d + r] = (uint8_t)sel;
}

// which reference fields a field picture has: bit 2 d + q, direction d, parity q.  A P field's "backward" fields are its forward ones
M2V_HD inline uint32_t fp_have(uint32_t ptype, const FPicParams &pp)
{
    if (ptype == 1u) return 0u;
    if (ptype == 3u) return 15u;
    const uint32_t par = pp.ps - 1u;
    const uint32_t f = pp.noref ? 1u << (par ^ 1u) : 3u;     // the second field of the stream's first frame: only its first field
    return f | f << 2;
}

// the reads of a record lie inside fields that are there: both halves of either direction (a 16 x 16 read is inside where both of its
// halves are, the vector being the same); rows: the field's macroblock rows
M2V_HD inline bool fp_inside(int col, int row, const IMb &m, int mbw, int rows, uint32_t have)
{
    bool ok = true;
    if (m.dirs & kFwd) ok = ok && ((have >> m.sel[0]) & 1u) && ((have >> m.sel[1]) & 1u) && il_field_inside(col, 2 * row, m.mvx, m.mvy, mbw, 2 * rows) &&
                            il_field_inside(col, 2 * row + 1, m.mvx1, m.mvy1, mbw, 2 * rows);
    if (m.dirs & kBwd) ok = ok && ((have >> (2u + m.sel[2])) & 1u) && ((have >> (2u + m.sel[3])) & 1u) && il_field_inside(col, 2 * row, m.bvx, m.bvy, mbw, 2 * rows) &&
                            il_field_inside(col, 2 * row + 1, m.bvx1, m.bvy1, mbw, 2 * rows);
    return ok;
}

// one macroblock of a field picture behind its address increment; pmv: PMV[r][s][t]; false = refused
template <class Put>
M2V_HD inline bool fp_macroblock(Bits &b, uint32_t ptype, const FPicParams &pp, SliceState &s, int32_t (&pmv)[2][2][2], uint32_t &qcode, IMb &m, int32_t (&dc)[6], Put put)
{
    const uint32_t e = ptype == 3 ? vlc_type_b(peek(b, 6)) : il_type_ip(peek(b, 6), ptype);
    if (!e) return false;
    skip(b, (int)(e & 255u));
    const uint32_t flags = e >> 8;
    const bool intra = (flags & 1u) != 0, pattern = ((flags >> 1) & 1u) != 0;
    const uint32_t dirs = (((flags >> 3) & 1u) ? (uint32_t)kFwd : 0u) | (((flags >> 2) & 1u) ? (uint32_t)kBwd : 0u);
    const uint32_t par = pp.ps - 1u;
    const BPicParams &f = pp.t.i.b;
    uint32_t motion_type = 1;                                // field_motion_type: 1 field-based, 2 16 x 8, 3 dual prime (a P field only)
    if (dirs) {
        motion_type = get(b, 2);
        if (motion_type == 0u || (motion_type == 3u && ptype != 2)) return false;
    }
    if (flags >> 4) {
        qcode = get(b, 5);
        if (!qcode) return false;
    }
    m = IMb{};
    for (int k = 0; k < 4; ++k) m.sel[k] = (uint8_t)par;
    bool dual = false;
    if (motion_type == 3u) {                                 // component, dmvector, component, dmvector; no select
        if (!bp_component(b, pmv[0][0][0], (int)f.p.fh - 1)) return false;
        const int32_t d0 = t_dmvector(b);
        if (!bp_component(b, pmv[0][0][1], (int)f.p.fv - 1)) return false;
        const int32_t d1 = t_dmvector(b);
        pmv[1][0][0] = pmv[0][0][0]; pmv[1][0][1] = pmv[0][0][1];
        const int32_t vx = pmv[0][0][0], vy = pmv[0][0][1];
        const int32_t ox = t_half(vx) + d0, oy = t_half(vy) + d1 + (par ? 1 : -1);
        for (int r = 0; r < 2; ++r) { fp_set_vector(m, 0, r, vx, vy, par); fp_set_vector(m, 1, r, ox, oy, par ^ 1u); }
        dual = true;
    }
    for (int d = 0; d < 2 && !dual; ++d) {
        if (!(dirs & (d ? (uint32_t)kBwd : (uint32_t)kFwd))) continue;
        const int r_h = (int)(d ? f.bh : f.p.fh) - 1, r_v = (int)(d ? f.bv : f.p.fv) - 1;
        if (motion_type == 1u) {                             // field-based: from PMV[0][s]; PMV[1][s] follows
            const uint32_t sel = get(b, 1);
            if (!bp_component(b, pmv[0][d][0], r_h) || !bp_component(b, pmv[0][d][1], r_v)) return false;
            pmv[1][d][0] = pmv[0][d][0]; pmv[1][d][1] = pmv[0][d][1];
            for (int r = 0; r < 2; ++r) fp_set_vector(m, d, r, pmv[0][d][0], pmv[0][d][1], sel);
            continue;
        }
        for (int r = 0; r < 2; ++r) {                        // 16 x 8: vector r from and into PMV[r][s]
            const uint32_t sel = get(b, 1);
            if (!bp_component(b, pmv[r][d][0], r_h) || !bp_component(b, pmv[r][d][1], r_v)) return false;
            fp_set_vector(m, d, r, pmv[r][d][0], pmv[r][d][1], sel);
        }
    }
    if (intra && pp.t.cmv) {                                 // a concealment vector behind its select: kept in the predictors, not used
        skip(b, 1);
        if (!bp_component(b, pmv[0][0][0], (int)f.p.fh - 1) || !bp_component(b, pmv[0][0][1], (int)f.p.fv - 1)) return false;
        pmv[1][0][0] = pmv[0][0][0]; pmv[1][0][1] = pmv[0][0][1];
        if (!get(b, 1)) return false;                        // marker_bit
    } else if (intra || (ptype == 2 && !(dirs & kFwd))) {    // 7.6.3.4
        for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
    }
    uint32_t cbp = intra ? 63u : 0u;
    if (pattern) {
        const uint32_t c = vlc_cbp(peek(b, 32));
        if (!c) return false;
        skip(b, (int)(c & 255u));
        cbp = c >> 8;
    }
    if (!intra) { for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0; }       // 7.2.1
    m.intra = intra; m.cbp = (uint8_t)cbp; m.mc = (dirs & kFwd) != 0;
    m.dirs = (uint8_t)(intra ? 0u : dual ? (uint32_t)(kFwd | kBwd) : ptype == 2 ? (uint32_t)kFwd : dirs);      // a P field's macroblock without a vector: the zero vector, its own parity
    m.motion_type = (uint8_t)kFieldBased;
    for (int blk = 0; blk < 6; ++blk) {
        dc[blk] = 0;
        if (!((cbp >> (5 - blk)) & 1u)) continue;
        if (!t_block(b, intra, pp.t.ivf != 0, blk < 4 ? 0 : blk - 3, s, dc[blk],
                     [&](uint32_t i, int32_t l) { put(blk, f.p.alt ? alternate_to_raster(zigzag_position(i)) : i, l); })) return false;
    }
    return !b.err;
}

// t_slice for a field picture: rows macroblock rows, fp_macroblock, skipped macroblocks field-predicted from the field of the same parity
template <class Sink>
M2V_HD inline bool fp_slice(const uint8_t *es, uint64_t start, uint64_t end, uint32_t ptype, const FPicParams &pp, int mbw, int rows, int row, Sink &sink,
                            int &first, int &last)
{
    first = last = -1;
    if (end < start + 4) return false;
    Bits b = unit_bits(es, start, end);
    const uint64_t lim = x_last_one(es, start + 4, end);
    uint32_t qcode = get(b, 5);
    if (get(b, 1)) {                                         // intra_slice_flag
        skip(b, 8);
        while (get(b, 1)) skip(b, 8);
    }
    if (b.err) return false;
    const uint32_t have = fp_have(ptype, pp), par = pp.ps - 1u;
    SliceState s{{0, 0, 0}, {0, 0}};
    int32_t pmv[2][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};
    uint32_t dirs = 0;
    int col = -1;
    const int32_t none[6] = {0, 0, 0, 0, 0, 0};
    while (b.pos < lim) {
        int incr = 0;
        uint32_t e;
        for (;;) {
            e = vlc_increment(peek(b, 11));
            if (!e) return false;
            skip(b, (int)(e & 255u));
            if ((e >> 8) != 34u) break;
            incr += 33;                                      // macroblock_escape
            if (col + incr >= mbw) return false;
        }
        incr += (int)(e >> 8);
        if (col + incr >= mbw || b.err) return false;
        if (col < 0) {
            first = incr - 1;
        } else if (incr > 1) {                               // 7.6.6: skipped - field prediction from the same parity, no residual
            if (ptype == 1) return false;
            IMb z{};
            z.skipped = 1; z.qcode = (uint8_t)qcode; z.motion_type = (uint8_t)kFieldBased;
            for (int k = 0; k < 4; ++k) z.sel[k] = (uint8_t)par;
            if (ptype == 2) {                                // the zero vector, the predictors reset
                z.dirs = (uint8_t)kFwd;
                for (int r = 0; r < 2; ++r) for (int d = 0; d < 2; ++d) pmv[r][d][0] = pmv[r][d][1] = 0;
            } else {                                         // the directions in front, PMV[0][s]
                if (!dirs) return false;
                z.dirs = (uint8_t)dirs; z.mc = (dirs & kFwd) != 0;
                for (int d = 0; d < 2; ++d)
                    if (dirs & (d ? (uint32_t)kBwd : (uint32_t)kFwd)) for (int r = 0; r < 2; ++r) fp_set_vector(z, d, r, pmv[0][d][0], pmv[0][d][1], par);
            }
            for (int k = 1; k < incr; ++k) {
                if (!fp_inside(col + k, row, z, mbw, rows, have)) return false;
                sink.mb(col + k, z, none);
            }
            for (int c = 0; c < 3; ++c) s.dc_pred[c] = 0;
        }
        col += incr;
        IMb m;
        int32_t dc[6];
        if (!fp_macroblock(b, ptype, pp, s, pmv, qcode, m, dc, [&](int blk, uint32_t i, int32_t l) { sink.level(col, blk, i, l); })) return false;
        if (!fp_inside(col, row, m, mbw, rows, have)) return false;
        m.qcode = (uint8_t)qcode;
        dirs = m.dirs;
        sink.mb(col, m, dc);
    }
    last = col;
    return !b.err && col >= 0;
}

// the prediction of the sample at (x, y) of a field for a record of a field picture: y is a line of the field, r the half of the
// macroblock it lies in.  ref[2 d + q]: the frame plane that holds the field of parity q of direction d (the field is rows q, q + 2, ..
// of it; stride: the frame's); chroma: the vectors are halved toward zero
M2V_HD inline int32_t fp_predict(const uint8_t *const (&ref)[4], int stride, int x, int y, int r, const IMb &m, bool chroma)
{
    int fx = r ? m.mvx1 : m.mvx, fy = r ? m.mvy1 : m.mvy, bx = r ? m.bvx1 : m.bvx, by = r ? m.bvy1 : m.bvy;
    if (chroma) { fx = chroma_vector(fx, kIso); fy = chroma_vector(fy, kIso); bx = chroma_vector(bx, kIso); by = chroma_vector(by, kIso); }
    const int sf = r ? m.sel[1] : m.sel[0], sb = r ? m.sel[3] : m.sel[2];
    int32_t a = 0, c = 0;
    if (m.dirs & kFwd) a = predict((sf ? ref[1] : ref[0]) + (size_t)sf * stride, 2 * stride, x + (fx >> 1), y + (fy >> 1), fx & 1, fy & 1, kIso);
    if (m.dirs & kBwd) c = predict((sb ? ref[3] : ref[2]) + (size_t)sb * stride, 2 * stride, x + (bx >> 1), y + (by >> 1), bx & 1, by & 1, kIso);
    return m.dirs == (kFwd | kBwd) ? bp_mean(a, c) : (m.dirs & kFwd) ? a : c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Streams cut from a broadcast (option "decode_join", bits kJoinHead and kJoinTail, on top of all of "decode_interlaced",
// "decode_extended", "decode_mb_tools" and "decode_field_pictures", "decode_b_pictures" either way; decoder.decode(..., join=) is the
// definition).  The functions above keep their text; these stand beside them:
//   window      the stream is read as its bytes [J, T): J the first sequence_header_code (head; else 0), T the start of the frame the
//               stream breaks off in (tail; else its end).  Everything above runs over the window's events with T as the stream's
//               length - a plan hands them the event list from J's event on, and adds that event's index to what it stores.
//   pairs       JPair is the pairing of fp_feed alone, over EVERY picture from J on, with the first picture of the frame a picture
//               belongs to: a range of events is summed for either state in front of it (j_pair_range) and the sums are joined in
//               order (j_pair_join), which also finds F - the last picture start code that begins a frame; one whose header does not
//               read begins one unless a first field waits, and leaves the pairing alone - and E2, the picture that begins the second anchor frame behind J.
//               No picture start code lies behind the window's last slice, so a picture of the window pairs as it does in the whole.
//   tail        T is the first group_start_code or picture_start_code behind the last slice in front of F (j_last_slice, j_first_head)
//   drop        a frame whose first picture is a B picture in front of E2 is dropped (j_dropped), its second field with it: its
//               units are judged by fp_event as any, its partner by fp_partner_ok (j_place), and it is absent from the sums
//               (j_keep_range), the tables, the slices counted in front of a picture and the record.  Dropped frames are whole, so
//               what is kept pairs among itself; only a range's first picture may be the partner of a kept field in front of it.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kJoinHead = 1u, kJoinTail = 2u;
constexpr uint32_t kJInherit = 1u;                               // JSum::out.open: the field that waited in front still waits

// the first sequence_header_code of events [a, b) (kNoEvent: none)
M2V_HD inline uint32_t j_first_seq(const uint64_t *ev, uint32_t a, uint32_t b)
{
    for (uint32_t i = a; i < b; ++i) if (ev_code(ev[i]) == 0xB3u) return i;
    return kNoEvent;
}

// il_first for a header group at J: nothing in front of it is judged
M2V_HD inline uint64_t j_first(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, MainPlan &P)
{
    if (!nev) return 0;
    MainSeq &q = P.seq;
    const uint64_t bad = main_group(es, n, ev, nev, 0, q.h, q.display, [&](int m, uint32_t i, uint32_t v) { (m ? q.wn : q.wi)[i & 63u] = (uint8_t)v; });
    if (bad != kNone) return bad;
    const SeqHdr &h = P.seq.h;
    if (!h.width || !h.height || h.width > (uint32_t)kMaxSize || h.height > (uint32_t)kMaxSize) return ev_pos(ev[0]);
    P.mbw = (h.width + 15u) / 16u; P.mbh = il_mbh(h.height, h.progressive);
    return kNone;
}

// open: fp_open_pack of the first field that waits (0: none); ff, fb: the event of the first picture of the frame the last picture
// belongs to (kNoEvent: none so far) and whether it is a B picture
struct JPair { uint32_t open, ff, fb; };
// what a range of events leaves, the state behind it; the last picture start code that begins a frame; the first two that begin an anchor frame
struct JSum { JPair out; uint32_t lastf, an1, an2; };
// the join: the state in front of the next range; anchor frames so far (2: two or more); E2; F
struct JScan { JPair in; uint32_t na, e2, f; };

M2V_HD inline JScan j_scan_none() { return JScan{JPair{0, kNoEvent, 0}, 0, kNoEvent, kNoEvent}; }

// the picture at event i into the pairing: true = it begins a frame
M2V_HD inline bool j_pair_feed(JPair &w, uint32_t i, uint32_t ps, uint32_t type, uint32_t tref)
{
    if (w.open) { w.open = 0; return false; }
    w.ff = i; w.fb = type == 3u;
    if (fp_is_field(ps)) w.open = fp_open_pack(ps, type, tref);
    return true;
}

// events [a, b) summed twice: A with nothing waiting in front, B with a first field waiting
M2V_HD inline void j_pair_range(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t a, uint32_t b, bool b_pictures, JSum &A, JSum &B)
{
    A = B = JSum{JPair{0, kNoEvent, 0}, kNoEvent, kNoEvent, kNoEvent};
    B.out.open = kJInherit;
    for (uint32_t i = a; i < b; ++i) {
        if (ev_code(ev[i]) != 0x00u) continue;
        uint32_t type, tref, ps;
        if (!fp_is_picture(es, n, ev, nev, i, b_pictures, type, tref, ps)) {      // it begins a frame unless a field waits for it
            if (!A.out.open) A.lastf = i;
            if (!B.out.open) B.lastf = i;
            continue;
        }
        for (int k = 0; k < 2; ++k) {
            JSum &s = k ? B : A;
            if (!j_pair_feed(s.out, i, ps, type, tref)) continue;
            s.lastf = i;
            if (type == 3u) continue;
            if (s.an1 == kNoEvent) s.an1 = i;
            else if (s.an2 == kNoEvent) s.an2 = i;
        }
    }
}

M2V_HD inline void j_pair_join(JScan &t, const JSum &A, const JSum &B)
{
    const JSum &r = t.in.open ? B : A;
    if (r.lastf != kNoEvent) t.f = r.lastf;
    if (t.na < 2u && r.an1 != kNoEvent) {
        if (t.na == 1u) { t.e2 = r.an1; t.na = 2u; }
        else if (r.an2 != kNoEvent) { t.e2 = r.an2; t.na = 2u; }
        else t.na = 1u;
    }
    if (r.out.ff != kNoEvent) { t.in.ff = r.out.ff; t.in.fb = r.out.fb; }
    if (r.out.open != kJInherit) t.in.open = r.out.open;
}

// the last slice of events [a, b), and the first group_start_code or picture_start_code (kNoEvent: none)
M2V_HD inline uint32_t j_last_slice(const uint64_t *ev, uint32_t a, uint32_t b)
{
    for (uint32_t i = b; i > a; --i) { const uint32_t c = ev_code(ev[i - 1u]); if (c >= 1u && c <= 0xAFu) return i - 1u; }
    return kNoEvent;
}

M2V_HD inline uint32_t j_first_head(const uint64_t *ev, uint32_t a, uint32_t b)
{
    for (uint32_t i = a; i < b; ++i) { const uint32_t c = ev_code(ev[i]); if (c == 0x00u || c == 0xB8u) return i; }
    return kNoEvent;
}

// one past the last byte of [0, t) that is not zero, for the one rule that asks: a sequence_end_code as the window's last unit
M2V_HD inline uint64_t j_last_nz(const uint8_t *es, uint64_t t, const uint64_t *ev, uint32_t nev)
{
    if (!nev || ev_code(ev[nev - 1u]) != 0xB7u) return t;
    uint64_t k = t;
    for (const uint64_t lo = ev_pos(ev[nev - 1u]) + 4u; k > lo && !es[k - 1u]; --k) {}
    return k;
}

// whether the frame the pairing stands in is dropped: its first picture is a B picture in front of the second anchor frame
M2V_HD inline bool j_dropped(const JPair &w, uint32_t e2, bool drop) { return drop && w.ff != kNoEvent && w.fb && w.ff < e2; }

// the picture at event i behind the pairing w: whether it is dropped; bad: the second field of a dropped frame that is no legal partner
M2V_HD inline bool j_place(JPair &w, uint32_t i, uint32_t ps, uint32_t type, uint32_t tref, uint32_t e2, bool drop, bool &bad)
{
    const uint32_t open = w.open;
    const bool begins = j_pair_feed(w, i, ps, type, tref);
    const bool gone = j_dropped(w, e2, drop);
    bad = gone && !begins && !fp_partner_ok(open, ps, type, tref);
    return gone;
}

// the kept pictures of events [a, b) behind the pairing w: their sums r (the first of them left out where it is the partner of a
// field in front of the range, as fp_range's B), m of them, ns slices of theirs, and the frames dropped
struct JKeep { FpRange r; uint32_t m, ns, dropped; };

M2V_HD inline void j_keep_range(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t a, uint32_t b, bool b_pictures, JPair w, uint32_t e2, bool drop,
                                JKeep &k)
{
    k.r = fp_range_none();
    k.m = k.ns = k.dropped = 0;
    bool front = w.open != 0u, gone = j_dropped(w, e2, drop);
    for (uint32_t i = a; i < b; ++i) {
        const uint32_t code = ev_code(ev[i]);
        if (code != 0x00u) { k.ns += code <= 0xAFu && !gone; continue; }
        uint32_t type, tref, ps;
        if (!fp_is_picture(es, n, ev, nev, i, b_pictures, type, tref, ps)) continue;
        const bool begins = j_pair_feed(w, i, ps, type, tref);
        gone = j_dropped(w, e2, drop);
        if (gone) k.dropped += begins;
        else {
            if (begins || !front) (void)fp_feed(k.r, k.m, ps, type, tref);
            ++k.m;
        }
        front = false;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Damaged slices (option "decode_conceal" on top of all of "decode_interlaced", "decode_extended", "decode_mb_tools" and
// "decode_field_pictures", "decode_b_pictures" either way, "decode_join" 0 .. 3; decoder.decode(..., conceal=True) is the
// definition).  The functions above keep their text; these stand beside them:
//   grammar     c_event: fp_event's rules, but a slice is legal behind a coding extension or a slice whatever the two codes are, and a
//               picture may end behind a slice of any code or behind its coding extension (c_top).  No rule reads the rows
//   bad slice   a slice whose code is above its picture's rows (c_bad_code) is not walked; its span says "not readable" with its code,
//               which is no row's
//   rows        c_row_kept: the spans of a picture that carry a row's code, in stream order - all readable, the first from column 0,
//               each further one from the last column of the one in front + 1, the last to column mbw - 1.  Any other row is concealed
//   record      c_record: every macroblock of a concealed row - a P picture's skipped macroblock (a field: field-based from its own
//               parity), or intra without a block where no frame stands in front
//   reference   c_place: fp_place, but an I picture is placed with a P picture's forward frame
// ---------------------------------------------------------------------------------------------------------------------------
M2V_HD inline bool c_top(const uint8_t *es, uint64_t n, const uint64_t *ev, int prev)
{
    if (prev < 0) return false;
    const int role = main_role(es, n, ev[prev]);
    return role == rSeqExt || role == rDisp || role == rSlice || role == rPicExt;
}

// event i by its own rule; prev: the significant event in front of it, -1: none
M2V_HD inline EvInfo c_event(const uint8_t *es, uint64_t n, const uint64_t *ev, uint32_t nev, uint32_t i, const MainPlan &P, uint64_t last_nz, int prev, bool b_pictures)
{
    const int role = x_role(es, n, ev[i]);
    if (role == rQuant) return x_event(es, n, ev, nev, i, P, last_nz, prev, b_pictures, true);      // (behind a coding extension, once, never the last unit)
    EvInfo r{kNone, 0, 0, 0, 0};
    const uint64_t pos = ev_pos(ev[i]), end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
    const int prole = prev >= 0 ? main_role(es, n, ev[prev]) : rBad;
    const int before = i ? main_role(es, n, ev[i - 1]) : rBad;      // the event right in front, transparent or not
    const bool top = c_top(es, n, ev, prev);
    bool ok = true;
    switch (role) {
    case rBad: ok = false; break;
    case rSeq:
        if (i) {
            SeqHdr h;
            uint32_t display;
            bool same = true;
            const uint64_t bad = main_group(es, n, ev, nev, i, h, display,
                                            [&](int m, uint32_t k, uint32_t v) { same = same && (m ? P.seq.wn : P.seq.wi)[k & 63u] == v; });
            if (bad != kNone) r.bad = bad;
            else { ok = top && same && seq_equal(h, P.seq.h) && display == P.seq.display; r.rep = 1; }
        }
        break;
    case rSeqExt: ok = before == rSeq; break;
    case rDisp: { SeqHdr h; ok = prole == rSeqExt && parse_display_extension(es, pos, end, h); break; }
    case rUser: ok = prole == rSeqExt || prole == rDisp || prole == rGop || prole == rPicExt; break;
    case rSkipExt: ok = prole == rPicExt; break;
    case rGop: { const bool good = parse_gop_header(es, pos, end); ok = top && good; r.gop = good; break; }
    case rPic: {
        const bool good = b_pictures ? bp_picture_header(es, pos, end, r.type) : parse_picture_header(es, pos, end, r.type);
        ok = (top || prole == rGop) && good;
        r.pic = good;
        break;
    }
    case rPicExt: {
        FPicParams q;
        const uint64_t pp = i ? ev_pos(ev[i - 1]) : 0;
        const uint32_t ptype = before == rPic && pp + 5 < n ? (es[pp + 5] >> 3) & 7u : 0u;
        ok = before == rPic && fp_picture_extension(es, pos, end, ptype, b_pictures, P.seq.h.progressive, q);
        break;
    }
    case rSlice: ok = prole == rPicExt || prole == rSlice; break;
    default:                                                       // rEnd: the last code, zeros behind it
        ok = top && i + 1 == nev && last_nz <= pos + 4;
        break;
    }
    if (i + 1 == nev && role != rEnd && ok)                        // no sequence_end_code: the stream ends where a picture may end
        ok = c_top(es, n, ev, main_significant(role) ? (int)i : prev);
    if (!ok) r.bad = min64(r.bad, pos);
    return r;
}

// fp_place, but an I picture gets the forward frame a P picture would get in its place
M2V_HD inline FpPlace c_place(FpRange &s, uint32_t cp, uint32_t ps, uint32_t type, uint32_t tref)
{
    const int32_t a1 = s.a1;
    const uint32_t openf = s.openf;
    FpPlace q = fp_place(s, cp, ps, type, tref);
    if (type == 1u) {
        // a second I field: s.a1 is its own frame (its first field was an I field too), the frame in front s.a2
        const int32_t f = q.second ? (s.a1 == (int32_t)openf ? s.a2 : s.a1) : a1;
        q.fwd = q.bwd = (uint32_t)f;
    }
    return q;
}

M2V_HD inline bool c_bad_code(uint32_t code, uint32_t rows) { return code < 1u || code > rows; }

// whether the row with slice code `code` is kept: spans[0 .. nslices) are the picture's, in stream order
M2V_HD inline bool c_row_kept(const uint32_t *spans, uint32_t nslices, uint32_t code, uint32_t mbw)
{
    uint32_t next = 0;
    bool seen = false, ok = true;
    for (uint32_t k = 0; k < nslices; ++k) {
        const uint32_t s = spans[k];
        if (((s >> 16) & 255u) != code) continue;
        seen = true;
        ok = ok && (s >> 31) && ((s >> 8) & 255u) == next;
        next = (s & 255u) + 1u;
    }
    return seen && ok && next == mbw;
}

// the record of every macroblock of a concealed row; grey: no frame stands in front
M2V_HD inline IMb c_record(bool field, uint32_t par, bool grey)
{
    IMb m{};
    if (grey) { m.intra = 1; m.motion_type = (uint8_t)kFrameBased; return m; }
    m.skipped = 1; m.dirs = (uint8_t)kFwd;
    m.motion_type = (uint8_t)(field ? kFieldBased : kFrameBased);
    for (int k = 0; k < 4; ++k) m.sel[k] = (uint8_t)(field ? par : 0u);
    return m;
}

// what a call concealed, as m2v_decode_conceal of include/m2v_mi355x.h carries it
struct CReport { uint64_t first_offset; uint32_t bad_slices, concealed_rows, grey_rows, damaged_pictures; };

}  // namespace dec
}  // namespace m2v
