// m2v_types.hpp — structures and constants shared by the device code (m2v_kernels.hpp) and the host translation units
// (m2v_host.hpp): what crosses a kernel launch.  No device code here: host-only sources include this, not the kernels.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace m2v {

// -DM2V_DEBUG builds libm2v_mi355x_dbg.so, the library the stage-level parity tests and the profiling scripts load:
// it can dump the quantised levels and keep every frame's reconstruction (option "keep_recon").  The shipped library
// has none of that code in its kernels.
#ifdef M2V_DEBUG
constexpr bool kDebug = true;
#else
constexpr bool kDebug = false;
#endif

// ----------------------------------------------------------------------------------------------
// shared host/device structures
// ----------------------------------------------------------------------------------------------
struct Geom {
    int W, H;        // clamped luma size (RTL:985-1006)
    int mbw, mbh;    // macroblocks per row / column
    int cw, ch;      // chroma plane size
    int Q;           // Q_LEVEL
    int mbs;         // mbw * mbh
    uint32_t ysz;    // W*H
    uint32_t csz;    // cw*ch
    uint32_t rysz;   // bytes of the luma tiles of a reconstruction: (mbw + 1) * mbh * 256 (the chroma tiles follow; m2v_kernels.hpp, rec_luma_off)
    int row0, row1;  // macroblock rows this GPU encodes: [0, mbh) normally, a strip in multi-GPU strip mode
    int strip;       // 1 = strip mode: the stream buffer holds only this strip's slices, no headers
    uint32_t strip_mbs;      // (row1 - row0) * mbw
    uint32_t magic_strip;    // floor(2^32 / strip_mbs), floor(2^32 / mbw): wave-uniform divisions on the scalar unit
    uint32_t magic_mbw;      // (geom_finish() fills the three after any change of the rows)
    uint32_t s16_off;        // word offset of the 64-byte slot class inside the compact-slot buffer (plan_chunk: macroblocks of the chunk * 32)
    uint32_t s8_off;         // ... and of the 32-byte class behind it
    int cu_pack;             // experiment (xcd_remap): option "cu_pack"
    int rstride;             // macroblock rows between the launch's local rows: 1 normally; the EDGE launch of strip mode runs two local
                             // rows, the strip's first and its last (row0 and row0 + rstride)
    int edge_top, edge_bot;  // strip mode: the strip's first and last macroblock row (k_mb<.., EDGE> copies their outer rows of the
                             // reconstruction into the halo buffers)
};

inline void geom_finish(Geom &g)
{
    if (g.rstride == 0) g.rstride = 1;
    g.strip_mbs = (uint32_t)((g.row1 - g.row0) * g.mbw);
    g.magic_strip = g.strip_mbs > 1 ? (uint32_t)(0x100000000ull / g.strip_mbs) : 0xFFFFFFFFu;
    g.magic_mbw = g.mbw > 1 ? (uint32_t)(0x100000000ull / (uint32_t)g.mbw) : 0xFFFFFFFFu;
}

// Which macroblock a block of a k_mb launch works on, worked out by the HOST once per launch shape (m2v_launch.hip, mbmap_for) and read
// with one scalar load: the XCD / CU permutation (xcd_remap), the row / column split and the neighbour flags were ~60 scalar
// instructions at the head of every macroblock, on a scalar unit that four SIMDs share and that is as busy as the vector ALUs
// (profiles/r04_experiments.txt item 19).
struct MbMap {
    uint32_t mb;            // bits 0-23: macroblock index by * mbw + bx; bit 24 / 25 / 26 / 27: it has a neighbour on the left / right / above / below
                            // (inside the FRAME); bit 28: the block is one of the strip's edge rows (k_mb<.., EDGE>)
    uint32_t byx;           // by << 16 | bx
};

struct FrameJob {           // one per frame of the chunk (device memory)
    const uint8_t *in;      // 4:4:4 planar frame: Y, U, V planes of W*H bytes
    const uint8_t *ref;     // reconstruction of the previous frame (4:2:0 planar) or nullptr
    uint8_t       *rec;     // where to store this frame's reconstruction, nullptr = not needed
    int32_t        i_frame; // index inside the GOP, 0 = I frame (RTL:1078)
    uint32_t       n;       // frame number inside the sequence (time code, RTL:2685-2698)
    uint32_t       valid_beats;  // beats of real input in this frame; the rest is black (RTL:1048-1056)
    uint32_t       fidx;    // k_mb's copies in launch-list order: the frame's index in the chunk (0 in the per-frame array)
    int32_t        hidx;    // strip mode: the frame's position in its GOP step's halo list (frames whose reconstruction is referenced later), -1 = none
    int32_t        rhidx;   // ... and that of its reference frame in the previous step's list (where the neighbours' rows of it were received)
    uint32_t       q;       // the level (1..4) the frame's GOP is coded at: the handle's Q_LEVEL, or m2v_set_gop_levels' entry; k_assemble prints it
                            // in the slice headers, k_gop_judge raises it (k_mb takes the level from its launch's Geom::Q, not from here)
    uint32_t       pad;     // 0 in a call of one sequence.  In a batch (m2v_set_sequences) a flags word: kSeqFirst / kSeqLast, and from bit
                            // kSeqOrdShift on the ordinal of the frame's sequence among those the chunk touches (k_seq_scan, k_assemble)
                            // (the structure is compared and copied as whole dwords: no unnamed padding)
};
constexpr uint32_t kSeqFirst = 1u;      // the frame is the first of its sequence: the sequence headers stand in front of it
constexpr uint32_t kSeqLast = 2u;       // ... the last: sequence_end_code and the final word's padding follow it
constexpr int kSeqOrdShift = 2;

// what k_scene_judge leaves per frame of a chunk, on the device and in pinned memory (option "scene_cut")
struct SceneRec { unsigned long long diff; uint32_t flag; uint32_t pad; };
static_assert(sizeof(SceneRec) == 16, "k_scene_judge writes the record in place");

struct StreamCtl {          // device-resident stream bookkeeping, carried across chunks
    unsigned long long base_bytes;   // bytes of the stream already produced before this chunk
    unsigned long long total_bytes;  // bytes after this chunk (incl. final padding when last)
    unsigned long long cap_bytes;    // capacity of the output buffer
    unsigned long long prior_bytes;  // stream bytes of this sequence that left in earlier buffers (final padding rule)
    uint32_t overflow;               // 1 = the chunk did not fit, nothing was written
    uint32_t pad;
};

constexpr int kSlotWords = 304;       // per-macroblock bit slot: 3 bit-contiguous segments, <= 9300 bits
constexpr int kSmallSlotWords = 32;   // macroblocks of <= 1024 stored bits (nearly all) use a compact 128-byte slot instead (64-byte slots were
                                      // tried: k_assemble touches half the lines for P frames, but most macroblocks of an I frame then sit in
                                      // the overflow slots, which it reads word by word - no net gain, profiles/archive/r02_v_bench.json)
constexpr int kSlotChunks = kSmallSlotWords / 4;
constexpr int kMicroSlotWords = 8;    // ... and those of <= 256 bits (the median P macroblock is 134 bits) a 32-byte slot in a third array
constexpr int kTinySlotWords = 16;    // ... and those of <= 512 bits (99 % of a P frame) a 64-byte slot in a second array behind the first:
                                      // k_assemble is bound by the cache lines it touches, two of these share one

struct MbAux {                        // 16 bytes per macroblock next to the uint32 info word
    uint32_t w0;                      // lenA | lenB << 16        (bits)
    uint32_t w1;                      // lenC | dcV  << 16
    uint32_t w2;                      // dcY00 | dcY11 << 16      (quantised DC levels, 16-bit two's complement)
    uint32_t w3;                      // dcU
};

// strip mode, peer transport (k_mb<.., EDGE, PEER>; m2v_comm.hpp PeerState): the strip's whole GOP step is ONE launch whose first
// n_edge blocks are the strip's first and last macroblock row.  They store their outer rows of the reconstruction straight into
// the NEIGHBOURS' landing buffers (the launch's halo_up / halo_down: peer or IPC-mapped memory) with write-through stores, then add
// one to the neighbour's arrival counter of their GOP; before they read the rows the neighbours delivered in the previous step (nb_up /
// nb_down: this rank's own landing buffers) they wait - bounded - until this rank's own counter of the GOP has reached
// (frame's index in the GOP) x (macroblocks per row): every block of the neighbour's edge row, of every earlier frame of this GOP.
// One counter per GOP of the sequence (= position in the step's halo list) and side, kPeerCntStride words apart: a thousand
// wavefronts asking for ONE word at the start of a launch are served one after the other (~12 ns each, measured: 36 us per step).
constexpr int kPeerSlots = 256;            // GOPs of one sequence the peer form can count (more: the ordinary exchange)
constexpr int kPeerCntStride = 64;         // uint32 words between the counters of consecutive GOPs: [slot][side], 128 bytes each
struct PeerStep {
    unsigned int *cnt_up, *cnt_down;            // the neighbours' arrival counters of GOP 0 (the one this rank's top row / bottom row adds to)
    const unsigned int *seen_up, *seen_down;    // own arrival counters of GOP 0: edge blocks of the rank above / below that have delivered
    unsigned int *gaveup;                       // own word: set when a wait ran out of budget (the sequence is then encoded again, exchanged the ordinary way)
    unsigned int budget;                        // bound of one wait, in 10 ns ticks of the 100 MHz wall clock
    unsigned int n_edge;                        // blocks [0, n_edge) of the launch are the edge rows, the others the rows in between
};

// strip mode: final assembly on the output rank (k_strip_layout / k_strip_assemble)
struct CopySeg { const uint8_t *src; unsigned long long dst_off; unsigned long long len; };
struct StripSrc { const uint8_t *strip[16]; };            // by value: the strips' device pointers (<= kMaxStripRanks)
constexpr int kMaxStripRanks = 16;

constexpr uint32_t kSeqHeaderBytes = 34;   // 269 bits + alignment (RTL:2598-2617)
constexpr uint32_t kGopHeaderBytes = 8;    // 59 bits + alignment  (RTL:2650-2656)

#ifdef __HIPCC__
#define M2V_HD __host__ __device__
#else
#define M2V_HD
#endif

// What the stream says about itself (m2v_set_stream_desc, m2v_desc.hip), as the header writers take it: a by-value kernel argument.
// The module's stream is the writers with seq_desc_module().
struct SeqDesc {
    uint32_t a;         // frame_rate_code | aspect_ratio_information << 4 | video_format << 8 | repeat_headers << 11 | vbv_buffer_size (18 bits) << 12
    uint32_t bit_rate;  // 30 bits, units of 400 bit/s
    uint32_t colour;    // colour_primaries | transfer_characteristics << 8 | matrix_coefficients << 16
    uint32_t display;   // display width | height << 16; 0 = the size sequence_header prints
    M2V_HD uint32_t rate_code() const { return a & 15u; }
    M2V_HD uint32_t aspect() const { return (a >> 4) & 15u; }
    M2V_HD uint32_t video_format() const { return (a >> 8) & 7u; }
    M2V_HD uint32_t repeat() const { return (a >> 11) & 1u; }
    M2V_HD uint32_t vbv() const { return a >> 12; }
};
constexpr SeqDesc seq_desc_module() { return SeqDesc{2u | 1u << 4 | 1u << 8, 10000u, 5u | 5u << 8 | 5u << 16, 0u}; }   // RTL:2598-2617

// frames per second the time code counts at for frame_rate_code 1..8 (table 6-4, rounded up: no drop-frame counting)
M2V_HD inline uint32_t time_code_rate(uint32_t code) { return (uint32_t)(0x3C3C321E1E191818ull >> (8u * ((code - 1u) & 7u))) & 0xFFu; }
// The 32 bits behind the group_start_code for a GOP whose I picture is frame n, counted at F frames per second: the module's formula
// (RTL:2685-2698) with its 24 replaced by F.  The six bits in front - drop_frame_flag and hours - hold min(n / 3600F, 63): the module's
// saturation, and its spill into drop_frame_flag from 32 hours on.  Then marker, seconds, pictures, closed_gop = 1, broken_link = 0.
// The one definition: write_frame_headers prints it, m2v_time_code exports it.
M2V_HD inline uint32_t time_code(uint32_t F, uint32_t n)
{
    const uint32_t hh = n / (3600u * F);
    return (hh > 63u ? 63u : hh) << 26 | ((n / (60u * F)) % 60u) << 20 | 1u << 19 | ((n / F) % 60u) << 13 | (n % F) << 7 | 2u << 5;
}

}  // namespace m2v
