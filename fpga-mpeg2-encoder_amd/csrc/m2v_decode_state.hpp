// m2v_decode_state.hpp — what the translation units of the decoder share on the host side: the call's state and picture table on the
// device (m2v_decode.hip: the module syntax and everything syntax-blind), every option's picture table and the plan / chunk functions
// m2v_decode.hip dispatches to (m2v_decode_main.hip, _b, _i, _x, _f, _j), and - at the end - the batch entries' table of streams with
// the launchers of their one scan and of the main-syntax batch entries' first pass, output kernel and report.  The device code the units
// share is m2v_decode_device.hpp's, the chunk schedule m2v_decode_chunks.hpp's; a kernel lives in one unit and is launched from there.
#pragma once
#include <functional>
#include "m2v_host.hpp"
#include "m2v_decode_kernels.hpp"
#include "m2v_decode_device.hpp"
#include "m2v_decode_chunks.hpp"

namespace m2v {

constexpr int kDecThreads = 256;

struct DecState {
    unsigned long long err, last_nz;               // the earliest error's offset (dec::kNone: none); one past the last byte that is not zero
    uint32_t nev, ev_cap;
    int32_t status;
    uint32_t npics, gops, reps, chains, width, height, mbw, mbh, pad;
    unsigned long long frame_bytes;
    // option "decode_conceal" (m2v_decode_c.hip), summed over the chunks: the first damaged picture's start code (dec::kNone: none), the
    // slices that did not read, the rows concealed, those of them without a frame in front, the pictures with such a row
    unsigned long long c_first;
    uint32_t c_bad, c_rows, c_grey, c_pics;
};
struct DecPic { uint32_t ev, type, chain, step; };

// the main syntax's share of the call's state (e->d_dec_main): the two matrices, raster order, then one entry per picture
constexpr size_t kDecMainMatrices = 128;
struct DecMainPic { uint32_t slice0, params; };    // the event of the picture's first slice; dec::params_pack of its coding extension

// m2v_decode_main.hip: the main-syntax variants of k_dec_plan, k_dec_slices and k_dec_recon, launched where decode_impl launches those
void dec_main_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                   unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main);
void dec_main_slices(hipStream_t s, unsigned blocks, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, const DecPic *pics, const uint8_t *d_main,
                     uint32_t p0, uint32_t np, dec::MbRec *mb, int32_t *dc, int16_t *lv);
void dec_main_recon(hipStream_t s, unsigned mbs, unsigned count, const DecState *st, const uint32_t *list, uint32_t p0, const uint8_t *d_main, const dec::MbRec *mb,
                    const int32_t *dc, const int16_t *lv, uint8_t *buf, size_t psz);

// B pictures (option "decode_b_pictures"; m2v_decode_b.hip): the table behind the matrices holds these instead of DecMainPic - the
// picture's display index and the coded indices of its references (a P picture: fwd; a B picture: fwd and bwd; 0xFFFFFFFF: none)
struct DecBPic { uint32_t slice0, params, display, fwd, bwd; };      // params: dec::bp_params_pack

// m2v_decode_b.hip: the plan in k_dm_plan's place, and everything behind the plan's wait - the chunks with two carried anchors, the
// anchors step by step, the chunk's B pictures in one launch, the pictures placed at their display indices, the verdict
void dec_b_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main);
void dec_b_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t B, const uint8_t *types,
                  uint32_t *h_list, m2v_decode_stat *h_rec);

// Interlaced frame pictures (option "decode_interlaced"; m2v_decode_i.hip), with "decode_b_pictures" (b_pictures) 0 or 1: DecBPic again,
// its params dec::il_params_pack.  The plan also leaves the picture's macroblock rows at h_mbh (pinned): a sequence that is not
// progressive has 2 * ((height + 31) / 32) of them, and the chunks take them from there
void dec_i_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, uint32_t *h_mbh);
void dec_i_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t mbh, size_t B,
                  const uint8_t *types, uint32_t *h_list, m2v_decode_stat *h_rec);

// Several slices a row, slice header extras, quant_matrix_extension, composite_display_flag 1 (option "decode_extended";
// m2v_decode_x.hip), with "decode_b_pictures" and "decode_interlaced" 0 or 1 each: the table behind the matrices holds DecBPic's fields,
// then the slice table - the picture's slices are the events [slice0, slice0 + nslices), sbase of them lie in front of it in the stream -
// and the events whose quant_matrix_extension loaded the intra / non-intra matrix in force (0xFFFFFFFF: the sequence's).  The plan leaves
// h_sl[p] = sbase of picture p and h_sl[pictures] = all slices (pinned): a chunk's slice walk is launched over its slices.  e->d_dec_x
// holds the matrix table (128 bytes a picture) and the spans of the chunk's slices
struct DecXPic { uint32_t slice0, params, display, fwd, bwd, nslices, sbase, mi, mn; };      // params: dec::il_params_pack

// tools: Table B-15, concealment motion vectors, dual prime (option "decode_mb_tools" on top of "decode_extended").  The plan is then
// dec_t_plan (m2v_decode_t.hip) with the same tables: DecXPic::params carries dec::t_params_pack's three flags above bit 20, and a P
// picture's bwd is its fwd - a dual-prime macroblock's second prediction reads the same reference
void dec_x_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int interlaced, uint32_t *h_mbh, uint32_t *h_sl);
void dec_t_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int interlaced, uint32_t *h_mbh, uint32_t *h_sl);
void dec_x_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t mbh, size_t B,
                  const uint8_t *types, bool tools, uint32_t *h_list, const uint32_t *h_sl, m2v_decode_stat *h_rec);

// Field pictures (option "decode_field_pictures" on top of "decode_interlaced", "decode_extended" and "decode_mb_tools";
// m2v_decode_f.hip): the table behind the matrices holds one DecFPic a CODED PICTURE - a frame picture or one field -, DecXPic's fields
// with display, fwd and bwd counted in FRAMES, and the picture's frame.  params: dec::fp_params_pack (the structure, "second field of its
// frame" and "no field of its own parity in front" above bit 23).  The record counts frames; the plan leaves the coded pictures at
// h_mbh[1], every coded picture's type | structure << 2 | second << 4 at h_types and the slices in front of it at h_sl.  A chunk is B
// whole frames
struct DecFPic { uint32_t slice0, params, display, fwd, bwd, nslices, sbase, mi, mn, frame; };

void dec_f_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, uint32_t *h_mbh, uint32_t *h_sl);
// h_conceal: nullptr, or (option "decode_conceal") where the report goes with the record - the walk and the verdict per row are then
// dec_c_walk's, an I picture is a step behind the anchor frame in front of it, and the last kernel is dec_c_finish's
void dec_f_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t mbh, size_t B,
                  const uint8_t *types, size_t ncp, uint32_t *h_list, const uint32_t *h_sl, m2v_decode_stat *h_rec, uint32_t *h_conceal = nullptr);
// the first record of coded picture Q in a chunk that begins at frame f0: a frame's stretch is mbs records, a second field's half of it
// lies behind its first field's
__device__ inline size_t df_first(const DecFPic &Q, uint32_t f0, uint32_t mbs) { return (size_t)(Q.frame - f0) * mbs + (((Q.params >> 26) & 1u) ? mbs / 2u : 0u); }

// Streams cut from a broadcast (option "decode_join" on top of "decode_field_pictures" and what it stands on; m2v_decode_j.hip): the
// plan alone, in dec_f_plan's place, with its tables and for dec_f_chunks.  The pictures it drops are in no table, the kept pictures'
// events keep their indices into the event list.  It leaves the join record behind the coded pictures: h_mbh[2 .. 7] = join_offset,
// tail_offset (low word first), dropped_leading, dropped_trailing
constexpr size_t kDecPlanWords = 96;               // the plan's words (h_mbh) in the pinned block, behind the record; the types begin at 128
constexpr uint32_t kDecJoinWord = 2;               // h_mbh[kDecJoinWord .. kDecJoinWord + 6): the join record
static_assert(kDecPlanWords + 4 * (kDecJoinWord + 6) <= 128, "the join record ends where the types begin");
void dec_j_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int join, uint32_t *h_mbh, uint32_t *h_sl);

// Damaged slices (option "decode_conceal" on top of "decode_field_pictures" and what it stands on, "decode_join" 0 .. 3;
// m2v_decode_c.hip).  The plan is k_dj_plan's text with the relaxed rules (dec_c_plan, k_dc_plan: a picture may have no slice,
// so the picture tables hold a picture per two events); the chunks stay dec_f_chunks, which hands the walk of a chunk's slices and
// the verdict per macroblock row to dec_c_walk - k_dc_slices refuses nothing, k_dc_rows writes the records of the concealed rows and
// sums the report in DecState - and the end to dec_c_finish, which leaves the report (kDecConcealWords words: first_offset low, high,
// bad_slices, concealed_rows, grey_rows, damaged_pictures) in pinned memory beside the record
constexpr size_t kDecConcealWords = 6;
void dec_c_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int join, uint32_t *h_mbh, uint32_t *h_sl);
void dec_c_walk(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, const DecPic *pics, const DecFPic *xp, uint32_t p0, uint32_t np,
                uint32_t f0, uint32_t total, dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *spans);
void dec_c_finish(hipStream_t s, const DecState *st, m2v_decode_stat *h_rec, uint32_t *h_conceal);

// The batch entries (m2v_decode_streams.hip, m2v_decode_streams_main.hip, m2v_decode_streams_ex.hip): the table of streams, a stream's
// state on the device and its verdict in pinned memory are the same for all three, and so are the kernels that do not read the syntax.
// They live in m2v_decode_streams.hip
struct DsIn { unsigned long long off, n, ev_base, pic_base; uint32_t tile0, ntiles, ev_cap, pic_cap; };
struct DsState { unsigned long long err, last_nz; uint32_t nev; int32_t status; uint32_t mbw, mbh; };
struct DsVerdict { unsigned long long err; int32_t status; uint32_t pad; };

inline size_t ds_up64(size_t v) { return (v + 63) & ~(size_t)63; }
// the counts of every tile, the prefix sum per stream, the events (k_ds_scan<false>, k_ds_tiles, k_ds_scan<true>); tiles 0: nothing
void ds_scan(hipStream_t s, const uint8_t *es, const DsIn *d_in, size_t n, size_t tiles, DsState *d_st, uint32_t *d_tiles, unsigned long long *d_ev);
void ds_judge(hipStream_t s, DsState *d_st, size_t n);                                  // k_ds_judge, a lane per stream
void ds_finish(hipStream_t s, const DsState *d_st, size_t n, DsVerdict *h_v);           // k_ds_finish
// every stream's record into e->ds_q; v: the verdicts behind the last chunk, or nullptr where nothing was decoded
void ds_report(m2v_enc *e, const uint64_t *off, size_t n, const std::vector<uint64_t> &out_offset, const std::vector<uint8_t> &overflow,
               const std::vector<m2v_decode_stat> &rec, const DsVerdict *v);

// The two main-syntax batch entries share their first pass and their output kernel (m2v_decode_streams_main.hip).  ds_main_first: the
// layout of e->h_ds, the limits (`entry` names the caller in the messages), the uploads, the scan, the unit's plan kernel through `plan`,
// the call's one wait, and the second run where a stream's event list was too small.  pic_bytes: a picture's entry in e->d_dec_pics;
// slices: the plan leaves every picture's slice events at h_sl (else h_sl is nullptr and nsl stays empty).  M2V_OK or M2V_E_PARAM
struct DsMainFirst { std::vector<m2v_decode_stat> rec; std::vector<uint8_t> types; std::vector<uint32_t> mbh, nsl; std::vector<size_t> pic_base; };
typedef std::function<void(const DsIn *d_in, DsState *d_st, uint8_t *h_types, uint32_t *h_sl, m2v_decode_stat *h_rec, uint32_t *h_mbh)> DsPlanLaunch;
int ds_main_first(m2v_enc *e, hipStream_t s, const char *entry, const uint8_t *es, const uint64_t *off, const uint64_t *bytes, size_t n, size_t pic_bytes,
                  bool slices, const DsPlanLaunch &plan, DsMainFirst &out);
namespace dec { struct MainChunkPic; }
// k_dsm_out over the `count` pictures of the chunk's table, 65535 a launch; most_units: the 16-byte units of its largest frame
void dsm_out(hipStream_t s, const DsState *d_st, const dec::MainChunkPic *tab, size_t count, uint32_t most_units, const uint8_t *buf, uint8_t *dst, int layout);

}  // namespace m2v
