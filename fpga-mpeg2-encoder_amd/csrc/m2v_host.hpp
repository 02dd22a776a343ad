// m2v_host.hpp — internals shared by the host translation units of libm2v_mi355x.so (not installed; the ABI is include/m2v_mi355x.h).
//
//   m2v_launch.hip    the ONLY unit that includes the device code (m2v_kernels.hpp): constant-table upload and one plain C++ launch
//                     function per kernel (device globals live in the code object of the unit that defines them, so every launch
//                     has to come from there)
//   m2v_core.hip      handle life cycle, options, geometry (RTL:985-1006), the chunk plan (GOP segments, reconstruction slots, launch
//                     lists) and its execution: plan_chunk -> run_step* -> finish_chunk
//   m2v_port.hip      the port path: beats in (RTL:1027-1095), 32-byte words out (RTL:2961-2994), double-buffered staging; the input
//                     conversions in front of a chunk (k_unpack444, k_fit, k_expand420, k_rgb2yuv: no device globals, so they can live here)
//   m2v_resident.hip  whole sequences resident in HBM (what bench.py times), one or several per call
//   m2v_strips.hip    strip mode (BASELINE config c5) and the communicators of m2v_comm.hpp
//   m2v_begin.hip     where a sequence starts, for every entry: what may run with what (begin_refusal), what the sequence samples from
//                     the settings (begin_sequence: all of m2v_enc::seq, nowhere else), and the records' way from a chunk or a call to
//                     the queues the report functions pop (collect_chunk, collect_call, drop_records)
//   m2v_gop.hip       a level per GOP: the caller's schedule (m2v_set_gop_levels) and option "gop_bytes_max", the byte cap the device judges
//                     (k_gop_judge, m2v_gop_kernels.hpp, launched from m2v_launch.hip) and the host's redo loop; m2v_gop_report
//   m2v_scene.hip     where GOPs start: the rule (gop_layout_run, m2v_gop_layout), the caller's list (m2v_set_gop_starts), option
//                     "scene_cut" - the detector's buffers, its launches (k_mbsum, k_scene_judge, m2v_scene_kernels.hpp, launched from
//                     m2v_launch.hip) and the host's one wait per chunk - and m2v_scene_report
//   m2v_stats.hip     option "stats": the per-picture records of m2v_picture_stats - their buffers and their way to the host (the
//                     kernels that fill them, m2v_stats_kernels.hpp, need m2v_kernels.hpp and so belong to m2v_launch.hip)
//   m2v_desc.hip      m2v_set_stream_desc: what the stream says about itself - the setting, its validation, its packed form (the SeqDesc
//                     the header writers of m2v_kernels.hpp take by value) - and the plain arithmetic of m2v_frame_rate_code and
//                     m2v_time_code
//   m2v_recon.hip     m2v_set_recon_out: the setting and the size of a frame in the caller's buffer (the kernel, m2v_recon_kernels.hpp,
//                     is launched from m2v_launch.hip)
//   m2v_sequences.hip m2v_set_sequences: a batch of sequences in one resident call - the setting, what the host knows of a batch's
//                     records when the call starts, and m2v_sequence_report (the scan that places the streams, k_seq_scan in
//                     m2v_seq_kernels.hpp, is launched from m2v_launch.hip)
//   m2v_mux.hip       m2v_set_mux_out / m2v_mux_device: transport or program stream out of the stream in HBM.  Its three kernels touch no
//                     device global and nothing of m2v_kernels.hpp, so they live in their own unit with their launches (m2v_mux_kernels.hpp
//                     holds the arithmetic, for the device and the host alike)
//   m2v_decode.hip    m2v_decode_device: an elementary stream in HBM back to 4:2:0 frames.  Its kernels touch no device global and nothing of
//                     m2v_kernels.hpp, so they live in their own unit with their launches (m2v_decode_kernels.hpp holds the arithmetic, for
//                     the device and the host alike)
//   m2v_decode_main.hip, m2v_decode_b.hip, m2v_decode_i.hip, m2v_decode_x.hip, m2v_decode_t.hip, m2v_decode_f.hip, m2v_decode_j.hip, m2v_decode_c.hip   m2v_decode_device's other syntaxes:
//                     the main syntax (option "decode_syntax"), B pictures on top of it (option "decode_b_pictures"), interlaced frame
//                     pictures (option "decode_interlaced"), several slices a row, slice header extras and quant_matrix_extension (option
//                     "decode_extended") with Table B-15, concealment motion vectors and dual prime (option "decode_mb_tools": a template
//                     flag of m2v_decode_x.hip's slice walk; m2v_decode_t.hip holds its plan alone), field pictures, two a frame (option
//                     "decode_field_pictures"), the plan for streams cut from a broadcast (option "decode_join"), and damaged slices concealed (option "decode_conceal").  A unit holds what
//                     its option changes - the plan, the slice walk, where a record, its weights and its slots come from.  What the
//                     units have in common exists once: m2v_decode_state.hpp (the call's state, the tables, every launcher),
//                     m2v_decode_device.hpp (the dec::IMb sink, the reconstruction of a macroblock, the output loop, slot) and
//                     m2v_decode_chunks.hpp (the chunk schedule, plain C++)
//   m2v_decode_streams.hip   m2v_decode_streams_device: a batch of elementary streams of any sizes in one call - the same arithmetic over a
//                     table of streams (m2v_decode_streams.hpp lays the batch out, for the host build too).  Its scan, judge, finish and
//                     report serve all three batch entries (m2v_decode_state.hpp declares their launchers)
//   m2v_decode_streams_main.hip   m2v_decode_streams_main_device: the same for main-syntax streams, B pictures and interlaced frame pictures
//                     by the call's flags (m2v_decode_streams_main.hpp lays the batch out); its first pass and its output kernel serve
//                     m2v_decode_streams_ex.hip (m2v_decode_streams_main_ex_device: the extended options by the call's flags) too
//   m2v_demux.hip     m2v_demux_device: transport / program streams in HBM back to the elementary stream, the inverse of m2v_mux.hip and like it
//                     a unit of its own (m2v_demux_kernels.hpp holds the arithmetic, for the device and the host alike)
//   m2v_scale.hip     m2v_set_source_size: frames of another size resampled to the picture size in front of the conversions - the setting,
//                     the tap tables (m2v_scale_taps), k_scale and its launch (m2v_scale_kernels.hpp holds the arithmetic, for the device
//                     and the host alike; no device global, nothing of m2v_kernels.hpp)
//   m2v_deint.hip     m2v_deinterlace_device: woven 4:2:0 frames in HBM to progressive frames, behind the decoder and in front of an encode -
//                     the entry, k_deint and its launch (m2v_deint_kernels.hpp holds the arithmetic, for the device and the host alike; no
//                     device global, nothing of m2v_kernels.hpp, no state on the handle)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/m2v_mi355x.h"
#include "m2v_types.hpp"

namespace m2v {

struct HipError { hipError_t e; const char *what; };

#define HIPCHK(expr)                                                        \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) throw ::m2v::HipError{_e, #expr};             \
    } while (0)


// Bumped whenever device or pinned memory of any handle is (re)allocated or freed: a recorded hipGraph holds raw pointers, and a
// graph recorded under an older generation is recorded again instead of launched (m2v_strip_encode).
inline std::atomic<unsigned long long> &alloc_generation()
{
    static std::atomic<unsigned long long> gen{0};
    return gen;
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    bool recorded = true;       // false: no recorded graph ever references this buffer (its reallocation invalidates none)
    void ensure(size_t count)
    {
        if (count <= n) return;
        if (recorded) ++alloc_generation();
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        HIPCHK(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
    }
    void release() { if (p) { if (recorded) ++alloc_generation(); (void)hipFree(p); } p = nullptr; n = 0; }
};

// Records waiting for a report function (m2v_picture_stats, m2v_gop_report, ...): oldest first
template <typename T>
struct Records {
    std::deque<T> q;
    void push(const T *first, const T *last) { q.insert(q.end(), first, last); }
    void clear() { q.clear(); }
    // up to max records into out, which leave the queue; out == nullptr: how many are waiting
    size_t pop(T *out, size_t max)
    {
        if (!out) return q.size();
        const size_t n = std::min(max, q.size());
        std::copy(q.begin(), q.begin() + (std::ptrdiff_t)n, out);
        q.erase(q.begin(), q.begin() + (std::ptrdiff_t)n);
        return n;
    }
    // ... for the report functions that answer an int
    int pop31(T *out, size_t max) { return (int)std::min<size_t>(pop(out, std::min<size_t>(max, 0x7FFFFFFF)), 0x7FFFFFFF); }
};

struct KStat { int launches = 0; double ms = 0, units = 0; };
struct SrcSize { int w = 0, h = 0; };       // pixels of a source frame; 0 x 0: the frames are W x H

struct StripFlight;


struct TimedLaunch { hipEvent_t a, b; int kernel; double units; int count; };

}  // namespace m2v

using namespace m2v;      // (an internal header: every unit that includes it is part of the library)

struct m2v_enc {
    // module parameters (RTL:11-14)
    int XL, YL, VL, Q;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // options
    size_t batch_frames = 96;
    bool profile = false;
    bool inject_strip_failure = false;  // debug: a strip encode fails on this rank after the collective set-up (option "inject_strip_failure")
    bool keep_recon = false;      // debug: every frame keeps its own reconstruction buffer, levels are dumped

    // sequence state (RTL:1017-1022)
    enum State { IDLE, DURING, ENDED } state = IDLE;
    Geom g{};
    uint32_t pframes = 0;
    size_t frames_total = 0;      // frames of this sequence handed to the GPU so far
    bool first_chunk = true;

    // Host staging, double buffered: while the GPU works on the chunk submitted from one stage the caller
    // fills the other one.  Each stage owns everything the host and the device touch asynchronously:
    // the pinned frames, the pinned launch plan, the control read-back, the chunk's stream buffer.
    struct HostStage {
        uint8_t *h_in = nullptr;              // pinned planar 4:4:4 frames of the chunk being filled
        size_t h_in_cap = 0;                  // bytes
        StreamCtl *h_ctl = nullptr;           // pinned: [0] read-back, [1] initial values
        FrameJob *h_jobs = nullptr;           // pinned staging of the per-frame jobs
        size_t h_jobs_cap = 0;
        FrameJob *h_joblist = nullptr;        // pinned staging of the jobs in launch-list order
        int *h_lists = nullptr;               // pinned staging of the launch lists
        size_t h_lists_cap = 0;
        uint8_t *h_out = nullptr;             // pinned read-back buffer
        size_t h_out_cap = 0;
        DevBuf<uint8_t> d_in;                 // the chunk's frames on the device: the upload of chunk k+1 (up_stream) runs
                                              // while the kernels of chunk k read the other stage's buffer
        DevBuf<uint8_t> d_out;                // chunk output when it goes to the host
        // Frames that arrived as PACKED 4:4:4 samples (m2v_push_packed) keep the caller's byte order until they are on the device: one
        // linear run of bytes per chunk, frame after frame in arrival order, staged in pinned memory (or uploaded straight from
        // page-locked caller memory) and de-interleaved into d_in by k_unpack444 in front of the chunk's kernels
        // Whole 4:2:0 frames (m2v_push_frames420) are one more kind of run in the same bytes: kPk420 + M2V_420_*, expanded by k_expand420;
        // whole RGB frames (m2v_push_rgb) another: pk_rgb(M2V_RGB_* layout, matrix), converted by k_rgb2yuv.  While the sequence pads its
        // frames (m2v_set_frame_size) every run holds frames of the SOURCE size, k_fit runs in front of the conversion, and whole planar
        // 4:4:4 frames are a run kind too: kPk444
        struct PkFrame { uint32_t frame; int layout; size_t off; };       // chunk frame index, M2V_PACKED_* / kPk420 + M2V_420_* / pk_rgb(), where its bytes start in h_pk / d_pk
        std::vector<PkFrame> pk;
        uint8_t *h_pk = nullptr;              // pinned staging (only when packed beats come from ordinary memory)
        size_t h_pk_cap = 0;
        DevBuf<uint8_t> d_pk;
        size_t pk_used = 0;                   // bytes reserved for the packed frames of the chunk being filled (whole frames)
        size_t pk_valid = 0;                  // ... of which the caller has delivered this many (the frame in progress ends here)
        size_t pk_up = 0;                     // ... of which this many are on the device (or on their way) already
        hipEvent_t ev_ctl = nullptr, ev_out = nullptr, ev_up = nullptr;
        size_t uploaded = 0;                  // leading frames of the chunk being filled that are already in d_in (page-locked
                                              // caller memory goes to the device directly, without the pinned staging copy)
        m2v_picture_stat *h_pstat = nullptr;  // pinned: the chunk's picture records (option "stats"), read back in front of the control word
        size_t h_pstat_cap = 0;
        size_t nstat = 0;                     // records of the submitted chunk that collect_chunk has not moved to the handle's queue yet
        m2v_gop_stat *h_gop = nullptr;        // pinned: the chunk's GOP records (option "gop_bytes_max"), written by k_gop_judge itself
        size_t h_gop_cap = 0;
        size_t ngop = 0;                      // records of the submitted chunk that collect_chunk has not moved to the handle's queue yet
        std::vector<m2v_scene_stat> scene;    // the submitted chunk's records of m2v_scene_report (plan_chunk makes them on the host)
        int stage = 0;                        // 0 free, 1 encode submitted, 2 stream read-back submitted
        bool last = false;
        size_t bytes = 0;
    } hs[2];
    int cur = 0;                  // stage being filled by m2v_push_*
    HostStage &st() { return hs[cur]; }
    std::deque<int> pending;      // submitted stages, oldest first
    int cu_pack = 5;              // option "cu_pack": log2 of the CUs an XCD deals its workgroups to in turn (xcd_remap; 0 = plain XCD remap)
    bool dct_mfma = true;         // option "dct_mfma": luma DCT through the matrix cores (k_mb<.., MFMA = true>); 0 = integer VALU / LDS
                                  // path.  Same results; kept by the rocprofv3 number (profiles/archive/r02_mfma_*: 138.3 vs 140.3 us per launch)
    bool conformant = false;      // option "conformant": ISO reconstruction loop instead of the RTL's (NOT byte-identical to the reference)
    int copy_threads = 8;         // option "copy_threads": threads that copy m2v_push_frames input into pinned memory
    bool direct_upload = true;    // option "direct_upload": page-locked caller memory is uploaded without the staging copy
    bool direct_upload_deferred = false;   // ... = 2: and m2v_push_frames returns while its frames are still being read (see include/m2v_mi355x.h)
    hipEvent_t ev_upl[2] = {nullptr, nullptr}, ev_up2 = nullptr;
    bool upl_pending[2] = {false, false};
    int up_parity = 0;
    // Blocking m2v_push_frames from page-locked memory: the chunk's kernels wait for the upload through an event WITHOUT system fence, and
    // the call waits for that event itself (not for the upload stream) - m2v_port.hip, flush_buffered
    bool up_unsynced = false;            // a direct upload has been issued and not yet waited for on the host
    hipEvent_t up_wait_ev = nullptr;     // the event behind the LAST transfer issued on the upload stream, if one was recorded there (else: wait for the stream)
    void *call_sink = nullptr;           // m2v_push_frames_pull: the call's destination (a PullSink), seen by every progress() inside the call
    int split_streams = 2;        // GOP segments of a chunk run as this many independent groups on as many streams (encode_chunk)
    static constexpr int kMaxSplit = 8;
    hipStream_t side[kMaxSplit - 1] = {};            // group 0 runs on the caller's stream
    hipEvent_t ev_fork = nullptr, ev_join[kMaxSplit - 1] = {};
    hipStream_t up_stream = nullptr;     // host -> device uploads of the port path
    hipStream_t up_stream2 = nullptr;    // ... the second one of option direct_upload = 2
    bool async = true;            // option "async": 0 = every chunk is completed before m2v_push_* returns
    hipStream_t copy_stream = nullptr;   // stream read-back, concurrent with the next chunk's kernels
    size_t buffered = 0;          // complete frames waiting in st().h_in
    size_t beat_pos = 0;          // beats received of the frame in progress
    int cur_kind = 0;             // the form the frame in progress is kept in (that of its first beats): 0 = three planes in h_in, 1 + layout = packed
    size_t cur_pk_off = 0;        // ... a packed one: where it starts in the stage's packed bytes
    uint32_t last_frame_valid_beats = 0;   // for a black-filled last frame

    // host output FIFO (32-byte words are handed out by m2v_pull)
    std::vector<uint8_t> fifo;
    size_t fifo_rd = 0;
    bool end_pending = false;     // the data in the FIFO ends with the o_last word

    // device buffers
    DevBuf<int16_t> d_coef;               // debug only: quantised levels
    DevBuf<MbAux> d_mbaux;
    DevBuf<uint32_t> d_slots;             // per-macroblock VLC bit segments (kSlotWords each), used on overflow only
    DevBuf<uint32_t> d_slots_small;       // compact 128-byte slots (kSmallSlotWords each): the common case
    DevBuf<uint32_t> d_mbinfo, d_mblen, d_slice_bytes;
    DevBuf<unsigned long long> d_slice_off, d_frame_off;
    DevBuf<FrameJob> d_jobs;
    DevBuf<int> d_lists;
    DevBuf<FrameJob> d_joblist;           // the jobs again, in launch-list order (k_mb reads its frame's job with ONE dependent scalar load)
    // block -> macroblock tables of the k_mb launches (MbMap), one per launch shape seen, built by the launch functions (m2v_launch.hip)
    struct MbMapKey { int row0, row1, mbw, mbh, cu_pack, mode, rstride, n_edge; };
    struct MbMapCache { MbMapKey key; DevBuf<MbMap> d; hipStream_t filled_on = nullptr; hipEvent_t ev = nullptr; std::vector<hipStream_t> waited; };
    std::deque<MbMapCache> mbmaps;
    DevBuf<StreamCtl> d_ctl;
    int ctl_init = 0;                     // how the next k_frame_scan sets the control word up (ctl_begin): 0 leaves it, 1 new stream, 2 continues
    unsigned long long ctl_cap = 0;
    // strip mode, peer transport: what the next k_frame_scan does about the give-up word and the next sequence's arrival counters (PeerScan)
    unsigned int *scan_peer_gaveup = nullptr, *scan_peer_clear = nullptr;
    int scan_peer_lines = 0;
    unsigned long long scan_peer_mark = 0;
    std::vector<uint8_t *> rec_pool;      // reconstruction buffers (4:2:0 planar), each ysz + 2*csz
    size_t rec_bytes = 0;
    size_t rec_pool_bytes = 0;            // allocation size of every buffer in rec_pool
    int persist_slot = -1;                // slot holding recon of the last encoded frame (GOP continues)
    unsigned long long stream_bytes = 0;  // bytes of the current sequence already moved to the FIFO

    // plan of the chunk being encoded (plan_chunk -> run_step* -> finish_chunk)
    struct Step { int off_i, n_i, off_p, n_p, off_h, n_h; int cut_i[kMaxSplit + 1], cut_p[kMaxSplit + 1]; };   // cut_*[k]: first list entry of segment group k
    // what d_jobs / d_lists / d_joblist hold: a caller that encodes sequence after sequence of one shape from the same buffers (the
    // resident entry in a loop) gets the same plan every time, and three small host-to-device copies in front of the first kernel
    // of every call are ~25 us of latency the GPU spends idle
    std::vector<FrameJob> dev_jobs;
    std::vector<int> dev_lists;
    const void *dev_jobs_p = nullptr, *dev_lists_p = nullptr, *dev_joblist_p = nullptr;
    int plan_groups = 1;                  // groups the launch lists of the current plan are cut into
    int plan_gf[kMaxSplit + 1] = {};      // chunk-frame index where each group's frames start (its GOP segments are consecutive frames)
    bool resident_inflight = false;       // between m2v_encode_resident_begin and m2v_encode_resident_end
    bool resident_empty = false;          // ... of a sequence without frames
    hipStream_t resident_stream = nullptr;
    bool slice_scan_done = false;         // the groups ran k_slice_scan on their own streams (encode_chunk): finish_chunk skips it
    std::vector<Step> plan_steps;
    size_t plan_nf = 0;
    bool strip_active = false;            // between m2v_strip_begin and m2v_strip_finish
    bool strip_inflight = false;          // between m2v_strip_encode_begin and m2v_strip_encode_end
    StripFlight *flight = nullptr;        // ... what the second half needs to know of the first (m2v_strips.hip)
    hipStream_t strip_stream = nullptr;
    DevBuf<uint8_t> d_segs;               // CopySeg table of the strip assembly (written by k_strip_layout)
    DevBuf<unsigned long long> d_frame_pos;   // where every frame's headers start in the assembled stream (k_strip_layout)
    DevBuf<unsigned long long> d_alloff;  // [ranks][frames + 1] frame offsets of every rank's strip
    uint8_t *h_asm = nullptr;             // pinned staging of the offsets (m2v_strip_assemble: up; m2v_strip_encode: the all-gathered sizes down)
    size_t h_asm_cap = 0;
    hipEvent_t ev_asm = nullptr;          // the staging may be rewritten once this has been reached
    uint8_t *h_strip = nullptr;           // pinned: this strip's frame offsets + control word (m2v_strip_finish_async -> m2v_strip_offsets)
    size_t h_strip_cap = 0;
    size_t strip_nf = 0;
    hipEvent_t ev_strip = nullptr;
    // m2v_strip_encode: the whole strip sequence in one call
    DevBuf<uint8_t> d_halo, d_strip_own, d_gather;      // (d_gather: sized from the other ranks' strips AFTER the host wait; no recording references it)
    hipStream_t comm_stream = nullptr;    // send / recv with the neighbours, beside the interior rows on the main stream
    hipEvent_t ev_edges = nullptr, ev_halo = nullptr, ev_interior = nullptr, ev_done = nullptr;
    // m2v_strip_encode as a recorded hipGraph (option "strip_graph"): everything one call enqueues before its one host wait
    struct StripGraph {
        hipGraphExec_t exec = nullptr;
        std::vector<unsigned long long> key;       // what the recording depends on (shape, ranks, buffers' generation)
        std::vector<unsigned long long> seen;      // the key of the previous call: a shape is recorded when it comes a second time
        bool broken = false;                       // recording failed once on this handle: not tried again
        int launches = 0, captures = 0;
    } strip_graph;
    // -1 = automatic: recorded with world == 1 and with the single-GPU timing communicators; call by call between the ranks of a real
    // RCCL job (a recording with cross-rank ncclSend / ncclRecv inside has never run on hardware: opt in with 1); 0 = never
    int strip_graph_opt = -1;
    struct StripStats { double halo_total_ms = 0, halo_exposed_ms = 0, gather_ms = 0, host_us_per_step = 0, comm_us_per_step = 0; int steps = 0; int graph = 0; int peer = 0; } strip_stats;

    // m2v_encode_resident420 / m2v_encode_resident_rgb: the chunk's frames as planar 4:4:4 in front of its kernels (no recording references the buffer)
    DevBuf<uint8_t> d_x444;
    size_t x444_bytes = 0;                // ... what the last call's last chunk left there (m2v_debug_read, what = 4)

    // What the setters write, on idle handles only, and what the sequence in progress runs with.  begin_sequence (m2v_begin.hip) decides
    // from `set` whether an entry may start and writes ALL of `seq`, for every entry: a setting the entry does not take samples as off.
    // Besides it only m2v_set_frame_size, m2v_set_source_size, m2v_set_recon_out and m2v_set_mux_out write `seq`: they clear what goes with
    // the old setting.
    // plan_chunk, the launch sites and the feature units read `seq` only.
    struct ReconDst { uint8_t *p = nullptr; size_t cap = 0; int layout = 0; size_t fb = 0; };      // fb (seq only): bytes of one frame in the caller's buffer
    struct MuxDst { int kind = 0; uint8_t *p = nullptr; size_t cap = 0; };
    struct Settings {
        SrcSize size;                           // m2v_set_frame_size (0 x 0 = off) ...
        int header = M2V_HEADER_MODULE;         // ... and what the headers say
        SrcSize src;                            // m2v_set_source_size (0 x 0 = off) ...
        int filter = M2V_SCALE_TRIANGLE;        // ... and its filter
        std::vector<uint8_t> gop_levels;        // m2v_set_gop_levels
        unsigned long long gop_bytes_max = 0;   // option "gop_bytes_max"
        std::vector<uint32_t> gop_starts;       // m2v_set_gop_starts
        uint32_t scene_cut = 0;                 // option "scene_cut"
        m2v_stream_desc desc{};                 // m2v_set_stream_desc ...
        bool desc_set = false;                  // ... and whether it differs from the module's
        std::vector<uint32_t> sequences;        // m2v_set_sequences
        ReconDst recon;                         // m2v_set_recon_out (p == nullptr: off)
        MuxDst mux;                             // m2v_set_mux_out (kind 0: off)
    } set;
    struct Sampled {
        SrcSize fit;                            // the source size when the frames have to be padded (0 x 0 when not: no size set, or one of whole macroblocks)
        bool hdr_true = false;                  // the headers say it
        SrcSize src;                            // the source size when the frames have to be resampled (0 x 0 when not: none set, or the picture size) ...
        SrcSize pic;                            // ... the picture size they are resampled to, and the filter
        int filter = M2V_SCALE_TRIANGLE;
        std::vector<uint8_t> levels;            // empty: every GOP at Q
        unsigned long long cap = 0;             // 0: no cap
        std::vector<uint32_t> starts;           // empty and cut 0: the fixed cadence, nothing of m2v_scene.hip is touched
        uint32_t cut = 0;
        SeqDesc desc = seq_desc_module();       // launch_frame_scan and launch_assemble take it by value
        std::vector<uint32_t> lens;             // empty: one sequence, nothing of m2v_sequences.hip is touched
        ReconDst recon;
        MuxDst mux;
    } seq;

    DevBuf<uint8_t> d_fit;                // padded frames in their own format, between k_fit or k_scale and the conversion (no recording references it)
    // m2v_set_source_size (m2v_scale.hip): the four tap tables of the last scaled sequence on the device, their pinned source, and what
    // they were built for (source, picture, filter)
    DevBuf<uint8_t> d_scale_tab;
    uint8_t *h_scale_tab = nullptr;
    size_t h_scale_cap = 0;
    int scale_key[5] = {0, 0, 0, 0, 0};

    // option "stats" (m2v_stats.hip): the chunk's records on the device - k_picstat and k_picstat_mb fill them in place - and the
    // completed pictures' records nobody has popped yet
    bool stats_on = false;
    DevBuf<m2v_picture_stat> d_pstat;
    Records<m2v_picture_stat> pstat_q;

    // a level per GOP (m2v_gop.hip)
    std::vector<uint8_t> plan_list_q;     // the level of every entry of the plan's launch lists (the redo lists of the cap follow the plan's)
    size_t plan_nlists = 0;               // entries of the plan's own lists in d_lists / d_joblist
    DevBuf<m2v_gop_stat> d_gop;           // the chunk's GOP records on the device (k_gop_judge reads its own verdict of the previous try there)
    Records<m2v_gop_stat> gop_q;        // completed GOPs' records nobody has popped yet
    hipEvent_t ev_gop = nullptr;          // behind a k_gop_judge whose verdict the host needs
    uint8_t *h_redo = nullptr;            // pinned staging of the redo lists
    size_t h_redo_cap = 0;

    // where GOPs start (m2v_scene.hip)
    size_t gop_s = 0, gop_k = 0;          // the GOP in progress at frames_total: the frame number of its I picture, and its ordinal
    std::vector<uint8_t> chunk_cut;       // the detector's flag of every frame of the chunk about to be planned (scene_detect -> plan_chunk)
    std::vector<unsigned long long> chunk_diff;       // ... and D(n)
    Records<m2v_scene_stat> scene_q;    // completed pictures' records nobody has popped yet
    DevBuf<uint32_t> d_mbsum;             // [frame][mb] luma sums of the chunk
    DevBuf<uint32_t> d_carry;             // 2 x [mb]: the sums of the last frame of the previous chunk, and where this chunk leaves its own
    int carry_cur = -1;                   // which half holds the previous chunk's (-1: the sequence starts with this chunk)
    DevBuf<uint8_t> d_scene;              // SceneRec of every frame of the chunk
    uint8_t *h_scene = nullptr;           // pinned: the same records, written by k_scene_judge itself
    size_t h_scene_cap = 0;
    hipEvent_t ev_scene = nullptr;        // behind the k_scene_judge whose flags the host needs

    // a batch of sequences (m2v_sequences.hip).  seq_at / seq_f0: the sequence open at frames_total and the call frame it starts at,
    // carried across chunks; plan_seq0 / plan_nsq: the sequence of the planned chunk's first frame, and how many it touches
    size_t seq_at = 0, seq_f0 = 0, plan_seq0 = 0, plan_nsq = 0;
    size_t dev_base = 0;                  // frames_total of the plan d_joblist holds (a batch's copies there carry the CALL's frame number)
    DevBuf<m2v_sequence_stat> d_seq;      // the call's records on the device: offset and bytes of the open sequence travel from chunk to chunk here
    DevBuf<unsigned long long> d_seqtmp;  // k_seq_scan's raw starts and deltas of the chunk's sequences
    m2v_sequence_stat *h_seq = nullptr;   // pinned: the same records, written by k_seq_scan itself
    size_t h_seq_cap = 0;
    bool seq_pending = false;             // a batch is in flight or has just completed: its records have not moved to seq_q yet
    Records<m2v_sequence_stat> seq_q;   // the last call's records nobody has popped yet

    // a container out of the stream (m2v_mux.hip): the muxer's work buffers - the streams' state, their start-code events, the picture
    // tables; no recording references them - and the records: written into pinned memory by k_mux_plan itself, complete where the
    // control word is
    DevBuf<uint8_t> d_mux_st, d_mux_pic;
    DevBuf<unsigned long long> d_mux_ev;
    uint8_t *h_mux = nullptr;             // pinned: the streams' initial state on its way up, then the records
    size_t h_mux_cap = 0;
    size_t mux_n = 0;                     // streams of the last mux
    bool mux_pending = false;             // a resident call with a container is in flight: its records have not moved to mux_q yet
    Records<m2v_mux_stat> mux_q;        // the last mux's records nobody has popped yet

    // the decoder (m2v_decode.hip): its work buffers - state, tile counts, start-code events, picture table, the chunk's macroblock records,
    // DC values, levels and planar pictures, the launch lists; no recording references them - allocated by the first decode, and the
    // pinned memory the plan's record and picture types arrive in
    DevBuf<uint8_t> d_dec_st, d_dec_pics, d_dec_mb, d_dec_buf;
    DevBuf<uint32_t> d_dec_tiles, d_dec_list;
    DevBuf<unsigned long long> d_dec_ev;
    DevBuf<int32_t> d_dec_dc;
    DevBuf<int16_t> d_dec_lv;
    uint8_t *h_dec = nullptr;
    size_t h_dec_cap = 0;
    DevBuf<uint8_t> d_dec_main;           // the main syntax's share of the state (m2v_decode_state.hpp): the matrices and the pictures' parameters
    int decode_syntax = 0;                // option "decode_syntax": M2V_SYNTAX_MODULE / M2V_SYNTAX_MAIN
    int decode_b_pictures = 0;            // option "decode_b_pictures": B pictures on top of the main syntax, frames in display order (m2v_decode_b.hip)
    int decode_interlaced = 0;            // option "decode_interlaced": frame pictures with frame_pred_frame_dct 0 on top of the main syntax (m2v_decode_i.hip)
    int decode_extended = 0;              // option "decode_extended": several slices a row, slice extras, quant_matrix_extension on top of the main syntax (m2v_decode_x.hip)
    DevBuf<uint8_t> d_dec_x;              // its matrix table (128 bytes a picture) and the spans of a chunk's slices
    int decode_mb_tools = 0;              // option "decode_mb_tools": Table B-15, concealment vectors, dual prime on top of "decode_extended" (m2v_decode_t.hip: the plan; m2v_decode_x.hip: the rest)
    int decode_field_pictures = 0;        // option "decode_field_pictures": picture_structure 1 / 2, two fields a frame, on top of the three above it (m2v_decode_f.hip)
    int decode_join = 0;                  // option "decode_join": M2V_JOIN_HEAD | M2V_JOIN_TAIL on top of the four above it (m2v_decode_j.hip)
    m2v_decode_join dec_join{};           // the last call's join record (m2v_decode_join_report)
    int decode_conceal = 0;               // option "decode_conceal": damaged slices dropped, their rows concealed, on top of the four above "decode_join" (m2v_decode_c.hip)
    m2v_decode_conceal dec_conceal{};     // the last call's concealment report (m2v_decode_conceal_report)
    size_t decode_batch = 0;              // option "decode_batch": pictures per chunk (0: as many as keep the levels within 256 MiB, 256 at most)
    m2v_decode_stat dec_rec{};            // the last call's record (m2v_decode_report)
    // several streams per call (m2v_decode_streams.hip): the work buffers above serve it too; its own are the streams' table, the
    // chunks' tables, and the pinned memory for both and for the records - allocated by the first m2v_decode_streams_device
    DevBuf<uint8_t> d_ds_in, d_ds_tab;
    uint8_t *h_ds = nullptr, *h_ds_tab = nullptr;
    size_t h_ds_cap = 0, h_ds_tab_cap = 0;
    Records<m2v_decode_stream_stat> ds_q; // the last call's records nobody has popped yet

    // the demultiplexer (m2v_demux.hip): the containers' state, the tiles' sums, the tables of payload runs - no recording references
    // them - allocated by the first m2v_demux_device, and the pinned memory the state goes up and the records arrive in
    DevBuf<uint8_t> d_dmx_st, d_dmx_tiles, d_dmx_seg;
    uint8_t *h_dmx = nullptr;
    size_t h_dmx_cap = 0;
    Records<m2v_demux_stat> dmx_q;        // the last demux's records nobody has popped yet
    size_t demux_blocks = 0;              // option "demux_blocks": the most workgroups of one launch (0: 4096); what is left over goes round the kernels' loops

    // debug bookkeeping of the last resident encode
    size_t dbg_frames = 0;
    std::vector<int> dbg_rec_slot;

    // profiling
    KStat stats[7];
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> ev_pool;      // timing events, reused from step to step
    size_t ev_used = 0;
    hipEvent_t chain_ev = nullptr;        // stop event of the previous timer while nothing else was enqueued after it
    hipStream_t chain_stream = nullptr;
    // the timer that stopped last and has not recorded its stop event yet: consecutive launches of ONE kind on one stream are timed as
    // one interval (an event between two kernels costs the second one ~3 us: the eight P launches of a sequence read 110.8 us each with
    // an event in every gap and 107 under rocprofv3)
    struct { bool on = false; hipEvent_t a = nullptr; int kernel = 0; double units = 0; int count = 0; hipStream_t s = nullptr; } open_t;
    bool timer_merge = false;             // only where launches follow each other on one stream with nothing in between (encode_chunk's step loop)

    void set_err(const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
    }
};

namespace m2v {

// ---- m2v_core.hip ----
Geom make_geom(const m2v_enc *e, uint32_t xs, uint32_t ys);
hipEvent_t pool_event(m2v_enc *e);
void collect_timers(m2v_enc *e);
void plan_chunk(m2v_enc *e, hipStream_t s, const uint8_t *d_frames, size_t nf, bool last, uint32_t last_valid_beats);
void run_step(m2v_enc *e, hipStream_t s, size_t j);
void run_step_rows(m2v_enc *e, hipStream_t s, size_t j, int r0, int r1);
void run_step_edges_fused(m2v_enc *e, hipStream_t s, size_t j, uint8_t *up, uint8_t *down, const uint8_t *nb_up, const uint8_t *nb_down);
void run_step_peer(m2v_enc *e, hipStream_t s, size_t j, int group, uint8_t *put_up, uint8_t *put_down, const uint8_t *got_up, const uint8_t *got_down, PeerStep ps);
void finish_chunk(m2v_enc *e, hipStream_t s, bool first, bool last, uint8_t *d_stream, bool advance = false);
void encode_chunk(m2v_enc *e, hipStream_t s, const uint8_t *d_frames, size_t nf, bool first, bool last, uint32_t last_valid_beats,
                  uint8_t *d_stream, bool advance = false);
// pinned host memory of at least `bytes`, kept with the handle
void ensure_pinned(uint8_t *&p, size_t &cap, size_t bytes);
// every C-ABI entry runs its body through this: selects the handle's device, turns exceptions into M2V_E_* + the handle's error text
int guard(m2v_enc *e, int (*fn)(m2v_enc *, void *), void *arg);

// HIP-event timers of option "profile": events come from a pool that lives as long as the handle, and a timer
// that starts right where the previous one stopped (same stream, nothing enqueued in between) reuses that
// event, so a step of n back-to-back launches costs n + 1 event records and no create / destroy.
// closes the open timer: its stop event goes into its stream HERE (call it before anything untimed is enqueued there)
inline void timer_close(m2v_enc *e)
{
    if (!e->open_t.on) return;
    hipEvent_t b = pool_event(e);
    HIPCHK(hipEventRecord(b, e->open_t.s));
    e->timed.push_back(TimedLaunch{e->open_t.a, b, e->open_t.kernel, e->open_t.units, e->open_t.count});
    e->chain_ev = b;
    e->chain_stream = e->open_t.s;
    e->open_t.on = false;
}
// ... and the next timer records a start event of its own (untimed work follows)
inline void timer_break(m2v_enc *e)
{
    if (e->profile) timer_close(e);
    e->chain_ev = nullptr;
}

struct Timer {
    m2v_enc *e; hipStream_t s; int kernel; double units; hipEvent_t a = nullptr; bool merged = false;
    Timer(m2v_enc *e_, hipStream_t s_, int k, double u) : e(e_), s(s_), kernel(k), units(u)
    {
        if (e->profile) {
            if (e->open_t.on && e->open_t.kernel == kernel && e->open_t.s == s) { merged = true; return; }     // one more launch of the open interval
            timer_close(e);
            if (e->chain_ev && e->chain_stream == s) a = e->chain_ev;
            else { a = pool_event(e); HIPCHK(hipEventRecord(a, s)); }
            e->chain_ev = nullptr;
        }
    }
    void stop()
    {
        if (e->profile) {
            if (merged) { e->open_t.units += units; ++e->open_t.count; return; }
            e->open_t.on = true; e->open_t.a = a; e->open_t.kernel = kernel; e->open_t.units = units; e->open_t.count = 1; e->open_t.s = s;
            if (!e->timer_merge) timer_close(e);        // everywhere else the stop event follows its launch at once
        }
    }
};

// ---- m2v_begin.hip: where a sequence starts, and its records ----
// The entries that start something.  Beats: m2v_push_beats, m2v_push_packed; Frames: m2v_push_frames / 420 / rgb and their _pull forms;
// Resident: the six m2v_encode_resident* entries; Strip: m2v_strip_begin, m2v_strip_encode(_begin) and, for the rule alone, m2v_strip_assemble
enum class Entry { Beats, Frames, Resident, Strip };
// The rule of what may run with what, in one place: M2V_OK, or the code of the first refusal with its text in the handle (fn: the entry
// it names).  Reads the handle and writes nothing but that text
int begin_refusal(m2v_enc *e, const char *fn, Entry en, uint32_t xs, uint32_t ys, uint32_t pf, size_t nframes);
// ... and the start itself: the rule, then all of e->seq, the geometry, the record queues emptied and the per-sequence counters reset.
// nframes == 0 (a resident call without frames) answers M2V_OK with nothing sampled
int begin_sequence(m2v_enc *e, const char *fn, Entry en, uint32_t xs, uint32_t ys, uint32_t pf, size_t nframes);
// the setters of what a sequence samples, and m2v_mux_device: true = refused (M2V_E_STATE) because the handle is not idle
bool in_progress(m2v_enc *e, const char *fn, const char *why);
// the beat entries take no frames of another size, in any state: true = refused (M2V_E_STATE) because a size is set
bool size_refuses_beats(m2v_enc *e, const char *fn);
// a completed chunk's picture, GOP and scene records (its stream has been waited for) from the stage to the handle's queues
void collect_chunk(m2v_enc *e, m2v_enc::HostStage &h);
// a completed call's sequence and container records to the handle's queues; ok = false: the call overflowed, a batch has none
void collect_call(m2v_enc *e, bool ok);
// a new sequence, or m2v_reset: all five queues empty, and nothing waits in a stage or for a call any more
void drop_records(m2v_enc *e);

// ---- m2v_gop.hip ----
// the level GOP number k of the sequence in progress is coded at, before the cap has had its say
inline int level_of_gop(const m2v_enc *e, size_t k)
{
    if (e->seq.levels.empty()) return e->Q;
    return e->seq.levels[std::min(k, e->seq.levels.size() - 1)];
}
// ... and frame n of a sequence at the fixed cadence (with a list or the detector plan_chunk counts the GOPs itself)
inline int level_of_frame(const m2v_enc *e, size_t n) { return level_of_gop(e, n / (e->pframes + 1u)); }
// the chunk's steps have been enqueued and every group has joined s: slice scan, k_gop_judge, and the GOPs over the cap again at the next
// level until every GOP fits or is at level 4.  Waits for the device, at most three times (encode_chunk, only with the cap on)
void gop_cap_chunk(m2v_enc *e, hipStream_t s);

// ---- m2v_desc.hip ----
// the description as the header writers take it
SeqDesc pack_desc(const m2v_stream_desc &d);

// ---- m2v_scene.hip ----
// The rule of include/m2v_mi355x.h, frame by frame: s = the I picture of the GOP in progress, k = GOP starts so far, list / at = the
// caller's list and the first entry not yet passed.  step(n, cut) answers frame n's M2V_GOP_* bits (0: the GOP goes on) and moves on.
struct GopRule {
    uint32_t pf; const uint32_t *list; size_t nlist, at; size_t s, k;
    uint32_t step(size_t n, bool cut)
    {
        uint32_t fl = 0;
        if (n == 0) fl |= M2V_GOP_FIRST;
        else if (n - s == (size_t)pf + 1) fl |= M2V_GOP_CADENCE;
        while (at < nlist && list[at] < n) ++at;
        if (at < nlist && list[at] == n) fl |= M2V_GOP_LIST;
        if (cut) fl |= M2V_GOP_CUT;
        if (fl) { s = n; ++k; }
        return fl;
    }
};
inline bool seq_has_layout(const m2v_enc *e) { return !e->seq.starts.empty() || e->seq.cut; }
// option "scene_cut", in front of plan_chunk: k_mbsum and k_scene_judge over the chunk's nf frames on s, then the one wait; leaves
// e->chunk_cut / e->chunk_diff
void scene_detect(m2v_enc *e, hipStream_t s, const uint8_t *d_frames, size_t nf);
void scene_release(m2v_enc *e);

// ---- m2v_port.hip ----
// PkFrame::layout of a planar 4:4:4 frame of a sequence that pads its frames (no other planar frame travels as a run)
constexpr int kPk444 = 8;
// PkFrame::layout of a 4:2:0 frame is kPk420 + M2V_420_*
constexpr int kPk420 = 16;
inline bool layout420_ok(int layout) { return layout >= M2V_420_I420 && layout <= M2V_420_NV21; }
// nframes 4:2:0 frames (ysz * 3 / 2 bytes each, back to back at src) -> planar 4:4:4 frames of 3 * ysz bytes at dst, every chroma
// sample repeated 2 x 2 (k_expand420).  src and dst 16-byte aligned.
void launch_expand420(hipStream_t s, int layout, const uint8_t *src, uint8_t *dst, const Geom &g, uint32_t nframes);
// PkFrame::layout of an RGB frame: two neighbours that differ in layout or matrix are two runs
constexpr int kPkRgb = 32;
inline bool rgb_layout_ok(int layout) { return layout >= M2V_RGB_RGB24 && layout <= M2V_RGB_RGBP; }
inline bool rgb_matrix_ok(int matrix) { return matrix >= M2V_RGB_BT601 && matrix <= M2V_RGB_BT709F; }
inline int pk_rgb(int layout, int matrix) { return kPkRgb + 8 * matrix + layout; }
inline int rgb_bpp(int layout) { return layout >= M2V_RGB_RGBX32 && layout <= M2V_RGB_XBGR32 ? 4 : 3; }
// source bytes of one frame of a run kind (PkFrame::layout) whose frames are sz (0 x 0: W x H)
size_t pk_frame_bytes(int kind, const Geom &g, SrcSize sz);
// the frames of a 4:4:4 (kPk444), 4:2:0 or RGB run kind (back to back at src) -> planar 4:4:4 frames of 3 * ysz bytes at dst (16-byte
// aligned).  e->seq.fit set: the frames are of that size and are padded first (k_fit; src at any address), into e->d_fit or, 4:4:4, straight
// into dst; e->seq.src set: they are of that size and are resampled and padded by k_scale instead, the same way.  Else src is 16-byte aligned.
void launch_convert(m2v_enc *e, hipStream_t s, int kind, const uint8_t *src, uint8_t *dst, uint32_t nframes);
// nframes RGB frames (ysz * rgb_bpp(layout) bytes each) -> planar 4:4:4 by the integer transform of include/m2v_mi355x.h (k_rgb2yuv)
void launch_rgb2yuv(hipStream_t s, int layout, int matrix, const uint8_t *src, uint8_t *dst, uint32_t ysz, uint32_t nframes);
// the size of the frames a sequence's whole-frame entries take: the source size of a scaled sequence, else the size to pad, else 0 x 0 (W x H)
inline SrcSize seq_frame_size(const m2v_enc *e) { return e->seq.src.w ? e->seq.src : e->seq.fit; }

// ---- m2v_scale.hip: m2v_set_source_size ----
// a scaled sequence has started (e->seq.src set): the tap tables for its sizes and filter, built and uploaded on s unless the handle holds them
void scale_prepare(m2v_enc *e, hipStream_t s);
// nframes frames of e->seq.src in the form of a run kind, back to back at src (any address) -> the same form at W x H, resampled to
// e->seq.pic and padded, back to back at dst (16-byte aligned): one k_scale launch
void launch_scale(m2v_enc *e, hipStream_t s, int kind, const uint8_t *src, uint8_t *dst, uint32_t nframes);
void scale_release(m2v_enc *e);

// ---- m2v_strips.hip ----
void strip_flight_release(m2v_enc *e);

// ---- m2v_stats.hip: option "stats"; plan_chunk and encode_chunk call the first two, and only while the option is on ----
// the chunk's nf records on the device, zeroed on s (plan_chunk, in front of the chunk's first kernel)
void stats_begin_chunk(m2v_enc *e, hipStream_t s, size_t nf);
// behind the chunk's scans: macroblock counts and bits of its plan_nf frames, then the records into the current stage's pinned memory
void stats_finish_chunk(m2v_enc *e, hipStream_t s);

// ---- m2v_recon.hip: m2v_set_recon_out ----
// bytes of one frame k_recon_out writes for a sequence of xs x ys macroblocks
size_t recon_frame_bytes(const m2v_enc *e, uint32_t xs, uint32_t ys);

// ---- m2v_sequences.hip: m2v_set_sequences ----
inline bool seq_batch(const m2v_enc *e) { return !e->seq.lens.empty(); }
// a batch starts (e->seq.lens and e->pframes are sampled): room for its records, and what the host knows of them into pinned memory
void seq_begin_call(m2v_enc *e);
void seq_release(m2v_enc *e);

// ---- m2v_mux.hip: m2v_set_mux_out ----
// behind the last chunk's assembly on s, in front of the control word's copy: the three kernels over the call's stream(s) in d_out
void mux_resident(m2v_enc *e, hipStream_t s, const uint8_t *d_out, size_t cap, size_t nframes);
// a completed mux's records (its stream has been waited for) to the handle's queue
void mux_collect(m2v_enc *e);
void mux_release(m2v_enc *e);

// ---- m2v_decode.hip: m2v_decode_device ----
void dec_release(m2v_enc *e);
// ---- m2v_decode_streams.hip ----
void ds_release(m2v_enc *e);
// ---- m2v_demux.hip ----
void dmx_release(m2v_enc *e);

// ---- m2v_launch.hip: everything that touches device code ----
// The constant tables live in each device's copy of the code object: uploaded once per device, whichever thread creates the first
// handle there (config c4 creates 8 handles from 8 threads).
void upload_tables(int device);
template <bool P> void launch_mb(m2v_enc *e, hipStream_t s, const int *d_list, int count, const Geom &g);
template <bool P> void launch_mb_edges(m2v_enc *e, hipStream_t s, const int *d_list, int count, const Geom &g, uint8_t *up, uint8_t *down,
                                       const uint8_t *nb_up, const uint8_t *nb_down);
template <bool P> void launch_mb_peer(m2v_enc *e, hipStream_t s, const int *d_list, int count, const Geom &g, uint8_t *put_up, uint8_t *put_down,
                                      const uint8_t *got_up, const uint8_t *got_down, const PeerStep &ps);
extern template void launch_mb_peer<false>(m2v_enc *, hipStream_t, const int *, int, const Geom &, uint8_t *, uint8_t *, const uint8_t *, const uint8_t *, const PeerStep &);
extern template void launch_mb_peer<true>(m2v_enc *, hipStream_t, const int *, int, const Geom &, uint8_t *, uint8_t *, const uint8_t *, const uint8_t *, const PeerStep &);
extern template void launch_mb<false>(m2v_enc *, hipStream_t, const int *, int, const Geom &);
extern template void launch_mb<true>(m2v_enc *, hipStream_t, const int *, int, const Geom &);
// entries [off, off + count) of the launch lists, one launch_mb per run of one level (plan_chunk partitions by level: one per level
// present, and exactly launch_mb(.., e->g) where every entry is at the handle's Q_LEVEL)
template <bool P> inline void launch_mb_levels(m2v_enc *e, hipStream_t s, int off, int count)
{
    for (int a = off, end = off + count; a < end;) {
        int b = a + 1;
        while (b < end && e->plan_list_q[(size_t)b] == e->plan_list_q[(size_t)a]) ++b;
        Geom gg = e->g;
        gg.Q = e->plan_list_q[(size_t)a];
        launch_mb<P>(e, s, e->d_lists.p + a, b - a, gg);
        a = b;
    }
}
extern template void launch_mb_edges<false>(m2v_enc *, hipStream_t, const int *, int, const Geom &, uint8_t *, uint8_t *, const uint8_t *, const uint8_t *);
extern template void launch_mb_edges<true>(m2v_enc *, hipStream_t, const int *, int, const Geom &, uint8_t *, uint8_t *, const uint8_t *, const uint8_t *);
// start of a chunk's stream: the bytes of the sequence that precede it are the previous chunk's prior + total (still in *ctl: one
// stream, in order); only the padding rule needs them.  No launch and no copy: the chunk's k_frame_scan sets the control word up
// itself (its ctl_init argument), this only notes how
void ctl_begin(m2v_enc *e, unsigned long long cap, bool first);
void launch_plan_upload(m2v_enc *e, hipStream_t s, const FrameJob *h_jobs, size_t nf, const int *h_lists, const FrameJob *h_joblist, size_t nlist);
// neighbour-dependent codes + bit offsets of the slices of frames [f0, f1) of the chunk (one block per slice)
void launch_slice_scan(m2v_enc *e, hipStream_t s, const Geom &g, int f0, int f1);
void launch_frame_scan(m2v_enc *e, hipStream_t s, const Geom &g, size_t nf, bool first, bool last, bool advance, uint8_t *d_stream);
// a batch's chunk (m2v_set_sequences): the same, with every sequence that ends in the chunk padded on its own, and the records (k_seq_scan)
void launch_seq_scan(m2v_enc *e, hipStream_t s, const Geom &g, size_t nf, bool advance, uint8_t *d_stream);
void launch_assemble(m2v_enc *e, hipStream_t s, const Geom &g, size_t nf, bool first, bool last, uint8_t *d_stream);
void launch_halo_pack(m2v_enc *e, hipStream_t s, const int *d_list, int count, uint8_t *up, uint8_t *down);
void launch_halo_unpack(m2v_enc *e, hipStream_t s, const int *d_list, int count, const uint8_t *from_up, const uint8_t *from_down);
// strip mode, output rank: where every (frame, rank) piece goes + the copy itself, headers and trailer (k_strip_layout, k_strip_assemble)
void launch_strip_assemble(m2v_enc *e, hipStream_t s, const Geom &g, uint32_t gop, size_t nf, int nranks, const StripSrc &src,
                           const unsigned long long *d_all_off, uint8_t *d_out, unsigned long long cap);
// option "stats": squared error of the `count` frames of a launch list (k_mb's own: d_list points into e->d_lists) into their records in
// e->d_pstat, behind their k_mb launch on s (k_picstat); the rest of the records of the chunk's nf frames, behind its scans (k_picstat_mb)
void launch_picstat(m2v_enc *e, hipStream_t s, const int *d_list, int count);
void launch_picstat_mb(m2v_enc *e, hipStream_t s, size_t nf);
// m2v_set_recon_out: the reconstruction of the `count` frames of a launch list (k_mb's own) as 4:2:0 frames into the buffer the sequence
// sampled, behind their k_mb launch on s (k_recon_out)
void launch_recon_out(m2v_enc *e, hipStream_t s, const int *d_list, int count);
// option "gop_bytes_max": one block per GOP of the chunk's nf frames (whole GOPs of gop frames, the last one may be cut short) sums the
// GOP's bytes, writes its record to e->d_gop and to h_recs (pinned) and raises FrameJob::q of a GOP over the cap (k_gop_judge)
void launch_gop_judge(m2v_enc *e, hipStream_t s, size_t nf, uint32_t gop, unsigned long long cap, m2v_gop_stat *h_recs);
// option "scene_cut": luma sums of the macroblocks of nf planar 4:4:4 frames into e->d_mbsum (k_mbsum), then one block per frame judges
// the difference to the frame before against limit = T * mbs and writes its record to e->d_scene and to h_recs (pinned; k_scene_judge)
void launch_mbsum(m2v_enc *e, hipStream_t s, const uint8_t *d_frames, size_t nf);
void launch_scene_judge(m2v_enc *e, hipStream_t s, size_t nf, unsigned long long limit, const uint32_t *carry_in, uint32_t *carry_out, void *h_recs);
int debug_table(int which, int i, int j);

}  // namespace m2v
