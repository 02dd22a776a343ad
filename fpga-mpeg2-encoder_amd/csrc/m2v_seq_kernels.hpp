// m2v_seq_kernels.hpp — device code of m2v_set_sequences (m2v_sequences.hip tells the whole story): k_seq_scan, which takes
// k_frame_scan's place for the chunks of a batch.  Included by m2v_launch.hip behind m2v_kernels.hpp, whose frame_header_bytes and
// wave_scan_incl it uses (that header defines kernels and device globals with external linkage, so one unit only can include it).
#pragma once
#include "../../include/m2v_mi355x.h"
#include "m2v_kernels.hpp"

static_assert(sizeof(m2v_sequence_stat) == 32 && offsetof(m2v_sequence_stat, bytes) == 8 && offsetof(m2v_sequence_stat, first_frame) == 16,
              "k_seq_scan writes the record in place");

namespace m2v {

constexpr int kSeqThreads = 1024;      // one block: 16 wavefronts
constexpr int kSeqLds = 1024;         // sequences of a chunk whose raw starts and deltas pass from thread to thread through LDS (more: through memory)
constexpr int kSeqCached = 4;          // items a thread keeps in registers between its passes (k_frame_scan keeps 8: it has one pass less)

// Inclusive scan of one 64-bit value per thread over the block, and the block's total.  Inside a wavefront by DPP - which moves 32 bits,
// so the value goes as three parts whose wavefront totals cannot wrap (bits 0-15, bits 16-31, the rest) - then the 16 wavefront totals
// through LDS (every call its own s_wtot: one barrier).
__device__ __forceinline__ unsigned long long seq_block_scan(unsigned long long v, unsigned long long *s_wtot, int tid, unsigned long long &grand)
{
    const unsigned long long wscan = (unsigned long long)(uint32_t)wave_scan_incl((int)((uint32_t)v & 0xFFFFu)) +
                                     ((unsigned long long)(uint32_t)wave_scan_incl((int)(((uint32_t)v >> 16) & 0xFFFFu)) << 16) +
                                     ((unsigned long long)(uint32_t)wave_scan_incl((int)(uint32_t)(v >> 32)) << 32);
    if ((tid & 63) == 63) s_wtot[tid >> 6] = wscan;
    __syncthreads();
    unsigned long long before = 0;
    grand = 0;
#pragma unroll
    for (int w = 0; w < kSeqThreads / 64; ++w) {
        const unsigned long long t = s_wtot[w];
        before += w < (tid >> 6) ? t : 0ull;
        grand += t;
    }
    return before + wscan;
}

// kSeqCached consecutive items from item i on (items at or past i1 count nothing): a slice's bytes, and in one word the header bytes
// in front of it (bits 0-7; at most 59, and not 0 exactly where the item is its frame's first slice) and its frame's flags word (from
// bit 8).  Every load is unconditional - an item out of range reads item 0 - so that the loads of a group are in flight together.
struct SeqItems { uint32_t sb[kSeqCached], hf[kSeqCached]; };
__device__ __forceinline__ SeqItems seq_load(const FrameJob *__restrict__ jobs, const uint32_t *__restrict__ slice_bytes, const Geom &g,
                                             int rows, int repeat, int i, int i1)
{
    SeqItems it;
    int f = i / rows, r = i - f * rows;
#pragma unroll
    for (int j = 0; j < kSeqCached; ++j) {
        const bool in = i + j < i1;
        const int ff = in ? f : 0, rr = in ? r : 0;
        const uint32_t sb = slice_bytes[(size_t)ff * g.mbh + g.row0 + rr], fl = jobs[ff].pad;
        const int i_frame = jobs[ff].i_frame;
        // bytes in front of the frame's first slice: its own headers, and the sequence headers in front of a sequence's first frame and,
        // with repeat_headers, in front of every later GOP
        const uint32_t hb = rr ? 0u : frame_header_bytes(i_frame) + ((fl & kSeqFirst) || (repeat && i_frame == 0) ? kSeqHeaderBytes : 0u);
        it.sb[j] = in ? sb : 0u;
        it.hf[j] = in ? hb | fl << 8 : 0u;
        if (++r == rows) { r = 0; ++f; }
    }
    return it;
}

// k_seq_scan: byte offsets of the frames and slices of a chunk whose frames belong to several sequences (FrameJob::pad says which:
// kSeqFirst, kSeqLast, the sequence's ordinal among those the chunk touches).  Behind every sequence that ends in the chunk stand its
// sequence_end_code and the padding of its final 32-byte word, whose length depends on the bytes in front - so a plain prefix sum over
// the items no longer does.  It stays a scan because every sequence starts on a 32-byte boundary of the output: its padded length,
// ((B + 4) / 32 + 1) * 32, depends on its own bytes B alone.  One block, as k_frame_scan:
//   1  items (a slice, preceded by its frame's headers when it is the frame's first) as k_frame_scan takes them, K consecutive ones per
//      thread: the block scan of their bytes gives every item its RAW offset - the offset with no tail anywhere - and, where an item
//      starts a sequence, that sequence's raw start (seq_raw[j]; seq_raw[nsq] = the raw total).  A sequence's bytes in this chunk are the
//      difference of two neighbours.
//   2  sequences, KS consecutive ones per thread: the padded length of each that ends here (the one the chunk starts in counts the bytes
//      it brought along: carry), the plain length of the one the chunk leaves open.
//   3  the block scan of those lengths places the sequences; seq_delta[j] = what the tails in front of sequence j add to a raw offset.
//      The same threads write the records (device: offset and bytes carry to the next chunk; pinned: what m2v_sequence_report hands
//      out) and clear each finished sequence's tail, as thread 1023 of k_frame_scan does for its one tail.
//   4  items again: frame_off / slice_off = raw offset + seq_delta[sequence of the item's frame].
// Sums are 64 bits throughout.  Thresholds: more than 1024 items make K > 1, more than 1024 * kSeqCached send a thread's items past the
// ones it keeps in registers (the others are fetched again in every pass, kSeqCached loads in flight at a time), more than kSeqLds
// sequences make KS > 1 and send seq_raw / seq_delta from LDS to memory.
// seq_tmp: room for [nsq + 1] raw starts, then [nsq] deltas, nsq <= nframes (used beyond kSeqLds sequences).  recs / h_recs: the call's
// records, seq0 = that of the chunk's first frame (first_frame, frames and gops of the pinned records are the host's; the device
// records hold offset and bytes only).  ctl_init, ctl_cap, advance: k_frame_scan's.
__global__ __launch_bounds__(kSeqThreads) void k_seq_scan(const FrameJob *__restrict__ jobs, Geom g, int nframes,
                                                          const uint32_t *__restrict__ slice_bytes,
                                                          unsigned long long *__restrict__ slice_off,
                                                          unsigned long long *__restrict__ frame_off, StreamCtl *ctl,
                                                          int advance, uint32_t *__restrict__ out32, int ctl_init, unsigned long long ctl_cap,
                                                          int repeat, unsigned long long *seq_tmp, m2v_sequence_stat *recs,
                                                          m2v_sequence_stat *h_recs, int seq0)
{
    __shared__ unsigned long long s_base;
    __shared__ unsigned long long s_wtot[2][kSeqThreads / 64];
    __shared__ unsigned long long s_seq[2 * kSeqLds + 1];
    const int tid = threadIdx.x;
    unsigned long long c_prior = 0, c_cap = ctl_cap & ~3ull;
    uint32_t c_ov = 0;
    if (ctl_init == 0) { c_prior = ctl->prior_bytes; c_cap = ctl->cap_bytes; c_ov = ctl->overflow; }
    else if (ctl_init == 2) c_prior = ctl->prior_bytes + ctl->total_bytes;
    if (tid == 0) {
        unsigned long long b = 0;
        if (ctl_init == 0) {
            b = ctl->base_bytes;
            if (advance && !ctl->overflow) { b = ctl->total_bytes; ctl->base_bytes = b; }
        }
        s_base = b;
    }
    // the sequence the chunk starts in: a new one, or one that brings its offset and its bytes so far along
    const uint32_t fl_first = jobs[0].pad, fl_last = jobs[nframes - 1].pad;
    const bool opens = (fl_first & kSeqFirst) != 0, closes = (fl_last & kSeqLast) != 0;
    const int nsq = (int)(fl_last >> kSeqOrdShift) + 1;
    const unsigned long long carry = opens ? 0ull : recs[seq0].bytes, carry_off = opens ? 0ull : recs[seq0].offset;
    // (LDS or memory behind one pointer: flat addressing; a round trip through memory is a microsecond in this one workgroup of pure latency)
    unsigned long long *const seq_raw = nsq <= kSeqLds ? s_seq : seq_tmp, *const seq_delta = seq_raw + nsq + 1;

    // ---- 1: raw offsets of the items ----
    const int rows = g.row1 - g.row0;
    const int S = nframes * rows;
    const int K = (S + kSeqThreads - 1) / kSeqThreads;
    const int i0 = tid * K, i1 = i0 + K < S ? i0 + K : S;
    // the thread's first kSeqCached items stay in registers for the later passes; the others are fetched again, a group at a time
    const SeqItems c0 = seq_load(jobs, slice_bytes, g, rows, repeat, i0, i1);
    auto group_bytes = [](const SeqItems &t) {
        unsigned long long v = 0;
#pragma unroll
        for (int j = 0; j < kSeqCached; ++j) v += (unsigned long long)t.sb[j] + (t.hf[j] & 0xFFu);
        return v;
    };
    unsigned long long sum = group_bytes(c0);
    for (int i = i0 + kSeqCached; i < i1; i += kSeqCached) sum += group_bytes(seq_load(jobs, slice_bytes, g, rows, repeat, i, i1));
    unsigned long long raw_total;
    const unsigned long long first_raw = seq_block_scan(sum, s_wtot[0], tid, raw_total) - sum;      // raw offset of the thread's first item
    {
        // where a sequence starts in the chunk: its raw start (the chunk's first frame belongs to ordinal 0 either way)
        unsigned long long run = first_raw;
        auto mark = [&](const SeqItems &t, int i) {
#pragma unroll
            for (int j = 0; j < kSeqCached; ++j) {
                const uint32_t hb = t.hf[j] & 0xFFu, fl = t.hf[j] >> 8;
                if (hb && i + j > 0 && (fl & kSeqFirst)) seq_raw[fl >> kSeqOrdShift] = run;
                run += (unsigned long long)t.sb[j] + hb;
            }
        };
        mark(c0, i0);
        for (int i = i0 + kSeqCached; i < i1; i += kSeqCached) mark(seq_load(jobs, slice_bytes, g, rows, repeat, i, i1), i);
        if (tid == 0) { seq_raw[0] = 0ull; seq_raw[nsq] = raw_total; }
    }
    __syncthreads();                                          // seq_raw is complete

    // ---- 2: lengths of the sequences ----
    const int KS = (nsq + kSeqThreads - 1) / kSeqThreads;
    const int j0 = tid * KS, j1 = j0 + KS < nsq ? j0 + KS : nsq;
    auto seq_len = [&](int j, unsigned long long raw) -> unsigned long long {
        if (j == nsq - 1 && !closes) return raw;              // goes on in the next chunk
        const unsigned long long c = j == 0 ? carry : 0ull;
        return ((c + raw + 4ull) / 32ull + 1ull) * 32ull - c;        // end code + the final word always leaves (RTL:2621-2628, 2932-2937)
    };
    unsigned long long lsum = 0;
    for (int j = j0; j < j1; ++j) lsum += seq_len(j, seq_raw[j + 1] - seq_raw[j]);
    unsigned long long all;
    unsigned long long srun = seq_block_scan(lsum, s_wtot[1], tid, all) - lsum;

    // ---- 3: the sequences' places, their records, their tails ----
    const unsigned long long base = s_base;
    const unsigned long long total = base + all;
    const bool ov = total > c_cap || c_ov;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long at = seq_raw[j], raw = seq_raw[j + 1] - at, len = seq_len(j, raw);
        seq_delta[j] = srun - at;
        const bool cont = j == 0 && !opens;
        // offset and bytes, to the device record and to the pinned one (whose other fields the host wrote when the call started)
        const unsigned long long off = cont ? carry_off : base + srun, bytes = (cont ? carry : 0ull) + len;
        *(ulonglong2 *)(recs + seq0 + j) = ulonglong2{off, bytes};
        *(ulonglong2 *)(h_recs + seq0 + j) = ulonglong2{off, bytes};
        if (!ov && len != raw)                                // the tail: k_assemble writes the end code into it, nobody the zeros
            for (unsigned long long w = (base + srun + raw) >> 2; w < (base + srun + len + 3ull) >> 2; ++w) out32[w] = 0u;
        srun += len;
    }
    __syncthreads();                                          // seq_delta is complete; everyone has read the control word

    // ---- 4: the items' places ----
    {
        unsigned long long run = first_raw;
        auto place = [&](const SeqItems &t, int i) {
            int f = i / rows, r = i - f * rows;
            unsigned long long d[kSeqCached];
#pragma unroll
            for (int j = 0; j < kSeqCached; ++j) d[j] = seq_delta[i + j < i1 ? t.hf[j] >> (8 + kSeqOrdShift) : 0u];
#pragma unroll
            for (int j = 0; j < kSeqCached; ++j) {
                if (i + j < i1) {
                    const uint32_t hb = t.hf[j] & 0xFFu;
                    if (r == 0) {
                        // the frame's own headers start here: behind the sequence headers where hb holds them (more than any frame's own headers)
                        frame_off[f] = run + d[j] + (hb > kGopHeaderBytes + 17u ? kSeqHeaderBytes : 0u);
                        run += hb;
                    }
                    slice_off[(size_t)f * g.mbh + g.row0 + r] = run + d[j];
                    run += t.sb[j];
                }
                if (++r == rows) { r = 0; ++f; }
            }
        };
        place(c0, i0);
        for (int i = i0 + kSeqCached; i < i1; i += kSeqCached) place(seq_load(jobs, slice_bytes, g, rows, repeat, i, i1), i);
    }
    if (tid == kSeqThreads - 1) {
        frame_off[nframes] = all;
        if (ctl_init) { ctl->base_bytes = 0; ctl->cap_bytes = c_cap; ctl->prior_bytes = c_prior; ctl->pad = 0; }
        ctl->total_bytes = total;
        ctl->overflow = ov ? 1u : 0u;
    }
}

}  // namespace m2v
