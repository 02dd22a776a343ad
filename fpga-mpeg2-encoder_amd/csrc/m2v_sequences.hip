// m2v_sequences.hip — a batch of sequences in one resident call, host side (include/m2v_mi355x.h, m2v_set_sequences): many short
// clips, one stream each, out of the launches of one call.  plan_chunk already runs step j of every closed GOP of a chunk in one launch
// because closed GOPs are independent; the frames of different sequences are exactly as independent, so on the plan side a sequence
// boundary is one more place where a GOP segment starts, and k_mb is untouched.
//
//   the plan               plan_chunk counts a frame from its own sequence's first frame (FrameJob::n, i_frame, the level schedule's
//                          ordinal) and notes in FrameJob::pad whether it is the first or the last of its sequence and which of the
//                          chunk's sequences it belongs to; the last picture of a sequence is followed by nothing.  The handle carries the
//                          open sequence (seq_at, seq_f0) across chunks: a chunk may cut a sequence anywhere.
//   the streams            k_seq_scan (m2v_seq_kernels.hpp, launched from m2v_launch.hip) takes k_frame_scan's place: every sequence
//                          that ends in the chunk gets its own end code and final-word padding, so every stream starts on a 32-byte
//                          boundary.  k_assemble's two conditions for the sequence headers and the end code also take the job's flags.
//   the records            first_frame, frames and gops are plain arithmetic, written here into pinned memory when the call starts;
//                          k_seq_scan fills in offset and bytes with every chunk, on the device (the open sequence's travel to the
//                          next chunk there) and in pinned memory, which is complete where the control word is.  No wait, no copy
//                          and no launch is added.
//
// A list of one entry samples as none (begin_sequence): nothing here or in plan_chunk is reached, the call is the call of a handle with nothing set.
#include "m2v_host.hpp"

static_assert(sizeof(m2v_sequence_stat) == 32, "the record of include/m2v_mi355x.h is 32 bytes");

namespace m2v {

void seq_begin_call(m2v_enc *e)
{
    const size_t n = e->seq.lens.size();
    e->d_seq.recorded = false;
    e->d_seq.ensure(n);
    if (e->h_seq_cap < n) {              // (free: the handle is idle, the previous call's records have been collected or dropped)
        if (e->h_seq) (void)hipHostFree(e->h_seq);
        e->h_seq = nullptr; e->h_seq_cap = 0;
        HIPCHK(hipHostMalloc((void **)&e->h_seq, n * sizeof(m2v_sequence_stat)));
        e->h_seq_cap = n;
    }
    const uint32_t gop = e->pframes + 1u;
    uint32_t f0 = 0;
    for (size_t b = 0; b < n; ++b) {
        const uint32_t len = e->seq.lens[b];
        e->h_seq[b] = m2v_sequence_stat{0ull, 0ull, f0, len, (len + gop - 1u) / gop, 0u};
        f0 += len;
    }
    e->seq_pending = true;
}

void seq_release(m2v_enc *e)
{
    e->d_seq.release(); e->d_seqtmp.release();
    if (e->h_seq) (void)hipHostFree(e->h_seq);
    e->h_seq = nullptr; e->h_seq_cap = 0;
}

}  // namespace m2v

extern "C" {

int m2v_set_sequences(m2v_enc *e, const uint32_t *frames_per_sequence, size_t n)
{
    if (!e) return M2V_E_PARAM;
    if (in_progress(e, "m2v_set_sequences", "the list is sampled when a call starts")) return M2V_E_STATE;
    if (!frames_per_sequence || !n) { e->set.sequences.clear(); return M2V_OK; }
    if (n > 0x3FFFFFFFu) { e->set_err("m2v_set_sequences: at most 2^30 - 1 entries"); return M2V_E_PARAM; }
    try { e->set.sequences.assign(frames_per_sequence, frames_per_sequence + n); }
    catch (...) { e->set_err("m2v_set_sequences: host allocation failed"); return M2V_E_NOMEM; }
    return M2V_OK;
}

int m2v_sequence_report(m2v_enc *e, m2v_sequence_stat *out, size_t max)
{
    if (!e) return M2V_E_PARAM;
    return e->seq_q.pop31(out, max);
}

}  // extern "C"
