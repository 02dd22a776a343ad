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
// A list of one entry samples as none: nothing here or in plan_chunk is reached, the call is the call of a handle with nothing set.
#include "m2v_host.hpp"

static_assert(sizeof(m2v_sequence_stat) == 32, "the record of include/m2v_mi355x.h is 32 bytes");

namespace m2v {

int seq_check(m2v_enc *e, const char *fn, size_t nframes)
{
    if (e->sequences.empty()) return M2V_OK;
    size_t sum = 0;
    for (size_t b = 0; b < e->sequences.size(); ++b) {
        if (!e->sequences[b]) { e->set_err("%s: entry %zu of m2v_set_sequences is 0: a sequence has at least one frame", fn, b); return M2V_E_PARAM; }
        sum += e->sequences[b];
    }
    if (sum != nframes) {
        e->set_err("%s: nframes = %zu, the entries of m2v_set_sequences add up to %zu", fn, nframes, sum);
        return M2V_E_PARAM;
    }
    if (e->sequences.size() < 2) return M2V_OK;
    if (!e->gop_starts.empty() || e->scene_cut || e->gop_bytes_max) {
        e->set_err("%s: a batch of sequences (m2v_set_sequences) is set together with %s: its host side counts one sequence", fn,
                   !e->gop_starts.empty() ? "m2v_set_gop_starts" : e->scene_cut ? "option \"scene_cut\"" : "option \"gop_bytes_max\"");
        return M2V_E_STATE;
    }
    return M2V_OK;
}

void sample_sequences(m2v_enc *e)
{
    e->seq_lens.clear();
    e->seq_at = e->seq_f0 = e->plan_seq0 = 0;
    e->plan_nsq = 0;
    if (e->sequences.size() < 2) return;
    e->seq_lens = e->sequences;
    const size_t n = e->seq_lens.size();
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
        const uint32_t len = e->seq_lens[b];
        e->h_seq[b] = m2v_sequence_stat{0ull, 0ull, f0, len, (len + gop - 1u) / gop, 0u};
        f0 += len;
    }
    e->seq_pending = true;
}

bool seq_refuses(m2v_enc *e, const char *fn)
{
    if (e->sequences.empty()) return false;
    e->set_err("%s: a batch of sequences is set (m2v_set_sequences): the port carries one sequence, the batch is the resident entries'", fn);
    return true;
}

void seq_collect(m2v_enc *e, bool ok)
{
    if (e->seq_pending && ok) e->seq_q.assign(e->h_seq, e->h_seq + e->seq_lens.size());
    e->seq_pending = false;
}

void seq_drop(m2v_enc *e)
{
    e->seq_q.clear();
    e->seq_pending = false;
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
    if (e->state != m2v_enc::IDLE || e->resident_inflight || e->strip_active || e->strip_inflight) {
        e->set_err("m2v_set_sequences: a sequence is in progress (the list is sampled when a call starts)");
        return M2V_E_STATE;
    }
    if (!frames_per_sequence || !n) { e->sequences.clear(); return M2V_OK; }
    if (n > 0x3FFFFFFFu) { e->set_err("m2v_set_sequences: at most 2^30 - 1 entries"); return M2V_E_PARAM; }
    try { e->sequences.assign(frames_per_sequence, frames_per_sequence + n); }
    catch (...) { e->set_err("m2v_set_sequences: host allocation failed"); return M2V_E_NOMEM; }
    return M2V_OK;
}

int m2v_sequence_report(m2v_enc *e, m2v_sequence_stat *out, size_t max)
{
    if (!e) return M2V_E_PARAM;
    if (!out) return (int)std::min<size_t>(e->seq_q.size(), 0x7FFFFFFF);
    const size_t n = std::min<size_t>({max, e->seq_q.size(), (size_t)0x7FFFFFFF});
    std::copy(e->seq_q.begin(), e->seq_q.begin() + (std::ptrdiff_t)n, out);
    e->seq_q.erase(e->seq_q.begin(), e->seq_q.begin() + (std::ptrdiff_t)n);
    return (int)n;
}

}  // extern "C"
