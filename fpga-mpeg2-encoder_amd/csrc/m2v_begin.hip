// m2v_begin.hip — where a sequence starts.  Every setting of the handle (m2v_enc::set) is taken by some entries and not by others, and a
// sequence runs with what it sampled when it started (m2v_enc::seq), whatever the caller sets afterwards.  Both halves of that are here,
// for every entry, and nowhere else:
//
//   begin_refusal          the rule of what may run with what: reads the handle, writes nothing but the refusal's text
//   begin_sequence         the rule, then ALL of m2v_enc::seq, the geometry, the record queues emptied and the per-sequence cursors reset.
//                          An entry refuses every setting it does not take, so what it samples of such a setting is "off": no path
//                          sees what another entry's sequence sampled.
//   the records            picture, GOP and scene records travel with a chunk's stage (collect_chunk), sequence and container records
//                          with a call (collect_call); drop_records empties all five queues.
//
// Nothing here allocates in the steady state (the vectors of `seq` are assigned into), waits, copies or launches.
#include "m2v_host.hpp"

namespace m2v {

static bool busy(const m2v_enc *e) { return e->state != m2v_enc::IDLE || e->resident_inflight || e->strip_active || e->strip_inflight; }

bool in_progress(m2v_enc *e, const char *fn, const char *why)
{
    if (!busy(e)) return false;
    e->set_err("%s: a sequence is in progress (%s)", fn, why);
    return true;
}

static int refuse(m2v_enc *e, int code, const char *fn, const char *what)
{
    e->set_err("%s: %s", fn, what);
    return code;
}

// a size is set (m2v_set_frame_size) and the entry takes no frames of another size
static int size_refuses(m2v_enc *e, const char *fn, const char *why)
{
    if (!e->set.size.w) return M2V_OK;
    e->set_err("%s: a frame size is set (m2v_set_frame_size): %s", fn, why);
    return M2V_E_STATE;
}

bool size_refuses_beats(m2v_enc *e, const char *fn) { return size_refuses(e, fn, "the port has no partial macroblock, push whole frames") != M2V_OK; }

// a source size is set (m2v_set_source_size) and the entry resamples nothing
static int source_refuses(m2v_enc *e, const char *fn, const char *why)
{
    if (!e->set.src.w) return M2V_OK;
    e->set_err("%s: a source size is set (m2v_set_source_size): %s", fn, why);
    return M2V_E_STATE;
}

// the picture size of a sequence that starts with xs, ys: the size set, else W x H
static SrcSize picture_size(m2v_enc *e, uint32_t xs, uint32_t ys)
{
    if (e->set.size.w) return e->set.size;
    const Geom g = make_geom(e, xs, ys);
    return SrcSize{g.W, g.H};
}

// xs, ys are not m2v_fit_size's for the size set
static int size_mismatch(m2v_enc *e, const char *fn, uint32_t xs, uint32_t ys)
{
    const SrcSize z = e->set.size;
    if (!z.w) return M2V_OK;
    uint32_t fx = 0, fy = 0;
    (void)m2v_fit_size(z.w, z.h, &fx, &fy);
    if (xs == fx && ys == fy) return M2V_OK;
    e->set_err("%s: xsize16, ysize16 = %u, %u, but the frame size set is %d x %d (m2v_fit_size: %u, %u)", fn, xs, ys, z.w, z.h, fx, fy);
    return M2V_E_PARAM;
}

// the port entries (from IDLE): what only the resident entries take
static int port_refusal(m2v_enc *e, const char *fn)
{
    const m2v_enc::Settings &set = e->set;
    if (const int r = source_refuses(e, fn, "the stage's packed bytes are sized for frames of the coded size, the resident entries resample")) return r;
    if (set.gop_bytes_max) return refuse(e, M2V_E_STATE, fn, "option \"gop_bytes_max\" is set: the cap needs whole GOPs in a chunk, which only the resident entries give");
    if (set.scene_cut) return refuse(e, M2V_E_STATE, fn, "option \"scene_cut\" is set: the detector runs in front of a chunk's plan, which only the resident entries wait for");
    if (!set.sequences.empty()) return refuse(e, M2V_E_STATE, fn, "a batch of sequences is set (m2v_set_sequences): the port carries one sequence, the batch is the resident entries'");
    if (set.recon.p) return refuse(e, M2V_E_STATE, fn, "a buffer for the reconstruction is set (m2v_set_recon_out): it is a device buffer, filled by the resident entries");
    if (set.mux.kind) return refuse(e, M2V_E_STATE, fn, "a container buffer is set (m2v_set_mux_out): it is a device buffer, filled by the resident entries");
    return M2V_OK;
}

// the strip entries: whole padded frames, one stream, the module's headers at the handle's Q_LEVEL and the fixed cadence
static int strip_refusal(m2v_enc *e, const char *fn)
{
    const m2v_enc::Settings &set = e->set;
    if (const int r = size_refuses(e, fn, "strips take whole padded frames")) return r;
    if (const int r = source_refuses(e, fn, "strips take whole padded frames of the coded size")) return r;
    if (!set.sequences.empty()) return refuse(e, M2V_E_STATE, fn, "a batch of sequences is set (m2v_set_sequences): the strip assembly writes one stream");
    if (set.mux.kind) return refuse(e, M2V_E_STATE, fn, "a container buffer is set (m2v_set_mux_out): the muxer follows the resident entries' stream");
    if (set.recon.p) return refuse(e, M2V_E_STATE, fn, "a buffer for the reconstruction is set (m2v_set_recon_out): a strip holds part of a picture, and nothing gathers the parts");
    if (e->stats_on) return refuse(e, M2V_E_STATE, fn, "option \"stats\" is on: a strip holds part of a picture, and nothing sums the records across ranks");
    if (!set.gop_levels.empty() || set.gop_bytes_max)
        return refuse(e, M2V_E_STATE, fn, "a level per GOP is set (m2v_set_gop_levels or option \"gop_bytes_max\"): a strip is coded at the handle's Q_LEVEL");
    if (!set.gop_starts.empty() || set.scene_cut)
        return refuse(e, M2V_E_STATE, fn, "GOP starts are set (m2v_set_gop_starts or option \"scene_cut\"): the strips of a frame run at the fixed cadence");
    if (set.desc_set) return refuse(e, M2V_E_STATE, fn, "a stream description is set (m2v_set_stream_desc): the strip assembly writes the module's headers");
    return M2V_OK;
}

// the resident entries, in front of the point where the previous call's records are dropped: the handle is busy, or the list of
// m2v_set_sequences does not describe this call
static int resident_refusal_early(m2v_enc *e, const char *fn, size_t nframes)
{
    const m2v_enc::Settings &set = e->set;
    if (busy(e)) return refuse(e, M2V_E_STATE, "m2v_encode_resident", "encoder busy");
    if (set.sequences.empty()) return M2V_OK;
    size_t sum = 0;
    for (size_t b = 0; b < set.sequences.size(); ++b) {
        if (!set.sequences[b]) { e->set_err("%s: entry %zu of m2v_set_sequences is 0: a sequence has at least one frame", fn, b); return M2V_E_PARAM; }
        sum += set.sequences[b];
    }
    if (sum != nframes) {
        e->set_err("%s: nframes = %zu, the entries of m2v_set_sequences add up to %zu", fn, nframes, sum);
        return M2V_E_PARAM;
    }
    if (set.sequences.size() >= 2 && (!set.gop_starts.empty() || set.scene_cut || set.gop_bytes_max)) {
        e->set_err("%s: a batch of sequences (m2v_set_sequences) is set together with %s: its host side counts one sequence", fn,
                   !set.gop_starts.empty() ? "m2v_set_gop_starts" : set.scene_cut ? "option \"scene_cut\"" : "option \"gop_bytes_max\"");
        return M2V_E_STATE;
    }
    return M2V_OK;
}

// ... and behind it (a call without frames starts nothing and is asked nothing more)
static int resident_refusal_late(m2v_enc *e, const char *fn, uint32_t xs, uint32_t ys, uint32_t pf, size_t nframes)
{
    const m2v_enc::Settings &set = e->set;
    if (!nframes) return M2V_OK;
    if (set.gop_bytes_max && (!set.gop_starts.empty() || set.scene_cut))
        return refuse(e, M2V_E_STATE, fn, "option \"gop_bytes_max\" is set together with GOP starts (m2v_set_gop_starts or option \"scene_cut\"): the cap judges GOPs of "
                                          "the fixed cadence");
    if (set.mux.kind && set.sequences.size() > 65535) return refuse(e, M2V_E_PARAM, fn, "a container buffer is set (m2v_set_mux_out): at most 65535 clips in a batch");
    if (set.recon.p) {
        const size_t fb = recon_frame_bytes(e, xs, ys);
        if (nframes > set.recon.cap / fb) {
            e->set_err("%s: %zu frames of %zu bytes do not fit the buffer of m2v_set_recon_out (%zu bytes)", fn, nframes, fb, set.recon.cap);
            return M2V_E_OVERFLOW;
        }
    }
    if (const int r = size_mismatch(e, fn, xs, ys)) return r;
    if (set.src.w) {
        const SrcSize pic = picture_size(e, xs, ys);
        if (set.src.w > 8 * pic.w || set.src.h > 8 * pic.h) {
            e->set_err("%s: the source size set (m2v_set_source_size) is %d x %d, more than 8 times the picture size %d x %d in a dimension", fn,
                       set.src.w, set.src.h, pic.w, pic.h);
            return M2V_E_PARAM;
        }
    }
    if (set.gop_bytes_max && (size_t)(pf & 0xFFu) + 1 > e->batch_frames) {
        e->set_err("m2v_encode_resident: option \"gop_bytes_max\" needs whole GOPs in a chunk: pframes_count + 1 = %u is more than batch_frames = %zu",
                   (pf & 0xFFu) + 1u, e->batch_frames);
        return M2V_E_PARAM;
    }
    return M2V_OK;
}

int begin_refusal(m2v_enc *e, const char *fn, Entry en, uint32_t xs, uint32_t ys, uint32_t pf, size_t nframes)
{
    switch (en) {
    case Entry::Beats: return port_refusal(e, fn);            // (size_refuses_beats has had its say, as it has in every state)
    case Entry::Frames: if (const int r = port_refusal(e, fn)) return r; return size_mismatch(e, fn, xs, ys);
    case Entry::Strip: return strip_refusal(e, fn);
    case Entry::Resident: break;
    }
    if (const int r = resident_refusal_early(e, fn, nframes)) return r;
    return resident_refusal_late(e, fn, xs, ys, pf, nframes);
}

int begin_sequence(m2v_enc *e, const char *fn, Entry en, uint32_t xs, uint32_t ys, uint32_t pf, size_t nframes)
{
    // A resident call drops the previous call's records once it is known not to be busy and to fit its list, and some of its refusals
    // fire after that: the caller of a call refused there finds the queues empty.  (Every other entry refuses with nothing touched.)
    int r = en == Entry::Resident ? resident_refusal_early(e, fn, nframes) : begin_refusal(e, fn, en, xs, ys, pf, nframes);
    if (r) return r;
    drop_records(e);
    if (en == Entry::Resident) {
        e->resident_empty = false;
        r = resident_refusal_late(e, fn, xs, ys, pf, nframes);
        if (r || !nframes) return r;                    // (no beat: the sequence never starts)
    }

    const m2v_enc::Settings &set = e->set;
    m2v_enc::Sampled &seq = e->seq;
    e->g = make_geom(e, xs, ys);                        // latched on the first beat (RTL:1060-1065)
    e->pframes = pf & 0xFFu;
    e->frames_total = 0;
    e->persist_slot = -1;
    for (auto &st : e->stats) st = KStat{};
    // Every setting is sampled as it stands: one that this entry does not take was refused above, so it is off here.
    const bool pad = set.size.w && ((set.size.w | set.size.h) & 15);
    seq.fit = pad ? set.size : SrcSize{};
    seq.hdr_true = pad && set.header == M2V_HEADER_TRUE;
    // (a source of the picture size samples as none: the launches and buffers of a handle with nothing set)
    seq.pic = picture_size(e, xs, ys);
    const bool scaled = set.src.w && (set.src.w != seq.pic.w || set.src.h != seq.pic.h);
    seq.src = scaled ? set.src : SrcSize{};
    seq.filter = set.filter;
    if (!scaled) seq.pic = SrcSize{};
    seq.levels = set.gop_levels;
    seq.cap = set.gop_bytes_max;
    seq.starts = set.gop_starts;
    seq.cut = set.scene_cut;
    seq.desc = set.desc_set ? pack_desc(set.desc) : seq_desc_module();
    if (set.sequences.size() >= 2) seq.lens = set.sequences;        // (a list of one entry samples as none)
    else seq.lens.clear();
    seq.recon = set.recon;
    if (seq.recon.p) seq.recon.fb = recon_frame_bytes(e, xs, ys);
    seq.mux = set.mux;
    // the cursors that travel from chunk to chunk
    e->gop_s = e->gop_k = 0;
    e->carry_cur = -1;
    e->chunk_cut.clear();
    e->chunk_diff.clear();
    e->seq_at = e->seq_f0 = e->plan_seq0 = e->plan_nsq = 0;
    if (seq_batch(e)) seq_begin_call(e);
    return M2V_OK;
}

void collect_chunk(m2v_enc *e, m2v_enc::HostStage &h)
{
    e->pstat_q.push(h.h_pstat, h.h_pstat + h.nstat);
    e->gop_q.push(h.h_gop, h.h_gop + h.ngop);
    e->scene_q.push(h.scene.data(), h.scene.data() + h.scene.size());
    h.nstat = h.ngop = 0;
    h.scene.clear();
}

void collect_call(m2v_enc *e, bool ok)
{
    if (e->seq_pending && ok) e->seq_q.push(e->h_seq, e->h_seq + e->seq.lens.size());
    e->seq_pending = false;
    mux_collect(e);
}

void drop_records(m2v_enc *e)
{
    e->pstat_q.clear(); e->gop_q.clear(); e->scene_q.clear(); e->seq_q.clear(); e->mux_q.clear();
    for (auto &h : e->hs) { h.nstat = h.ngop = 0; h.scene.clear(); }
    e->seq_pending = e->mux_pending = false;
}

}  // namespace m2v
