// m2v_resident.hip — whole sequences with input and output resident in HBM (what bench.py times): m2v_encode_resident, its two
// halves _begin / _end for callers that keep several sequences in flight, and the same for 4:2:0 input (m2v_encode_resident420) and
// RGB input (m2v_encode_resident_rgb).
#include "m2v_host.hpp"

extern "C" {

struct ResidentArgs { uint32_t xs, ys, pf; const uint8_t *d_in; size_t n; uint8_t *d_out; size_t cap; size_t *bytes; hipStream_t s; bool async = false;
                      int kind = -1; };        // kind >= 0: d_in holds 4:2:0 or RGB frames (a run kind: kPk420 + M2V_420_*, pk_rgb())

// The resident entry in two halves: everything enqueued (m2v_encode_resident_begin), then the one wait and the byte count
// (m2v_encode_resident_end).  m2v_encode_resident is both, back to back.
static int resident_end_impl(m2v_enc *e, void *argp)
{
    auto *bytes = (size_t *)argp;
    if (!e->resident_inflight) { e->set_err("m2v_encode_resident_end: nothing in flight"); return M2V_E_STATE; }
    e->resident_inflight = false;
    HIPCHK(hipStreamSynchronize(e->resident_stream));
    collect_timers(e);
    collect_chunk(e, e->st());
    collect_call(e, !e->st().h_ctl->overflow);
    if (e->st().h_ctl->overflow) { e->set_err("output buffer too small"); return M2V_E_OVERFLOW; }
    if (bytes) *bytes = (size_t)e->st().h_ctl->total_bytes;
    return M2V_OK;
}

static int resident_impl(m2v_enc *e, void *argp)
{
    auto *a = (ResidentArgs *)argp;
    // (the entry a refusal names: the _begin halves share the prefix)
    const char *fn = a->kind < 0 ? "m2v_encode_resident" : a->kind >= kPkRgb ? "m2v_encode_resident_rgb" : "m2v_encode_resident420";
    if (const int r = begin_sequence(e, fn, Entry::Resident, a->xs, a->ys, a->pf, a->n)) return r;
    if (a->n == 0) {                                    // no beat: the sequence never starts
        if (a->bytes) *a->bytes = 0;
        e->resident_empty = a->async;                   // only _begin leaves an _end to answer
        return M2V_OK;
    }
    hipStream_t s = a->s ? a->s : e->stream;
    const Geom &g = e->g;
    const size_t fb = (size_t)g.ysz * 3;
    // the control word is set up by the first chunk's k_frame_scan (no launch, no copy in front of the first kernel)
    if (!e->st().h_ctl) HIPCHK(hipHostMalloc((void **)&e->st().h_ctl, 2 * sizeof(StreamCtl)));
    ctl_begin(e, (unsigned long long)a->cap, true);
    const size_t chunk = std::max<size_t>(1, e->batch_frames);
    // align chunks to GOP boundaries so every chunk starts with an I frame where possible
    const size_t gop = e->pframes + 1u;
    size_t step = chunk >= gop ? chunk / gop * gop : chunk;
    if (seq_batch(e)) step = chunk;               // (a batch's GOPs count from their sequences' starts: there is no grid to align to)
    const SrcSize in = seq_frame_size(e);
    const int kind = a->kind < 0 && in.w ? kPk444 : a->kind;       // (planar 4:4:4 frames that have to be padded or resampled: through the handle's buffer too)
    const bool is420 = kind >= 0;                 // (or RGB)
    const size_t fb420 = is420 ? pk_frame_bytes(kind, g, in) : 0;
    if (e->seq.src.w) scale_prepare(e, s);
    if (is420) {
        // each chunk's frames are expanded or converted into planar 4:4:4 in front of its kernels, on the same stream; one buffer is enough because
        // the chunks are synchronised below
        e->d_x444.recorded = false;
        e->d_x444.ensure(std::min(step, a->n) * fb);
    }
    for (size_t k = 0; k < a->n; k += step) {
        const size_t nf = std::min(step, a->n - k);
        const bool first = k == 0, last = k + nf == a->n;
        const uint8_t *frames = is420 ? nullptr : a->d_in + k * fb;
        if (is420) {
            timer_break(e);
            launch_convert(e, s, kind, a->d_in + k * fb420, e->d_x444.p, (uint32_t)nf);
            e->x444_bytes = nf * fb;
            frames = e->d_x444.p;
        }
        if (e->seq.cut) scene_detect(e, s, frames, nf);        // option "scene_cut": the chunk's flags in front of its plan (waits for the device)
        encode_chunk(e, s, frames, nf, first, last, g.ysz / 4, a->d_out, /*advance=*/k > 0);
        if (!last) { HIPCHK(hipStreamSynchronize(s)); collect_chunk(e, e->st()); }    // the per-chunk work buffers are reused
    }
    mux_resident(e, s, a->d_out, a->cap, a->n);         // m2v_set_mux_out: the container out of the finished stream (nothing with no buffer set)
    HIPCHK(hipMemcpyAsync(e->st().h_ctl, e->d_ctl.p, sizeof(StreamCtl), hipMemcpyDeviceToHost, s));
    e->resident_inflight = true;
    e->resident_stream = s;
    if (a->async) return M2V_OK;
    return resident_end_impl(e, a->bytes);
}

int m2v_encode_resident(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count, const void *d_frames444,
                        size_t nframes, void *d_out, size_t cap, size_t *out_bytes, void *hip_stream)
{
    if (!e || (nframes && (!d_frames444 || !d_out))) return M2V_E_PARAM;
    ResidentArgs a{xsize16, ysize16, pframes_count, (const uint8_t *)d_frames444, nframes, (uint8_t *)d_out, cap, out_bytes,
                   (hipStream_t)hip_stream};
    return guard(e, resident_impl, &a);
}

int m2v_encode_resident_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count, const void *d_frames444,
                              size_t nframes, void *d_out, size_t cap, void *hip_stream)
{
    if (!e || (nframes && (!d_frames444 || !d_out))) return M2V_E_PARAM;
    ResidentArgs a{xsize16, ysize16, pframes_count, (const uint8_t *)d_frames444, nframes, (uint8_t *)d_out, cap, nullptr,
                   (hipStream_t)hip_stream, true};
    return guard(e, resident_impl, &a);
}

// 4:2:0 frames resident in HBM: the same sequence with k_expand420 in front of every chunk
int m2v_encode_resident420(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count, const void *d_frames420,
                           size_t nframes, int layout, void *d_out, size_t cap, size_t *out_bytes, void *hip_stream)
{
    if (!e || (nframes && (!d_frames420 || !d_out))) return M2V_E_PARAM;
    if (!layout420_ok(layout)) { e->set_err("m2v_encode_resident420: unknown layout %d", layout); return M2V_E_PARAM; }
    if ((uintptr_t)d_frames420 & 15) { e->set_err("m2v_encode_resident420: d_frames420 must be 16-byte aligned"); return M2V_E_PARAM; }
    ResidentArgs a{xsize16, ysize16, pframes_count, (const uint8_t *)d_frames420, nframes, (uint8_t *)d_out, cap, out_bytes,
                   (hipStream_t)hip_stream, false, kPk420 + layout};
    return guard(e, resident_impl, &a);
}

int m2v_encode_resident420_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count, const void *d_frames420,
                                 size_t nframes, int layout, void *d_out, size_t cap, void *hip_stream)
{
    if (!e || (nframes && (!d_frames420 || !d_out))) return M2V_E_PARAM;
    if (!layout420_ok(layout)) { e->set_err("m2v_encode_resident420_begin: unknown layout %d", layout); return M2V_E_PARAM; }
    if ((uintptr_t)d_frames420 & 15) { e->set_err("m2v_encode_resident420_begin: d_frames420 must be 16-byte aligned"); return M2V_E_PARAM; }
    ResidentArgs a{xsize16, ysize16, pframes_count, (const uint8_t *)d_frames420, nframes, (uint8_t *)d_out, cap, nullptr,
                   (hipStream_t)hip_stream, true, kPk420 + layout};
    return guard(e, resident_impl, &a);
}

// RGB frames resident in HBM: the same sequence with k_rgb2yuv in front of every chunk
static int resident_rgb(m2v_enc *e, const char *fn, ResidentArgs a, int layout, int matrix)
{
    if (!e) return M2V_E_PARAM;
    if (a.n && (!a.d_in || !a.d_out)) { e->set_err("%s: d_frames or d_out is NULL", fn); return M2V_E_PARAM; }
    if (!rgb_layout_ok(layout)) { e->set_err("%s: unknown layout %d", fn, layout); return M2V_E_PARAM; }
    if (!rgb_matrix_ok(matrix)) { e->set_err("%s: unknown matrix %d", fn, matrix); return M2V_E_PARAM; }
    if ((uintptr_t)a.d_in & 15) { e->set_err("%s: d_frames must be 16-byte aligned", fn); return M2V_E_PARAM; }
    a.kind = pk_rgb(layout, matrix);
    return guard(e, resident_impl, &a);
}

int m2v_encode_resident_rgb(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count, const void *d_frames,
                            size_t nframes, int layout, int matrix, void *d_out, size_t cap, size_t *out_bytes, void *hip_stream)
{
    return resident_rgb(e, "m2v_encode_resident_rgb", ResidentArgs{xsize16, ysize16, pframes_count, (const uint8_t *)d_frames, nframes,
                        (uint8_t *)d_out, cap, out_bytes, (hipStream_t)hip_stream, false}, layout, matrix);
}

int m2v_encode_resident_rgb_begin(m2v_enc *e, uint32_t xsize16, uint32_t ysize16, uint32_t pframes_count, const void *d_frames,
                                  size_t nframes, int layout, int matrix, void *d_out, size_t cap, void *hip_stream)
{
    return resident_rgb(e, "m2v_encode_resident_rgb_begin", ResidentArgs{xsize16, ysize16, pframes_count, (const uint8_t *)d_frames, nframes,
                        (uint8_t *)d_out, cap, nullptr, (hipStream_t)hip_stream, true}, layout, matrix);
}

int m2v_encode_resident_end(m2v_enc *e, size_t *out_bytes)
{
    if (!e) return M2V_E_PARAM;
    if (e->resident_empty && !e->resident_inflight) { e->resident_empty = false; if (out_bytes) *out_bytes = 0; return M2V_OK; }
    return guard(e, resident_end_impl, out_bytes);
}

}  // extern "C"
