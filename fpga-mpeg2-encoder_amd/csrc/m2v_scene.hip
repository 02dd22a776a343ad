// m2v_scene.hip — where GOPs start, host side.  The module starts a GOP every pframes_count + 1 frames from frame 0; here a GOP also
// starts where the caller says (m2v_set_gop_starts) or where the device finds a scene cut (option "scene_cut").  GOPs are closed, an I
// picture resets temporal_reference and the GOP header's time code is a function of the frame number alone, so the stream is the splice
// of the GOPs encoded alone.  Neither entry is the module's behaviour.
//
//   the rule               GopRule (m2v_host.hpp): one definition, stepped frame by frame by plan_chunk (the handle carries s and k across
//                          chunks) and by m2v_gop_layout.  The whole-frame kernels take a picture's place in its GOP from
//                          FrameJob::i_frame and FrameJob::n, so plan_chunk's jobs are all that changes; k_mb is untouched.
//   option "scene_cut"     resident entries, per chunk: the conversion as ever, then k_mbsum (m2v_scene_kernels.hpp: the luma sum of every
//                          macroblock, each byte read once) and k_scene_judge (one block per frame: the sum of |difference| to the frame
//                          before against T * mbs) write {D, flag} per frame into pinned memory; the host waits for that - the one wait the
//                          feature adds per chunk - and plans the chunk with the flags.  The sums of a chunk's last frame wait for the
//                          next chunk in one half of d_carry while that chunk leaves its own in the other half.
#include "m2v_host.hpp"

static_assert(sizeof(m2v_scene_stat) == 16, "the record of include/m2v_mi355x.h is 16 bytes");

namespace m2v {

void scene_detect(m2v_enc *e, hipStream_t s, const uint8_t *d_frames, size_t nf)
{
    const Geom &g = e->g;
    e->d_mbsum.recorded = e->d_carry.recorded = e->d_scene.recorded = false;
    e->d_mbsum.ensure(nf * (size_t)g.mbs);
    e->d_scene.ensure(nf * sizeof(SceneRec));
    if (e->d_carry.n < 2 * (size_t)g.mbs) {
        if (e->carry_cur >= 0) throw HipError{hipErrorInvalidValue, "scene carry lost on geometry change"};
        e->d_carry.ensure(2 * (size_t)g.mbs);
    }
    if (e->h_scene_cap < nf * sizeof(SceneRec)) {         // (free: the wait below is behind every earlier judge)
        if (e->h_scene) (void)hipHostFree(e->h_scene);
        e->h_scene = nullptr; e->h_scene_cap = 0;
        HIPCHK(hipHostMalloc((void **)&e->h_scene, nf * sizeof(SceneRec)));
        e->h_scene_cap = nf * sizeof(SceneRec);
    }
    if (!e->ev_scene) HIPCHK(hipEventCreateWithFlags(&e->ev_scene, hipEventDisableTiming | hipEventReleaseToSystem));
    const int out = e->carry_cur == 0 ? 1 : 0;
    {
        Timer t(e, s, 5, (double)nf * g.ysz);
        launch_mbsum(e, s, d_frames, nf);
        launch_scene_judge(e, s, nf, (unsigned long long)e->seq.cut * (unsigned long long)g.mbs,
                           e->carry_cur < 0 ? nullptr : e->d_carry.p + (size_t)e->carry_cur * (size_t)g.mbs,
                           e->d_carry.p + (size_t)out * (size_t)g.mbs, e->h_scene);
        t.stop();
    }
    timer_break(e);
    e->carry_cur = out;
    HIPCHK(hipEventRecord(e->ev_scene, s));
    HIPCHK(hipEventSynchronize(e->ev_scene));
    const SceneRec *r = (const SceneRec *)e->h_scene;
    e->chunk_cut.resize(nf);
    e->chunk_diff.resize(nf);
    for (size_t k = 0; k < nf; ++k) { e->chunk_cut[k] = (uint8_t)(r[k].flag != 0); e->chunk_diff[k] = r[k].diff; }
}

void scene_release(m2v_enc *e)
{
    e->d_mbsum.release(); e->d_carry.release(); e->d_scene.release();
    if (e->ev_scene) (void)hipEventDestroy(e->ev_scene);
    if (e->h_scene) (void)hipHostFree(e->h_scene);
    e->ev_scene = nullptr; e->h_scene = nullptr; e->h_scene_cap = 0;
}

static bool ascending(const uint32_t *f, size_t n)
{
    for (size_t k = 1; k < n; ++k) if (f[k] <= f[k - 1]) return false;
    return true;
}

}  // namespace m2v

extern "C" {

int m2v_set_gop_starts(m2v_enc *e, const uint32_t *frames, size_t n)
{
    if (!e) return M2V_E_PARAM;
    if (!frames || !n) { e->set.gop_starts.clear(); return M2V_OK; }
    if (!ascending(frames, n)) {
        e->set_err("m2v_set_gop_starts: the list must be strictly ascending frame numbers (the previous setting stays)");
        return M2V_E_PARAM;
    }
    try { e->set.gop_starts.assign(frames, frames + n); }
    catch (...) { e->set_err("m2v_set_gop_starts: host allocation failed"); return M2V_E_NOMEM; }
    return M2V_OK;
}

long long m2v_gop_layout(uint32_t pframes_count, const uint32_t *starts, size_t n, size_t nframes, uint8_t *flags_out)
{
    if (!starts) n = 0;
    if (!ascending(starts, n)) return M2V_E_PARAM;
    GopRule r{pframes_count & 0xFFu, starts, n, 0, 0, 0};
    for (size_t f = 0; f < nframes; ++f) {
        const uint32_t fl = r.step(f, false);
        if (flags_out) flags_out[f] = (uint8_t)fl;
    }
    return (long long)r.k;
}

long long m2v_scene_report(m2v_enc *e, m2v_scene_stat *dst, size_t cap)
{
    if (!e) return M2V_E_PARAM;
    return (long long)e->scene_q.pop(dst, cap);
}

}  // extern "C"
