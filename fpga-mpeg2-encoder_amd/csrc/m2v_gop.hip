// m2v_gop.hip — a level per GOP, host side.  GOPs are closed (closed_gop = 1, RTL:2656) and the level appears in the stream in one place
// only, the quantiser_scale_code of the slice headers, which ISO/IEC 13818-2 lets change from slice to slice: a GOP coded at level q is
// byte for byte the GOP of the whole sequence coded at q.  Neither entry below is the module's behaviour.
//
//   m2v_set_gop_levels     the caller's schedule: GOP k of a sequence at levels[min(k, n - 1)].  plan_chunk writes the level into
//                          FrameJob::q (k_assemble prints it) and partitions every launch list by level; launch_mb_levels then issues one
//                          k_mb launch per level present, each with a Geom whose Q is that level.  k_mb is untouched.
//   option "gop_bytes_max" the cap, resident entries: behind the chunk's steps and k_slice_scan, k_gop_judge (m2v_gop_kernels.hpp) sums
//                          every GOP's bytes on the device, writes its record to pinned memory and raises FrameJob::q of a GOP that is
//                          over.  The host waits for that verdict - the only wait the feature adds, at most three per chunk - builds the
//                          launch lists of those GOPs behind the plan's own in d_lists / d_joblist, runs their steps again one level up on
//                          the call's stream, scans their slices again and asks for the next verdict.  A GOP's two reconstruction slots are
//                          its own, so the others are not disturbed.  k_frame_scan and k_assemble run once, at the end, as ever.
//                          The search goes up one level at a time and stops at the first fit; the result depends on the clip alone.
#include "m2v_host.hpp"

static_assert(sizeof(m2v_gop_stat) == 32, "the record of include/m2v_mi355x.h is 32 bytes");

namespace m2v {

void gop_cap_chunk(m2v_enc *e, hipStream_t s)
{
    const Geom &g = e->g;
    const size_t nf = e->plan_nf, gop = e->pframes + 1u, nseg = (nf + gop - 1) / gop;
    m2v_enc::HostStage &h = e->st();
    timer_break(e);
    if (!e->slice_scan_done) launch_slice_scan(e, s, g, 0, (int)nf);
    e->slice_scan_done = true;
    e->d_gop.recorded = false;
    e->d_gop.ensure(nseg);
    HIPCHK(hipMemsetAsync(e->d_gop.p, 0, nseg * sizeof(m2v_gop_stat), s));
    if (h.h_gop_cap < nseg) {            // (the stage is free: its previous chunk has completed)
        if (h.h_gop) (void)hipHostFree(h.h_gop);
        h.h_gop = nullptr; h.h_gop_cap = 0;
        HIPCHK(hipHostMalloc((void **)&h.h_gop, nseg * sizeof(m2v_gop_stat)));
        h.h_gop_cap = nseg;
    }
    h.ngop = nseg;
    if (!e->ev_gop) HIPCHK(hipEventCreateWithFlags(&e->ev_gop, hipEventDisableTiming | hipEventReleaseToSystem));
    // GOPs whose verdict is still open, and the level each was last coded at (the plan's: every frame of a GOP has one level)
    std::vector<int> open(nseg);
    std::vector<uint8_t> level(nseg);
    for (size_t sg = 0; sg < nseg; ++sg) { open[sg] = (int)sg; level[sg] = (uint8_t)e->dev_jobs[sg * gop].q; }
    const size_t base = e->plan_nlists;
    for (;;) {
        launch_gop_judge(e, s, nf, (uint32_t)gop, e->seq.cap, h.h_gop);
        // nothing to wait for once every open GOP is at level 4: whatever the verdict, it stays (the records travel with the chunk)
        open.erase(std::remove_if(open.begin(), open.end(), [&](int sg) { return level[(size_t)sg] >= 4; }), open.end());
        if (open.empty()) break;
        HIPCHK(hipEventRecord(e->ev_gop, s));
        HIPCHK(hipEventSynchronize(e->ev_gop));
        open.erase(std::remove_if(open.begin(), open.end(), [&](int sg) { return !h.h_gop[sg].over; }), open.end());
        if (open.empty()) break;
        // the device has raised FrameJob::q of these GOPs: what plan_chunk remembers of d_jobs no longer describes it
        e->dev_jobs_p = nullptr;
        for (int sg : open) ++level[(size_t)sg];
        std::stable_sort(open.begin(), open.end(), [&](int x, int y) { return level[(size_t)x] < level[(size_t)y]; });
        // their launch lists, step by step (the I frames, then the P frames), each partitioned by level like the plan's
        const size_t lists_bytes = (nf * sizeof(int) + 15) & ~(size_t)15;
        ensure_pinned(e->h_redo, e->h_redo_cap, lists_bytes + nf * sizeof(FrameJob));      // (free: the wait above is behind the last try's copies)
        int *const hl = (int *)e->h_redo;
        FrameJob *const hj = (FrameJob *)(e->h_redo + lists_bytes);
        struct Redo { int off_i, n_i, off_p, n_p; };
        std::vector<Redo> steps(gop);
        size_t n = 0;
        for (size_t j = 0; j < gop; ++j) {
            Redo &r = steps[j];
            for (int pass = 0; pass < 2; ++pass) {
                const size_t off = n;
                for (int sg : open) {
                    const size_t f = (size_t)sg * gop + j;
                    if (f >= nf || (e->dev_jobs[f].i_frame == 0) != (pass == 0)) continue;
                    hl[n] = (int)f;
                    hj[n] = e->dev_jobs[f];
                    hj[n].fidx = (uint32_t)f;
                    e->plan_list_q[base + n] = level[(size_t)sg];
                    ++n;
                }
                if (pass == 0) { r.off_i = (int)(base + off); r.n_i = (int)(n - off); }
                else { r.off_p = (int)(base + off); r.n_p = (int)(n - off); }
            }
        }
        HIPCHK(hipMemcpyAsync(e->d_lists.p + base, hl, n * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->d_joblist.p + base, hj, n * sizeof(FrameJob), hipMemcpyHostToDevice, s));
        // option "stats": the records of a GOP that goes again are those of its final level
        if (e->stats_on)
            for (int sg : open) {
                const size_t a = (size_t)sg * gop, b = std::min(a + gop, nf);
                HIPCHK(hipMemsetAsync(e->d_pstat.p + a, 0, (b - a) * sizeof(m2v_picture_stat), s));
            }
        for (size_t j = 0; j < gop; ++j) {
            const Redo &r = steps[j];
            launch_mb_levels<false>(e, s, r.off_i, r.n_i);
            launch_mb_levels<true>(e, s, r.off_p, r.n_p);
            if (e->stats_on) {
                timer_break(e);
                launch_picstat(e, s, e->d_lists.p + r.off_i, r.n_i);
                launch_picstat(e, s, e->d_lists.p + r.off_p, r.n_p);
            }
            // m2v_set_recon_out: the frames of a GOP that goes again are overwritten by those of its final level
            if (e->seq.recon.p) {
                launch_recon_out(e, s, e->d_lists.p + r.off_i, r.n_i);
                launch_recon_out(e, s, e->d_lists.p + r.off_p, r.n_p);
            }
        }
        timer_break(e);
        for (int sg : open) {
            const size_t a = (size_t)sg * gop, b = std::min(a + gop, nf);
            launch_slice_scan(e, s, g, (int)a, (int)b);
        }
        HIPCHK(hipGetLastError());
    }
}

}  // namespace m2v

extern "C" {

int m2v_set_gop_levels(m2v_enc *e, const uint8_t *levels, size_t n)
{
    if (!e) return M2V_E_PARAM;
    if (!levels || !n) { e->set.gop_levels.clear(); return M2V_OK; }
    for (size_t k = 0; k < n; ++k)
        if (levels[k] < 1 || levels[k] > 4) {
            e->set_err("m2v_set_gop_levels: levels[%zu] = %u, a level is 1..4 (the previous setting stays)", k, (unsigned)levels[k]);
            return M2V_E_PARAM;
        }
    try { e->set.gop_levels.assign(levels, levels + n); }
    catch (...) { e->set_err("m2v_set_gop_levels: host allocation failed"); return M2V_E_NOMEM; }
    return M2V_OK;
}

long long m2v_gop_report(m2v_enc *e, m2v_gop_stat *dst, size_t cap)
{
    if (!e) return M2V_E_PARAM;
    return (long long)e->gop_q.pop(dst, cap);
}

}  // extern "C"
