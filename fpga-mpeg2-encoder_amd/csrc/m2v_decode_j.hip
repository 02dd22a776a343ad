// m2v_decode_j.hip — streams cut from a broadcast for m2v_decode_device (option "decode_join" = 1 .. 3 on top of "decode_interlaced",
// "decode_extended", "decode_mb_tools" and "decode_field_pictures" = 1, with "decode_b_pictures" 0 or 1).  m2v_decode.hip keeps the
// scan - whatever lies in front of the join point is just events -, and everything behind the plan's wait is dec_f_chunks of
// m2v_decode_f.hip with its kernels: this unit holds the plan alone, in k_df_plan's place.  decoder.decode(..., join=) is the definition;
// every function that decides an index or a verdict is a j_ (or fp_ ...) function of m2v_decode_kernels.hpp.
//
//   k_dj_plan    J: the first sequence_header_code, a minimum over the lanes.  The events from J on are cut into 256 ranges.  Every lane
//                sums the pairing of its range for both states in front of it (dec::j_pair_range), lane 0 joins the sums
//                (dec::j_pair_join): the state in front of every range, F - the last picture start code that begins a frame -, and E2,
//                the picture that begins the second anchor frame.  T follows from the last slice in front of F.  Then k_df_plan's
//                text runs over the window's events with T as the stream's length, but for the frames that are dropped - a frame whose
//                first picture is a B picture in front of E2 -: their events are judged, their pictures are in no sum and no table,
//                their slices are not counted (dec::j_keep_range, dec::j_place).  Event indices that leave the kernel are those of the
//                whole list, so the slice walk, the matrices and the spans of dec_f_chunks find the kept pictures' events where they are.
#include "m2v_decode_state.hpp"

namespace m2v {

constexpr uint32_t kNoPicJ = 0xFFFFFFFFu;

__global__ __launch_bounds__(kDecThreads) void k_dj_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev0, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecFPic *bp, int b_pictures, int join, uint32_t *h_mbh, uint32_t *h_sl)
{
    __shared__ dec::MainPlan s_P, s_Pf;                    // s_Pf: with a field's macroblock rows
    __shared__ unsigned long long s_bad, s_T, s_lnz;
    __shared__ dec::JSum s_A[kDecThreads], s_B[kDecThreads];
    __shared__ dec::JPair s_pin[kDecThreads];
    __shared__ dec::FpRange s_K[kDecThreads], s_in[kDecThreads], s_all;
    __shared__ uint32_t s_m[kDecThreads], s_cp[kDecThreads], s_ng[kDecThreads], s_nr[kDecThreads], s_ncp;
    __shared__ int s_sig[kDecThreads];
    __shared__ uint32_t s_ns[kDecThreads], s_mi[kDecThreads], s_mn[kDecThreads], s_rs[kDecThreads], s_slices;
    __shared__ uint32_t s_jev, s_f, s_e2, s_s, s_tw, s_gone, s_lastopen, s_lastpic, s_cut;
    const uint32_t tid = threadIdx.x, nev0 = st->nev;
    const bool head = (join & (int)dec::kJoinHead) != 0, tail = (join & (int)dec::kJoinTail) != 0, drop = head && b_pictures != 0;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (tid == 0) {                                // the join record of a call that drops nothing: 0, es_bytes, 0, 0
        uint32_t *j = h_mbh + kDecJoinWord;
        j[0] = j[1] = 0; j[2] = (uint32_t)n; j[3] = (uint32_t)(n >> 32); j[4] = j[5] = 0;
    }
    if (st->status == dec::kEvents) {              // the list was too small: the call runs again with the count
        if (tid == 0) { r.status = dec::kEvents; r.pictures = nev0; *h_rec = r; }
        return;
    }
    if (tid == 0) { s_jev = head ? nev0 : 0u; s_bad = dec::kNone; s_s = 0; s_gone = 0; s_lastopen = 0; s_lastpic = 0; }
    __syncthreads();
    if (head) {                                    // J: the first sequence header of any range
        const uint32_t per0 = (nev0 + kDecThreads - 1) / kDecThreads, a0 = min(nev0, tid * per0), b0 = min(nev0, a0 + per0);
        const uint32_t j = dec::j_first_seq((const uint64_t *)ev0, a0, b0);
        if (j != dec::kNoEvent) atomicMin(&s_jev, j);
    }
    __syncthreads();
    const uint32_t jev = s_jev;
    if (jev >= nev0 && (head || !nev0)) {          // no sequence header (no start code at all)
        if (tid == 0) { st->status = dec::kSyntax; st->err = 0; r.status = dec::kSyntax; r.err_offset = 0; *h_rec = r; }
        return;
    }
    const unsigned long long *ev = ev0 + jev;      // from here on an event's index counts from J's
    const uint32_t nw = nev0 - jev;
    const uint32_t per = (nw + kDecThreads - 1) / kDecThreads, a = min(nw, tid * per), b = min(nw, a + per);
    {   // the last significant event of every range, in the whole stream: whether it ends with sequence_end_code
        int sig = -1;
        for (uint32_t i = a; i < b; ++i) if (dec::main_significant(dec::main_role(es, n, ev[i]))) sig = (int)i;
        s_sig[tid] = sig;
    }
    __syncthreads();
    if (tid == 0) {
        int last = -1;
        for (int k = kDecThreads - 1; k >= 0 && last < 0; --k) last = s_sig[k];
        s_cut = tail && !(last >= 0 && dec::main_role(es, n, ev[last]) == dec::rEnd);
    }
    __syncthreads();
    const bool cut = s_cut != 0;
    {   // the pairing of everything behind J
        dec::JSum A, B;
        dec::j_pair_range(es, n, (const uint64_t *)ev, nw, a, b, b_pictures != 0, A, B);
        s_A[tid] = A; s_B[tid] = B;
    }
    __syncthreads();
    if (tid == 0) {
        dec::JScan t = dec::j_scan_none();
        for (int k = 0; k < kDecThreads; ++k) {
            s_pin[k] = t.in;
            dec::j_pair_join(t, s_A[k], s_B[k]);
        }
        s_f = cut ? t.f : dec::kNoEvent; s_e2 = t.e2;
        s_tw = s_f != dec::kNoEvent ? s_f : nw;
    }
    __syncthreads();
    const uint32_t F = s_f, e2 = s_e2;
    if (F != dec::kNoEvent) {                      // T: the first GOP or picture header behind the last slice in front of F (event 0 is J's)
        const uint32_t sl = dec::j_last_slice((const uint64_t *)ev, a, min(b, F));
        if (sl != dec::kNoEvent) atomicMax(&s_s, sl);
        __syncthreads();
        const uint32_t hd = dec::j_first_head((const uint64_t *)ev, max(a, s_s + 1u), min(b, F + 1u));
        if (hd != dec::kNoEvent) atomicMin(&s_tw, hd);
        __syncthreads();
    }
    const uint32_t tw = s_tw, nev = tw;            // the window: events [0, tw), bytes [J, T)
    if (tid == 0) {
        s_T = tw < nw ? dec::ev_pos(ev[tw]) : n;
        s_lnz = tw < nw ? dec::j_last_nz(es, s_T, (const uint64_t *)ev, tw) : st->last_nz;
        s_bad = head ? dec::j_first(es, s_T, (const uint64_t *)ev, tw, s_P) : dec::il_first(es, s_T, (const uint64_t *)ev, tw, s_P);
        s_Pf = s_P;
        s_Pf.mbh = s_P.mbh / 2u;
    }
    __syncthreads();
    const unsigned long long T = s_T;
    if (s_bad != dec::kNone) {
        if (tid == 0) { st->status = dec::kSyntax; st->err = s_bad; r.status = dec::kSyntax; r.err_offset = s_bad; *h_rec = r; }
        return;
    }
    const dec::MainPlan &P = s_P;
    const uint32_t progressive = P.seq.h.progressive;
    if (tid < 64) { mats[tid] = P.seq.wi[tid]; mats[64 + tid] = P.seq.wn[tid]; }
    const unsigned long long last_nz = s_lnz;
    const uint32_t aw = min(a, tw), bw = min(b, tw);
    __syncthreads();                               // (s_sig is written again)
    {   // the last significant event of every range of the window
        int sig = -1;
        for (uint32_t i = aw; i < bw; ++i) if (dec::main_significant(dec::main_role(es, T, ev[i]))) sig = (int)i;
        s_sig[tid] = sig;
    }
    __syncthreads();
    {
        int prev = -1;                             // the significant event in front of this range
        for (int k = (int)tid - 1; k >= 0 && prev < 0; --k) prev = s_sig[k];
        unsigned long long bad = dec::kNone;
        uint32_t ng = 0, nr = 0, reset = 0;
        dec::XMats xm{dec::kNoEvent, dec::kNoEvent};           // what the range's events loaded behind its last sequence header
        for (uint32_t i = aw; i < bw; ++i) {
            const dec::EvInfo f = dec::fp_event(es, T, (const uint64_t *)ev, nev, i, P, s_Pf, last_nz, prev, b_pictures != 0);
            const int role = dec::main_role(es, T, ev[i]);
            if (dec::main_significant(role)) prev = (int)i;
            reset |= role == dec::rSeq;
            dec::x_mats_event(es, T, (const uint64_t *)ev, nev, i, xm);
            bad = dec::min64(bad, f.bad);
            ng += f.gop; nr += f.rep;
        }
        if (bad != dec::kNone) atomicMin(&s_bad, bad);
        dec::JKeep K;                              // the range's kept pictures: the state in front of it is known
        dec::j_keep_range(es, T, (const uint64_t *)ev, nev, aw, bw, b_pictures != 0, s_pin[tid], e2, drop, K);
        s_K[tid] = K.r; s_m[tid] = K.m;
        if (K.dropped) atomicAdd(&s_gone, K.dropped);
        s_ng[tid] = ng; s_nr[tid] = nr; s_ns[tid] = K.ns; s_mi[tid] = xm.mi; s_mn[tid] = xm.mn; s_rs[tid] = reset;
    }
    __syncthreads();
    if (tid == 0) {                                // the sums in front of every range, joined in order
        uint32_t ng = 0, nr = 0, ns = 0, mi = dec::kNoEvent, mn = dec::kNoEvent, cp = 0;
        dec::FpRange all = dec::fp_range_none();
        for (int k = 0; k < kDecThreads; ++k) {
            const uint32_t sl = s_ns[k], ki = s_mi[k], kn = s_mn[k];
            s_in[k] = all; s_cp[k] = cp;
            s_ns[k] = ns; s_mi[k] = mi; s_mn[k] = mn;
            ns += sl;
            if (s_rs[k]) { mi = ki; mn = kn; }         // a sequence header in the range: only what was loaded behind it
            else { if (ki != dec::kNoEvent) mi = ki; if (kn != dec::kNoEvent) mn = kn; }
            dec::fp_join(all, cp, s_K[k], s_K[k], s_m[k]);     // (one sum: the lane knew what waited in front of it)
            ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = all.frames; r.gops = ng; r.repeated_headers = nr; r.chains = all.ni;
        s_all = all; s_ncp = cp; s_slices = ns;
    }
    __syncthreads();
    {
        dec::FpRange s = s_in[tid];
        dec::JPair w = s_pin[tid];
        bool gone = dec::j_dropped(w, e2, drop);               // whether the picture in front of event i is a dropped one
        uint32_t cp = s_cp[tid];
        uint32_t sl = s_ns[tid];                               // the kept pictures' slice events in front of event i
        dec::XMats xm{s_mi[tid], s_mn[tid]};                   // the matrices in force in front of event i
        for (uint32_t i = aw; i < bw; ++i) {
            const uint32_t code = dec::ev_code(ev[i]);
            const unsigned long long pos = dec::ev_pos(ev[i]);
            if (code != 0x00) {
                if (code <= 0xAFu) sl += !gone;
                else if (code == 0xB3u || code == 0xB5u) dec::x_mats_event(es, T, (const uint64_t *)ev, nev, i, xm);
                if (w.open && (code == 0xB3u || code == 0xB8u || code == 0xB7u)) atomicMin(&s_bad, pos);      // between the two fields of a frame
                continue;
            }
            uint32_t type, tref, ps;
            if (!dec::fp_is_picture(es, T, (const uint64_t *)ev, nev, i, b_pictures != 0, type, tref, ps)) continue;
            bool wrong;
            gone = dec::j_place(w, i, ps, type, tref, e2, drop, wrong);
            atomicMax(&s_lastpic, i + 1u);
            if (w.open) atomicMax(&s_lastopen, i + 1u);
            if (gone) { if (wrong) atomicMin(&s_bad, pos); continue; }
            const int32_t anchor_cp = s.a1cp;
            const dec::FpPlace q = dec::fp_place(s, cp, ps, type, tref);
            if (q.bad) atomicMin(&s_bad, pos);
            if (cp < pic_cap) {
                uint32_t slice0, nslices, quant;
                dec::FPicParams pp = dec::fp_picture_params(es, T, (const uint64_t *)ev, nev, i, b_pictures != 0, progressive, slice0, nslices, quant);
                pp.second = q.second; pp.noref = q.second && type == 2u && q.fwd == kNoPicJ;
                const dec::XMats own = dec::x_mats_picture(es, T, (const uint64_t *)ev, nev, xm, quant);
                DecFPic *d = bp + cp;                          // (field by field: an anchor frame's display index is another lane's to write)
                d->slice0 = slice0 + jev; d->params = dec::fp_params_pack(pp); d->fwd = q.fwd; d->bwd = q.bwd; d->nslices = nslices; d->sbase = sl;
                d->mi = own.mi == dec::kNoEvent ? own.mi : own.mi + jev; d->mn = own.mn == dec::kNoEvent ? own.mn : own.mn + jev; d->frame = q.frame;
                if (q.second) d->display = 0;
                else if (type == 3u) d->display = dec::bp_display_b(q.frame);
                h_sl[cp] = sl;
                pics[cp] = DecPic{i + jev, type, 0u, 0u};
                h_types[cp] = (uint8_t)(type | pp.ps << 2 | q.second << 4);
            }
            if (!q.second && type != 3u && anchor_cp >= 0 && (uint32_t)anchor_cp < pic_cap) bp[anchor_cp].display = dec::bp_display_anchor(q.frame);
            ++cp;
        }
    }
    __syncthreads();
    if (tid) return;
    if (s_lastopen && s_lastopen == s_lastpic) s_bad = dec::min64(s_bad, dec::ev_pos(ev[s_lastopen - 1u]));      // a first field no picture follows
    const dec::FpRange &all = s_all;
    if (all.a1cp >= 0 && (uint32_t)all.a1cp < pic_cap) bp[all.a1cp].display = dec::bp_display_anchor(all.frames);      // the last anchor frame
    const dec::SeqHdr &h = P.seq.h;
    r.width = h.width; r.height = h.height;
    r.frame_bytes = dec::frame_bytes(h.width, h.height);
    if (s_bad != dec::kNone) { r.status = dec::kSyntax; r.err_offset = s_bad; }
    else if (s_ncp > pic_cap) { r.status = dec::kSyntax; r.err_offset = 0; }           // (cannot happen: a picture is three events at least)
    else if (!probe && r.frame_bytes * r.pictures > cap) r.status = dec::kOverflow;
    else if (probe) r.out_bytes = r.frame_bytes * r.pictures;
    st->status = r.status; st->err = s_bad; st->npics = r.pictures; st->gops = r.gops; st->reps = r.repeated_headers; st->chains = r.chains;
    st->width = r.width; st->height = r.height; st->mbw = P.mbw; st->mbh = P.mbh; st->frame_bytes = r.frame_bytes;
    h_mbh[0] = P.mbh; h_mbh[1] = s_ncp;
    if (s_ncp <= pic_cap) h_sl[s_ncp] = s_slices;
    if (r.status != dec::kSyntax) {                // the join record: the join point, the tail's offset, the frames dropped
        const unsigned long long J = dec::ev_pos(ev[0]);
        uint32_t *j = h_mbh + kDecJoinWord;
        j[0] = (uint32_t)J; j[1] = (uint32_t)(J >> 32); j[2] = (uint32_t)T; j[3] = (uint32_t)(T >> 32);
        j[4] = s_gone; j[5] = tw < nw ? 1u : 0u;
    }
    *h_rec = r;
}

void dec_j_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int join, uint32_t *h_mbh, uint32_t *h_sl)
{
    k_dj_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecFPic *)(d_main + kDecMainMatrices), b_pictures, join, h_mbh,
                                        h_sl);
    HIPCHK(hipGetLastError());
}

}  // namespace m2v
