// m2v_decode_c.hip — damaged slices concealed for m2v_decode_device (option "decode_conceal" = 1 on top of "decode_interlaced",
// "decode_extended", "decode_mb_tools" and "decode_field_pictures" = 1, with "decode_b_pictures" 0 or 1 and "decode_join" 0 .. 3).
// m2v_decode.hip keeps the scan, and the chunks are dec_f_chunks of m2v_decode_f.hip with its reconstruction and output: a concealed
// macroblock is a record, and k_df_recon draws it as any other.  This unit holds the plan and what stands between the plan and the
// reconstruction of a chunk.
// decoder.decode(..., conceal=True) is the definition; every function that decides a bit, a verdict or a record is a c_ (or fp_ / t_ ..)
// function of m2v_decode_kernels.hpp.
//
//   k_dc_plan    k_dj_plan's text with dec::c_event and dec::c_place: a slice behind a coding extension or a slice whatever the codes, a
//                picture that ends behind any slice or none, an I picture with a P picture's forward frame; nslices may be 0
//   k_dc_slices  k_df_slices' text: one lane per slice EVENT of the chunk into the records of the row its code names.  It refuses
//                nothing: a slice whose code is above its picture's rows is not walked, and its span, like that of a slice that does not
//                read, says so.  A walk writes inside the row its code names alone (the column is below mbw before every store), so
//                whatever a damaged slice leaves lies in a row that k_dc_rows conceals whole
//   k_dc_rows    in k_df_cont's place: a block per coded picture of the chunk, a lane per macroblock row.  The lane walks the picture's
//                spans (dec::c_row_kept); for a concealed row it writes the mbw records (dec::c_record).  The counts are summed over
//                the wavefront by shuffles and added to DecState by lane 0, one atomic a count and block; the first damaged picture's
//                start code is a minimum
//   k_dc_finish  k_df_finish, and the report beside the record
#include "m2v_decode_state.hpp"

namespace m2v {

// k_dj_plan's text (m2v_decode_j.hip; join 0: the window is the stream, and the plan is k_df_plan's) with the relaxed rules: an event is
// judged by dec::c_event - no rule reads the rows, so there is no second plan with a field's -, a picture placed by dec::c_place.
// The text stands twice because as a template the instantiation the other paths run did not keep its registers and scratch: a fix
// made in k_dj_plan is to be made here too, and the other way round
__global__ __launch_bounds__(kDecThreads) void k_dc_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev0, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecFPic *bp, int b_pictures, int join, uint32_t *h_mbh, uint32_t *h_sl)
{
    __shared__ dec::MainPlan s_P;
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
    if (tid == 0) {                                // the join record of a call that drops nothing: 0, es_bytes, 0, 0 (read with "decode_join" alone)
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
            const dec::EvInfo f = dec::c_event(es, T, (const uint64_t *)ev, nev, i, P, last_nz, prev, b_pictures != 0);
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
            const dec::FpPlace q = dec::c_place(s, cp, ps, type, tref);
            if (q.bad) atomicMin(&s_bad, pos);
            if (cp < pic_cap) {
                uint32_t slice0, nslices, quant;
                dec::FPicParams pp = dec::fp_picture_params(es, T, (const uint64_t *)ev, nev, i, b_pictures != 0, progressive, slice0, nslices, quant);
                pp.second = q.second; pp.noref = q.second && type == 2u && q.fwd == kNoPic;
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
    else if (s_ncp > pic_cap) { r.status = dec::kSyntax; r.err_offset = 0; }           // (cannot happen: a picture is two events at least, and the table is sized so)
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

__global__ __launch_bounds__(64) void k_dc_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, const DecState *__restrict__ st,
                                                  const DecPic *__restrict__ pics, const DecFPic *__restrict__ xp, uint32_t p0, uint32_t np, uint32_t f0, uint32_t total,
                                                  dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *__restrict__ spans)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, nev = st->nev;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= total) return;
    uint32_t k;
    const uint32_t pic = dec::x_slice_pic(xp + p0, np, g, k);          // (pictures without a slice share their sbase with the next one: the search passes them)
    const DecPic P = pics[p0 + pic];
    const DecFPic Q = xp[p0 + pic];
    const uint32_t i = Q.slice0 + k;
    spans[g] = 0u;
    if (k >= Q.nslices || i >= nev || Q.frame < f0) return;            // (the plan counted the picture's slices: they are there)
    const unsigned long long start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : n;
    const uint32_t code = dec::ev_code(ev[i]);
    const dec::FPicParams pp = dec::fp_params_unpack(Q.params);
    const bool field = dec::fp_is_field(pp.ps);
    const uint32_t rows = field ? mbh / 2u : mbh;
    spans[g] = dec::x_span_pack(false, code, -1, -1);
    if (dec::c_bad_code(code, rows)) return;                           // a bad slice: counted behind the walk, not walked
    const size_t first = df_first(Q, f0, mbw * mbh) + (size_t)(code - 1u) * mbw;
    IMbSink sink{mb + first, dc + first * 6, lv + first * 384};
    int c0, c1;
    const bool ok = field ? dec::fp_slice(es, start, end, P.type, pp, (int)mbw, (int)rows, (int)code - 1, sink, c0, c1)
                          : dec::t_slice(es, start, end, P.type, pp.t, (int)mbw, (int)mbh, (int)code - 1, sink, c0, c1);
    spans[g] = dec::x_span_pack(ok, code, c0, c1);
}

// grid: the coded pictures [p0, p0 + gridDim.x) of the chunk that begins at frame f0; spans: the chunk's, picture p's from sbase on
__global__ __launch_bounds__(64) void k_dc_rows(const unsigned long long *__restrict__ ev, DecState *st, const DecPic *__restrict__ pics, const DecFPic *__restrict__ xp,
                                                uint32_t p0, uint32_t f0, dec::IMb *mb, const uint32_t *__restrict__ spans)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, l = threadIdx.x;
    const DecFPic Q = xp[p0 + blockIdx.x];
    if (Q.frame < f0) return;
    const dec::FPicParams pp = dec::fp_params_unpack(Q.params);
    const bool field = dec::fp_is_field(pp.ps);
    const uint32_t rows = field ? mbh / 2u : mbh, par = field ? pp.ps - 1u : 0u;
    const uint32_t *sp = spans + (Q.sbase - xp[p0].sbase);
    const bool grey = Q.fwd == kNoPic;                                 // no frame in front: the first anchor frame, both of its fields
    uint32_t bad = 0, hidden = 0;
    for (uint32_t k = l; k < Q.nslices; k += 64u) bad += !(sp[k] >> 31);
    const dec::IMb rec = dec::c_record(field, par, grey);
    dec::IMb *at = mb + df_first(Q, f0, mbw * mbh);
    for (uint32_t r = l; r < rows; r += 64u) {
        if (dec::c_row_kept(sp, Q.nslices, r + 1u, mbw)) continue;
        for (uint32_t c = 0; c < mbw; ++c) at[(size_t)r * mbw + c] = rec;
        ++hidden;
    }
    for (int o = 32; o; o >>= 1) { bad += __shfl_down(bad, o); hidden += __shfl_down(hidden, o); }
    if (l) return;
    if (bad) atomicAdd(&st->c_bad, bad);
    if (!hidden) return;
    atomicAdd(&st->c_rows, hidden);
    if (grey) atomicAdd(&st->c_grey, hidden);
    atomicAdd(&st->c_pics, 1u);
    atomicMin(&st->c_first, dec::ev_pos(ev[pics[p0 + blockIdx.x].ev]));
}

__global__ void k_dc_finish(const DecState *st, m2v_decode_stat *h_rec, uint32_t *h_conceal)
{
    if (st->status != dec::kOk) { h_rec->status = st->status; h_rec->err_offset = st->err; h_rec->out_bytes = 0; return; }
    h_rec->out_bytes = st->frame_bytes * st->npics;
    const unsigned long long first = st->c_first == dec::kNone ? h_rec->es_bytes : st->c_first;
    h_conceal[0] = (uint32_t)first; h_conceal[1] = (uint32_t)(first >> 32);
    h_conceal[2] = st->c_bad; h_conceal[3] = st->c_rows; h_conceal[4] = st->c_grey; h_conceal[5] = st->c_pics;
}

void dec_c_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int join, uint32_t *h_mbh, uint32_t *h_sl)
{
    k_dc_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecFPic *)(d_main + kDecMainMatrices), b_pictures, join, h_mbh,
                                        h_sl);
    HIPCHK(hipGetLastError());
}

void dec_c_walk(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, const DecPic *pics, const DecFPic *xp, uint32_t p0, uint32_t np,
                uint32_t f0, uint32_t total, dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *spans)
{
    if (total) {
        k_dc_slices<<<(total + 63u) / 64u, 64, 0, s>>>(es, n, ev, st, pics, xp, p0, np, f0, total, mb, dc, lv, spans);
        HIPCHK(hipGetLastError());
    }
    k_dc_rows<<<np, 64, 0, s>>>(ev, st, pics, xp, p0, f0, mb, spans);  // (a chunk without a slice has rows all the same)
    HIPCHK(hipGetLastError());
}

void dec_c_finish(hipStream_t s, const DecState *st, m2v_decode_stat *h_rec, uint32_t *h_conceal)
{
    k_dc_finish<<<1, 1, 0, s>>>(st, h_rec, h_conceal);
    HIPCHK(hipGetLastError());
}

}  // namespace m2v
