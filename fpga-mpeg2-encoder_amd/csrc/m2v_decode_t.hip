// m2v_decode_t.hip — the plan of Table B-15, concealment motion vectors and dual prime for m2v_decode_device (option "decode_mb_tools"
// = 1 on top of "decode_extended" = 1, with "decode_b_pictures" and "decode_interlaced" 0 or 1 each).  Everything behind the plan's
// wait is m2v_decode_x.hip's, which takes the option as `tools`.
// decoder.decode_main(extended=True, mb_tools=True) is the definition; every function that decides a bit, a column or a verdict is a t_
// (or x_ / il_ / bp_ / main_) function of m2v_decode_kernels.hpp.
//
//   k_dt_plan    k_dx_plan with dec::t_event and dec::t_picture_params: the coding extension's intra_vlc_format,
//                concealment_motion_vectors and top_field_first are kept in bits 21 .. 23 of the packed parameters, and a P picture's
//                "backward" picture is its forward reference - a dual-prime macroblock's record is a field-based one with both
//                directions, and the reconstruction reads it as such.
//
// Why this kernel has a unit to itself: it differs from k_dx_plan in three lines, and as k_dx_plan<true> beside k_dx_plan<false> it
// was tried.  dec::x_event then has two callers in one unit (the plan, and dec::t_event), the compiler no longer inlines it into
// either, and both plans go from 24 to 40 bytes of scratch a lane and from 168 to 216 VGPRs (profiles/decode_shared.json).  In two
// units each plan compiles to what it was.  Folding them needs dec::x_event forced inline in m2v_decode_kernels.hpp.
#include "m2v_decode_state.hpp"

static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

__global__ __launch_bounds__(kDecThreads) void k_dt_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecXPic *__restrict__ bp, int b_pictures, int interlaced, uint32_t *h_mbh,
                                                         uint32_t *h_sl)
{
    __shared__ dec::MainPlan s_P;
    __shared__ unsigned long long s_bad;
    __shared__ uint32_t s_np[kDecThreads], s_ng[kDecThreads], s_nr[kDecThreads], s_ni[kDecThreads], s_na[kDecThreads], s_total;
    __shared__ int s_last[kDecThreads], s_sig[kDecThreads], s_a1[kDecThreads], s_a2[kDecThreads], s_first[kDecThreads];
    __shared__ uint32_t s_ns[kDecThreads], s_mi[kDecThreads], s_mn[kDecThreads], s_rs[kDecThreads], s_slices;      // slices; the events that loaded the matrices; a reset
    const uint32_t tid = threadIdx.x, nev = st->nev;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (st->status == dec::kEvents) {              // the list was too small: the call runs again with the count
        if (tid == 0) { r.status = dec::kEvents; r.pictures = nev; *h_rec = r; }
        return;
    }
    if (tid == 0) s_bad = interlaced ? dec::il_first(es, n, (const uint64_t *)ev, nev, s_P) : dec::main_first(es, n, (const uint64_t *)ev, nev, s_P);
    __syncthreads();
    if (s_bad != dec::kNone) {
        if (tid == 0) { st->status = dec::kSyntax; st->err = s_bad; r.status = dec::kSyntax; r.err_offset = s_bad; *h_rec = r; }
        return;
    }
    const dec::MainPlan &P = s_P;
    const uint32_t progressive = P.seq.h.progressive;
    if (tid < 64) { mats[tid] = P.seq.wi[tid]; mats[64 + tid] = P.seq.wn[tid]; }
    const unsigned long long last_nz = st->last_nz;
    const uint32_t per = (nev + kDecThreads - 1) / kDecThreads, a = min(nev, tid * per), b = min(nev, a + per);
    {   // the last significant event of every range
        int sig = -1;
        for (uint32_t i = a; i < b; ++i) if (dec::main_significant(dec::main_role(es, n, ev[i]))) sig = (int)i;
        s_sig[tid] = sig;
    }
    __syncthreads();
    {
        int prev = -1;                             // the significant event in front of this range
        for (int k = (int)tid - 1; k >= 0 && prev < 0; --k) prev = s_sig[k];
        unsigned long long bad = dec::kNone;
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0, ns = 0, reset = 0;
        dec::XMats xm{dec::kNoEvent, dec::kNoEvent};           // what the range's events loaded behind its last sequence header
        int last = -1, a1 = -1, a2 = -1;           // the range's last I picture and its last two anchors, counted from its first picture
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dec::t_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev, b_pictures != 0, interlaced != 0);
            const int role = dec::main_role(es, n, ev[i]);
            if (dec::main_significant(role)) prev = (int)i;
            ns += role == dec::rSlice;
            reset |= role == dec::rSeq;
            dec::x_mats_event(es, n, (const uint64_t *)ev, nev, i, xm);
            bad = dec::min64(bad, f.bad);
            ng += f.gop; nr += f.rep;
            if (f.pic) {
                if (f.type == 1) { last = (int)np; ++ni; }
                if (f.type != 3) { a2 = a1; a1 = (int)np; ++na; }
                ++np;
            }
        }
        if (bad != dec::kNone) atomicMin(&s_bad, bad);
        s_np[tid] = np; s_ng[tid] = ng; s_nr[tid] = nr; s_ni[tid] = ni; s_na[tid] = na; s_last[tid] = last; s_a1[tid] = a1; s_a2[tid] = a2;
        s_ns[tid] = ns; s_mi[tid] = xm.mi; s_mn[tid] = xm.mn; s_rs[tid] = reset;
    }
    __syncthreads();
    if (tid == 0) {                                // exclusive sums; the last I picture and the last two anchors in front of every range (-1: none)
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0, ns = 0, mi = dec::kNoEvent, mn = dec::kNoEvent;
        int last = -1, a1 = -1, a2 = -1;
        for (int k = 0; k < kDecThreads; ++k) {
            const uint32_t p = s_np[k], i = s_ni[k], c = s_na[k], sl = s_ns[k], ki = s_mi[k], kn = s_mn[k];
            const int l = s_last[k], l1 = s_a1[k], l2 = s_a2[k];
            s_np[k] = np; s_ni[k] = ni; s_na[k] = na; s_last[k] = last; s_a1[k] = a1; s_a2[k] = a2;
            s_ns[k] = ns; s_mi[k] = mi; s_mn[k] = mn;
            ns += sl;
            if (s_rs[k]) { mi = ki; mn = kn; }         // a sequence header in the range: only what was loaded behind it
            else { if (ki != dec::kNoEvent) mi = ki; if (kn != dec::kNoEvent) mn = kn; }
            if (l >= 0) last = (int)np + l;
            if (c >= 2) { a2 = (int)np + l2; a1 = (int)np + l1; }
            else if (c == 1) { a2 = a1; a1 = (int)np + l1; }
            np += p; ni += i; na += c; ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = np; r.gops = ng; r.repeated_headers = nr; r.chains = ni;
        s_total = np; s_slices = ns;
    }
    __syncthreads();
    uint32_t p_end;
    {
        uint32_t p = s_np[tid], chain = s_ni[tid], anchors = s_na[tid];
        int last = s_last[tid], a1 = s_a1[tid], a2 = s_a2[tid], first = -1;
        uint32_t sl = s_ns[tid];                               // the slice events in front of event i
        dec::XMats xm{s_mi[tid], s_mn[tid]};                   // the matrices in force in front of event i
        for (uint32_t i = a; i < b; ++i) {
            const uint32_t code = dec::ev_code(ev[i]);
            if (code != 0x00) {
                if (code <= 0xAFu) ++sl;
                else if (code == 0xB3u || code == 0xB5u) dec::x_mats_event(es, n, (const uint64_t *)ev, nev, i, xm);
                continue;
            }
            const unsigned long long pos = dec::ev_pos(ev[i]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            if (type == 1) { last = (int)p; ++chain; }
            if (last < 0) atomicMin(&s_bad, pos);                      // a P picture without a reference
            if (type == 3 && anchors < 2u) atomicMin(&s_bad, pos);     // a B picture without two anchors in front of it
            if (p < pic_cap) {
                DecXPic q;
                uint32_t quant;
                q.params = dec::t_picture_params(es, n, (const uint64_t *)ev, nev, i, b_pictures != 0, interlaced != 0, progressive, q.slice0, q.nslices, quant);
                const dec::XMats own = dec::x_mats_picture(es, n, (const uint64_t *)ev, nev, xm, quant);
                q.sbase = sl; q.mi = own.mi; q.mn = own.mn;
                h_sl[p] = sl;
                q.display = 0;
                q.fwd = type == 2 ? (uint32_t)a1 : type == 3 ? (uint32_t)a2 : kNoPic;
                q.bwd = type == 3 ? (uint32_t)a1 : type == 2 ? (uint32_t)a1 : kNoPic;      // a P picture: its forward reference again (dual prime)
                pics[p] = DecPic{i, type, chain - 1u, (uint32_t)((int)p - last)}; h_types[p] = (uint8_t)type;
                bp[p] = q;
            }
            if (type != 3) { a2 = a1; a1 = (int)p; ++anchors; if (first < 0) first = (int)p; }
            ++p;
        }
        p_end = p;
        s_first[tid] = first;
    }
    __syncthreads();
    {   // display indices: the range backwards, the next anchor behind it from the lanes behind
        int next = -1;
        for (int k = (int)tid + 1; k < kDecThreads && next < 0; ++k) next = s_first[k];
        uint32_t nxt = next < 0 ? s_total : (uint32_t)next, p = p_end;
        for (uint32_t i = b; i > a; --i) {
            if (dec::ev_code(ev[i - 1]) != 0x00) continue;
            --p;
            const unsigned long long pos = dec::ev_pos(ev[i - 1]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            uint32_t d;
            if (type == 3) d = dec::bp_display_b(p);
            else { d = dec::bp_display_anchor(nxt); nxt = p; }
            if (p < pic_cap) bp[p].display = d;
        }
    }
    __syncthreads();
    if (tid) return;
    const dec::SeqHdr &h = P.seq.h;
    r.width = h.width; r.height = h.height;
    r.frame_bytes = dec::frame_bytes(h.width, h.height);
    if (s_bad != dec::kNone) { r.status = dec::kSyntax; r.err_offset = s_bad; }
    else if (r.pictures > pic_cap) { r.status = dec::kSyntax; r.err_offset = 0; }      // (cannot happen: a picture is three events at least)
    else if (!probe && r.frame_bytes * r.pictures > cap) r.status = dec::kOverflow;
    else if (probe) r.out_bytes = r.frame_bytes * r.pictures;
    st->status = r.status; st->err = s_bad; st->npics = r.pictures; st->gops = r.gops; st->reps = r.repeated_headers; st->chains = r.chains;
    st->width = r.width; st->height = r.height; st->mbw = P.mbw; st->mbh = P.mbh; st->frame_bytes = r.frame_bytes;
    *h_mbh = P.mbh;
    if (r.pictures <= pic_cap) h_sl[r.pictures] = s_slices;
    *h_rec = r;
}

void dec_t_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int interlaced, uint32_t *h_mbh, uint32_t *h_sl)
{
    k_dt_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecXPic *)(d_main + kDecMainMatrices), b_pictures, interlaced,
                                        h_mbh, h_sl);
    HIPCHK(hipGetLastError());
}

}  // namespace m2v
