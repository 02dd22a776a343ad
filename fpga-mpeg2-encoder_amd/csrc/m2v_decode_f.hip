// m2v_decode_f.hip — field pictures for m2v_decode_device (option "decode_field_pictures" = 1 on top of "decode_interlaced",
// "decode_extended" and "decode_mb_tools" = 1, with "decode_b_pictures" 0 or 1).  Modelled on m2v_decode_x.hip with TOOLS, whose tables
// and launches these are: m2v_decode.hip keeps the scan; this unit holds the plan and everything behind the plan's wait.
// decoder.decode_main(..., field_pictures=True) is the definition; every function that decides a bit, a column, a pair or a verdict is
// an fp_ (or t_ / x_ / il_ / bp_ / main_) function of m2v_decode_kernels.hpp.
//
// Two indices: a CODED PICTURE (a frame picture or one field: slices, records, parameters, matrices) and a FRAME (a slot of the
// chunk's buffer, a display index, a reference).  The table behind the matrices holds one DecFPic a coded picture.
//
//   k_df_plan    k_dx_plan's grammar by dec::fp_event, plus the pairs.  A lane sums the pictures of its range of events twice
//                (dec::fp_range: nothing waiting in front of it / a first field waiting), lane 0 joins the sums in order
//                (dec::fp_join), and every lane places its pictures behind the sums in front of its range (dec::fp_place): the frame,
//                "second field", the frames it refers to, and the refusals of a pair.  A pair parted by a range's edge is planned from
//                what crosses the edge, as one inside a range is.  Display indices go by frames: a B frame's at once, an anchor
//                frame's when the next anchor frame begins (written to the entry of its first picture, wherever that lies).
//   k_df_slices  one lane per slice EVENT of the chunk: dec::t_slice for a frame picture, dec::fp_slice for a field (half the rows).
//                A field's records lie in its frame's stretch: the first field's in the first half, the second field's behind them.
//   k_df_recon   the residual as every dec::IMb unit's (imb_residual); a frame picture predicts as k_dx_recon, a field writes the
//                lines of its parity of its frame's slot at twice the stride, and reads reference fields the same way (dec::fp_predict).  The second field of an anchor frame reads the other parity's
//                lines of its OWN slot: it is launched a step behind its first field, and those lines are not the ones it writes.
//   k_df_out     one frame per slot at its display index, through out_picture (the entry of the frame's first picture carries the index).
//   k_df_mats, k_df_cont, k_df_judge, k_df_finish   as k_dx_*, over DecFPic.
//
// A chunk is a run of whole FRAMES ("decode_batch" counts frames): its edge never parts a pair, and the two carried slots hold whole
// anchor frames.
#include "m2v_decode_state.hpp"

static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

__global__ __launch_bounds__(kDecThreads) void k_df_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecFPic *bp, int b_pictures, uint32_t *h_mbh, uint32_t *h_sl)
{
    __shared__ dec::MainPlan s_P, s_Pf;                    // s_Pf: with a field's macroblock rows
    __shared__ unsigned long long s_bad;
    __shared__ dec::FpRange s_A[kDecThreads], s_B[kDecThreads], s_in[kDecThreads], s_all;
    __shared__ uint32_t s_m[kDecThreads], s_cp[kDecThreads], s_ng[kDecThreads], s_nr[kDecThreads], s_ncp;
    __shared__ int s_sig[kDecThreads];
    __shared__ uint32_t s_ns[kDecThreads], s_mi[kDecThreads], s_mn[kDecThreads], s_rs[kDecThreads], s_slices;
    const uint32_t tid = threadIdx.x, nev = st->nev;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (st->status == dec::kEvents) {              // the list was too small: the call runs again with the count
        if (tid == 0) { r.status = dec::kEvents; r.pictures = nev; *h_rec = r; }
        return;
    }
    if (tid == 0) {
        s_bad = dec::il_first(es, n, (const uint64_t *)ev, nev, s_P);
        s_Pf = s_P;
        s_Pf.mbh = s_P.mbh / 2u;
    }
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
        uint32_t ng = 0, nr = 0, ns = 0, reset = 0;
        dec::XMats xm{dec::kNoEvent, dec::kNoEvent};           // what the range's events loaded behind its last sequence header
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dec::fp_event(es, n, (const uint64_t *)ev, nev, i, P, s_Pf, last_nz, prev, b_pictures != 0);
            const int role = dec::main_role(es, n, ev[i]);
            if (dec::main_significant(role)) prev = (int)i;
            ns += role == dec::rSlice;
            reset |= role == dec::rSeq;
            dec::x_mats_event(es, n, (const uint64_t *)ev, nev, i, xm);
            bad = dec::min64(bad, f.bad);
            ng += f.gop; nr += f.rep;
        }
        if (bad != dec::kNone) atomicMin(&s_bad, bad);
        dec::FpRange A, B;
        uint32_t m;
        dec::fp_range(es, n, (const uint64_t *)ev, nev, a, b, b_pictures != 0, A, B, m);       // the range's pictures, for either state in front of it
        s_A[tid] = A; s_B[tid] = B; s_m[tid] = m;
        s_ng[tid] = ng; s_nr[tid] = nr; s_ns[tid] = ns; s_mi[tid] = xm.mi; s_mn[tid] = xm.mn; s_rs[tid] = reset;
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
            dec::fp_join(all, cp, s_A[k], s_B[k], s_m[k]);
            ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = all.frames; r.gops = ng; r.repeated_headers = nr; r.chains = all.ni;
        s_all = all; s_ncp = cp; s_slices = ns;
    }
    __syncthreads();
    {
        dec::FpRange s = s_in[tid];
        uint32_t cp = s_cp[tid];
        uint32_t sl = s_ns[tid];                               // the slice events in front of event i
        dec::XMats xm{s_mi[tid], s_mn[tid]};                   // the matrices in force in front of event i
        unsigned long long waiting = dec::kNone;               // the first field of this range that waits for its partner
        for (uint32_t i = a; i < b; ++i) {
            const uint32_t code = dec::ev_code(ev[i]);
            const unsigned long long pos = dec::ev_pos(ev[i]);
            if (code != 0x00) {
                if (code <= 0xAFu) ++sl;
                else if (code == 0xB3u || code == 0xB5u) dec::x_mats_event(es, n, (const uint64_t *)ev, nev, i, xm);
                if (s.open && (code == 0xB3u || code == 0xB8u || code == 0xB7u)) atomicMin(&s_bad, pos);      // between the two fields of a frame
                continue;
            }
            uint32_t type, tref, ps;
            if (!dec::fp_is_picture(es, n, (const uint64_t *)ev, nev, i, b_pictures != 0, type, tref, ps)) continue;
            const int32_t anchor_cp = s.a1cp;
            const dec::FpPlace q = dec::fp_place(s, cp, ps, type, tref);
            if (q.bad) atomicMin(&s_bad, pos);
            waiting = s.open ? pos : dec::kNone;
            if (cp < pic_cap) {
                uint32_t slice0, nslices, quant;
                dec::FPicParams pp = dec::fp_picture_params(es, n, (const uint64_t *)ev, nev, i, b_pictures != 0, progressive, slice0, nslices, quant);
                pp.second = q.second; pp.noref = q.second && type == 2u && q.fwd == kNoPic;
                const dec::XMats own = dec::x_mats_picture(es, n, (const uint64_t *)ev, nev, xm, quant);
                DecFPic *d = bp + cp;                          // (field by field: an anchor frame's display index is another lane's to write)
                d->slice0 = slice0; d->params = dec::fp_params_pack(pp); d->fwd = q.fwd; d->bwd = q.bwd; d->nslices = nslices; d->sbase = sl;
                d->mi = own.mi; d->mn = own.mn; d->frame = q.frame;
                if (q.second) d->display = 0;
                else if (type == 3u) d->display = dec::bp_display_b(q.frame);
                h_sl[cp] = sl;
                pics[cp] = DecPic{i, type, 0u, 0u};
                h_types[cp] = (uint8_t)(type | pp.ps << 2 | q.second << 4);
            }
            if (!q.second && type != 3u && anchor_cp >= 0 && (uint32_t)anchor_cp < pic_cap) bp[anchor_cp].display = dec::bp_display_anchor(q.frame);
            ++cp;
        }
        if (s.open && waiting != dec::kNone && cp == s_ncp) atomicMin(&s_bad, waiting);      // a first field no picture follows
    }
    __syncthreads();
    if (tid) return;
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
    *h_rec = r;
}

// coded pictures [p0, p0 + np) - the frames from f0 on - with `total` slices: one slice EVENT per lane, into the row its code names.
// The lane leaves its span; a slice that cannot be read lowers st->err
__global__ __launch_bounds__(64) void k_df_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                  const DecPic *__restrict__ pics, const DecFPic *__restrict__ xp, uint32_t p0, uint32_t np, uint32_t f0, uint32_t total,
                                                  dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *__restrict__ spans)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, nev = st->nev;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= total) return;
    uint32_t k;
    const uint32_t pic = dec::x_slice_pic(xp + p0, np, g, k);
    const DecPic P = pics[p0 + pic];
    const DecFPic Q = xp[p0 + pic];
    const uint32_t i = Q.slice0 + k;
    spans[g] = 0u;
    if (k >= Q.nslices || i >= nev) return;                            // (the plan accepted the picture: its slices are there)
    const unsigned long long start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : n;
    const uint32_t code = dec::ev_code(ev[i]);
    const dec::FPicParams pp = dec::fp_params_unpack(Q.params);
    const bool field = dec::fp_is_field(pp.ps);
    const uint32_t rows = field ? mbh / 2u : mbh;
    if (code < 1u || code > rows || Q.frame < f0) { atomicMin(&st->err, start); return; }      // (the plan's grammar: 1 <= code <= rows)
    const size_t first = df_first(Q, f0, mbw * mbh) + (size_t)(code - 1u) * mbw;
    IMbSink sink{mb + first, dc + first * 6, lv + first * 384};
    int c0, c1;
    const bool ok = field ? dec::fp_slice(es, start, end, P.type, pp, (int)mbw, (int)rows, (int)code - 1, sink, c0, c1)
                          : dec::t_slice(es, start, end, P.type, pp.t, (int)mbw, (int)mbh, (int)code - 1, sink, c0, c1);
    spans[g] = dec::x_span_pack(ok, code, c0, c1);
    if (!ok) atomicMin(&st->err, start);
}

// continuity behind the walk: every readable slice against the span of the slice in front of it in its picture
__global__ __launch_bounds__(64) void k_df_cont(const unsigned long long *__restrict__ ev, DecState *st, const DecFPic *__restrict__ xp, uint32_t p0, uint32_t np,
                                                uint32_t total, const uint32_t *__restrict__ spans)
{
    if (st->status != dec::kOk) return;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= total) return;
    uint32_t k;
    const uint32_t pic = dec::x_slice_pic(xp + p0, np, g, k);
    const DecFPic Q = xp[p0 + pic];
    const uint32_t cur = spans[g];
    if (!(cur >> 31) || k >= Q.nslices || Q.slice0 + k >= st->nev) return;      // (not readable: reported by its walk)
    if (!dec::x_continuous(cur, k ? spans[g - 1] : 0u, k, Q.nslices, st->mbw)) atomicMin(&st->err, dec::ev_pos(ev[Q.slice0 + k]));
}

__global__ void k_df_judge(DecState *st)
{
    if (st->status == dec::kOk && st->err != dec::kNone) st->status = dec::kSyntax;
}

// the matrix table: block p writes coded picture p's 128 weights, raster order - the sequence's, or those of the extension in force
__global__ __launch_bounds__(128) void k_df_mats(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, const DecState *__restrict__ st,
                                                 const uint8_t *__restrict__ mats, const DecFPic *__restrict__ xp, uint8_t *__restrict__ table)
{
    if (st->status != dec::kOk) return;
    const uint32_t p = blockIdx.x, l = threadIdx.x, m = l >> 6, t = l & 63u;
    const uint32_t src = m ? xp[p].mn : xp[p].mi;
    table[(size_t)p * 128u + l] = (uint8_t)dec::x_matrix_weight(es, n, (const uint64_t *)ev, st->nev, src, (int)m, t, mats + 64u * m);
}

// grid = (macroblocks of a frame, coded pictures of the launch); list: their coded indices, all of the chunk that begins at frame f0.
// A frame picture is k_dx_recon's; a field has half the macroblocks and works on the lines of its parity.  Every read of a reference
// lies inside its picture or its field, and the field is there: the slice walk refused the slice otherwise (dec::il_inside,
// dec::fp_inside), and a refused slice stops the call before this kernel (k_df_judge) - or, with "decode_conceal", its whole row is
// concealed before it (k_dc_rows): a record that reaches this kernel is a readable slice's or dec::c_record's, which reads its own
// macroblock of the forward frame
__global__ __launch_bounds__(64) void k_df_recon(const DecState *__restrict__ st, const uint32_t *__restrict__ list, uint32_t f0, uint32_t c1,
                                                 const uint8_t *__restrict__ mats, const DecPic *__restrict__ pics, const DecFPic *__restrict__ bp,
                                                 const dec::IMb *__restrict__ mb, const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf, size_t psz)
{
    __shared__ int32_t F[6][64];
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, mbs = mbw * mbh, W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const uint32_t k = blockIdx.x, l = threadIdx.x, gp = list[blockIdx.y];
    const DecFPic Q = bp[gp];
    const dec::FPicParams fp = dec::fp_params_unpack(Q.params);
    const bool field = dec::fp_is_field(fp.ps);
    if ((field && k >= mbs / 2u) || Q.frame < f0) return;              // (the whole block: a field has half a frame's macroblocks)
    const dec::PicParams pp = fp.t.i.b.p;
    const size_t at = df_first(Q, f0, mbs) + k;
    const dec::IMb m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw, par = field ? fp.ps - 1u : 0u;
    uint8_t *cur = buf + (size_t)(Q.frame - f0 + 2u) * psz;
    const uint8_t *fwd = buf + (size_t)slot(Q.fwd, f0, c1) * psz, *bwd = buf + (size_t)slot(Q.bwd, f0, c1) * psz;
    // the frame that holds the field of parity q of direction d: the second field of an anchor frame finds the other parity in its own slot
    const bool own = field && fp.second && pics[gp].type == 2u;
    const uint8_t *const ref[4] = {own && par != 0u ? cur : fwd, own && par != 1u ? cur : fwd, own && par != 0u ? cur : bwd, own && par != 1u ? cur : bwd};
    const bool intra = m.intra != 0;
    imb_residual(F, m, pp, mats + (size_t)gp * 128u, dc, lv, at, l);
    {   // luma: four samples of one row per lane.  A field's row y of macroblock row `row` is line 16 row + y of the field: frame line 2 (16 row + y) + par
        const uint32_t y = l >> 2, x0 = (l & 3u) * 4u, blk = dec::il_luma_block(x0, y, m.dct_type), brow = dec::il_luma_row(y, m.dct_type);
        const bool coded = (m.cbp >> (5 - blk)) & 1;
        const int px = (int)(16u * col + x0), py = (int)(16u * row + y);
        const uint32_t line = field ? 2u * (16u * row + y) + par : 16u * row + y;
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t pred = intra ? 128 : field ? dec::fp_predict(ref, (int)W, px + j, py, (int)(y >> 3), m, false) : dec::il_predict(fwd, bwd, (int)W, px + j, py, m, false);
            const int32_t res = coded ? F[blk][brow * 8u + ((x0 + j) & 7u)] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint32_t *)(cur + (size_t)line * W + 16u * col + x0) = v;
    }
    {   // chroma: two samples per lane, U in the first half of the wavefront
        const uint32_t pl = l >> 5, y = (l >> 2) & 7u, x0 = (l & 3u) * 2u;
        const bool coded = (m.cbp >> (1 - pl)) & 1;
        const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2u);
        const int px = (int)(8u * col + x0), py = (int)(8u * row + y);
        const uint32_t line = field ? 2u * (8u * row + y) + par : 8u * row + y;
        const uint8_t *const cref[4] = {ref[0] + plane, ref[1] + plane, ref[2] + plane, ref[3] + plane};
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t pred = intra ? 128 : field ? dec::fp_predict(cref, (int)CW, px + j, py, (int)(y >> 2), m, true)
                                                     : dec::il_predict(fwd + plane, bwd + plane, (int)CW, px + j, py, m, true);
            const int32_t res = coded ? F[4u + pl][y * 8u + x0 + j] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint16_t *)(cur + plane + (size_t)line * CW + 8u * col + x0) = (uint16_t)v;
    }
}

// the frame of coded picture p0 + blockIdx.y (its first picture: a second field has nothing to put out) into dst at its display index:
// bytes [display * fb, (display + 1) * fb) of the output
__global__ __launch_bounds__(kDecThreads) void k_df_out(const DecState *__restrict__ st, const DecFPic *__restrict__ bp, const uint8_t *__restrict__ buf, size_t psz,
                                                        uint32_t p0, uint32_t f0, uint8_t *__restrict__ dst, int layout)
{
    if (st->status != dec::kOk) return;
    const uint32_t w = st->width, h = st->height, W = 16u * st->mbw, H = 16u * st->mbh;
    const DecFPic Q = bp[p0 + blockIdx.y];
    const uint32_t d = Q.display;
    if (((Q.params >> 26) & 1u) || d >= st->npics || Q.frame < f0) return;      // (an accepted stream's display indices are a permutation of its frames)
    const unsigned long long fb = st->frame_bytes, lo = (unsigned long long)d * fb;
    out_picture(buf + (size_t)(Q.frame - f0 + 2u) * psz, w, h, W, H, lo, lo + fb, dst, layout, kDecThreads);
}

__global__ void k_df_finish(const DecState *st, m2v_decode_stat *h_rec)
{
    if (st->status == dec::kOk) { h_rec->out_bytes = st->frame_bytes * st->npics; return; }
    h_rec->status = st->status; h_rec->err_offset = st->err; h_rec->out_bytes = 0;
}

void dec_f_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, uint32_t *h_mbh, uint32_t *h_sl)
{
    k_df_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecFPic *)(d_main + kDecMainMatrices), b_pictures, h_mbh, h_sl);
    HIPCHK(hipGetLastError());
}

// dec_x_chunks over frames: a chunk is B whole frames, its coded pictures the one or two of each.  types[p]: coded picture p's type,
// structure << 2, "second field" << 4 (the plan's); ncp: the coded pictures; h_sl[p]: the slices in front of coded picture p
void dec_f_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t mbh, size_t B,
                  const uint8_t *types, size_t ncp, uint32_t *h_list, const uint32_t *h_sl, m2v_decode_stat *h_rec, uint32_t *h_conceal)
{
    const bool conceal = h_conceal != nullptr;
    const size_t nf = R.pictures, mbw = (R.width + 15) / 16, mbs = mbw * mbh, psz = mbs * 384;
    auto type_of = [&](size_t p) { return (unsigned)(types[p] & 3u); };
    auto second = [&](size_t p) { return ((types[p] >> 4) & 1u) != 0; };
    // every frame's first coded picture, its type (its first picture's) and the anchor frame in front of it
    std::vector<size_t> fcp;
    for (size_t p = 0; p < ncp; ++p) if (!second(p)) fcp.push_back(p);
    if (fcp.size() != nf) throw ::m2v::HipError{hipErrorUnknown, "k_df_plan: as many first pictures as frames"};      // (an accepted stream: every frame has one)
    fcp.push_back(ncp);
    std::vector<long> before(nf, -1);
    {
        long a = -1;
        for (size_t f = 0; f < nf; ++f) { before[f] = a; if (type_of(fcp[f]) != 3u) a = (long)f; }
    }
    size_t most = 1;                                                   // the most slices of a chunk
    for (size_t f0 = 0; f0 < nf; f0 += B) most = std::max<size_t>(most, h_sl[fcp[std::min(f0 + B, nf)]] - h_sl[fcp[f0]]);
    const size_t span_off = (ncp * 128 + 3) & ~(size_t)3;
    e->d_dec_x.ensure(span_off + most * sizeof(uint32_t));
    e->d_dec_mb.ensure(B * mbs * sizeof(dec::IMb));
    e->d_dec_dc.ensure(B * mbs * 6);
    e->d_dec_lv.ensure(B * mbs * 384);
    e->d_dec_buf.ensure((B + 2) * psz);
    e->d_dec_list.ensure(ncp);
    // every chunk's anchor pictures ordered by their step inside the chunk - a picture is a step behind everything of the chunk it reads:
    // a P picture the anchor frame in front of its frame, the second field of a frame its first field too; with "decode_conceal" an I
    // picture as a P picture, for a concealed row of it reads that frame -, then its B pictures; and what
    // the chunk leaves in slots 0 and 1 for the next
    std::vector<DecChunk> chunks;
    long a1 = -1, a2 = -1;                                             // the last two anchor frames in front of the chunk
    for (size_t f0 = 0; f0 < nf; f0 += B) {
        const size_t nb = std::min(B, nf - f0), p0 = fcp[f0], p1 = fcp[f0 + nb];
        DecChunk C;
        C.c1 = a1;
        std::vector<long> step(p1 - p0, -1), fstep(nb, -1);
        long deepest = -1;
        for (size_t p = p0; p < p1; ++p) {
            if (type_of(p) == 3u) continue;
            const size_t f = (size_t)(std::upper_bound(fcp.begin(), fcp.end(), p) - fcp.begin()) - 1;
            long dep = -1;
            if (type_of(p) == 2u || conceal) {
                if (before[f] >= (long)f0) dep = std::max(dep, fstep[(size_t)before[f] - f0]);
                if (second(p)) dep = std::max(dep, step[p - 1 - p0]);
            }
            step[p - p0] = dep + 1;
            fstep[f - f0] = std::max(fstep[f - f0], step[p - p0]);
            deepest = std::max(deepest, step[p - p0]);
        }
        size_t at = p0;
        for (long j = 0; j <= deepest; ++j) {
            const size_t first = at;
            for (size_t p = p0; p < p1; ++p) if (step[p - p0] == j) h_list[at++] = (uint32_t)p;
            C.steps.push_back(DecLaunch{first, at - first});
        }
        C.b.off = at;
        for (size_t p = p0; p < p1; ++p) if (type_of(p) == 3u) h_list[at++] = (uint32_t)p;
        C.b.count = at - C.b.off;
        auto slot = [&](long r) { return r >= (long)f0 ? 2 + (r - (long)f0) : r == C.c1 ? 1L : 0L; };
        long n1 = a1, n2 = a2;
        for (size_t f = f0; f < f0 + nb; ++f) if (type_of(fcp[f]) != 3u) { n2 = n1; n1 = (long)f; }
        C.carry0 = n2 >= 0 && slot(n2) != 0 ? slot(n2) : -1;
        C.carry1 = n1 >= 0 && slot(n1) != 1 ? slot(n1) : -1;
        a1 = n1; a2 = n2;
        chunks.push_back(C);
    }
    auto *d_st = (DecState *)e->d_dec_st.p;
    auto *d_mb = (dec::IMb *)e->d_dec_mb.p;
    const uint8_t *mats = e->d_dec_x.p;                                // the matrix table: 128 bytes a coded picture
    auto *spans = (uint32_t *)(e->d_dec_x.p + span_off);
    const auto *bp = (const DecFPic *)(e->d_dec_main.p + kDecMainMatrices);
    const auto *pics = (const DecPic *)e->d_dec_pics.p;
    HIPCHK(hipMemcpyAsync(e->d_dec_list.p, h_list, ncp * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    k_df_mats<<<(unsigned)ncp, 128, 0, s>>>(es, n, e->d_dec_ev.p, d_st, e->d_dec_main.p, bp, e->d_dec_x.p);
    HIPCHK(hipGetLastError());
    for (size_t f0 = 0, c = 0; f0 < nf; f0 += B, ++c) {
        const size_t nb = std::min(B, nf - f0), p0 = fcp[f0], np = fcp[f0 + nb] - p0;
        const DecChunk &C = chunks[c];
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, nb * mbs * 768, s));
        const size_t total = h_sl[p0 + np] - h_sl[p0];                 // (every picture the plan accepted has a slice; with "decode_conceal" it may have none, and a chunk too)
        if (conceal) {                                                 // nothing is refused behind the plan: a verdict per row, the rows concealed
            dec_c_walk(s, es, n, e->d_dec_ev.p, d_st, pics, bp, (uint32_t)p0, (uint32_t)np, (uint32_t)f0, (uint32_t)total, d_mb, e->d_dec_dc.p, e->d_dec_lv.p, spans);
        } else if (total) {
            k_df_slices<<<(unsigned)((total + 63) / 64), 64, 0, s>>>(es, n, e->d_dec_ev.p, d_st, pics, bp, (uint32_t)p0, (uint32_t)np, (uint32_t)f0, (uint32_t)total, d_mb,
                                                                     e->d_dec_dc.p, e->d_dec_lv.p, spans);
            HIPCHK(hipGetLastError());
            k_df_cont<<<(unsigned)((total + 63) / 64), 64, 0, s>>>(e->d_dec_ev.p, d_st, bp, (uint32_t)p0, (uint32_t)np, (uint32_t)total, spans);
            HIPCHK(hipGetLastError());
        }
        if (!conceal) {
            k_df_judge<<<1, 1, 0, s>>>(d_st);
            HIPCHK(hipGetLastError());
        }
        auto recon = [&](const DecLaunch &l) {
            if (!l.count) return;
            k_df_recon<<<dim3((unsigned)mbs, (unsigned)l.count), 64, 0, s>>>(d_st, e->d_dec_list.p + l.off, (uint32_t)f0, (uint32_t)C.c1, mats, pics, bp, d_mb, e->d_dec_dc.p,
                                                                            e->d_dec_lv.p, e->d_dec_buf.p, psz);
            HIPCHK(hipGetLastError());
        };
        for (const DecLaunch &l : C.steps) recon(l);
        recon(C.b);                                                    // every B picture of the chunk at once: its anchor frames are done
        const size_t units = (R.frame_bytes + 15) / 16 + 1;
        k_df_out<<<dim3((unsigned)std::min<size_t>((units + kDecThreads - 1) / kDecThreads, 1024), (unsigned)np), kDecThreads, 0, s>>>(d_st, bp, e->d_dec_buf.p, psz,
                                                                                                                                      (uint32_t)p0, (uint32_t)f0, dst, layout);
        HIPCHK(hipGetLastError());
        if (f0 + B < nf) {                                             // the next chunk's carried anchor frames: slot 0 first (it may come from slot 1)
            if (C.carry0 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + (size_t)C.carry0 * psz, psz, hipMemcpyDeviceToDevice, s));
            if (C.carry1 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p + psz, e->d_dec_buf.p + (size_t)C.carry1 * psz, psz, hipMemcpyDeviceToDevice, s));
        }
    }
    if (conceal) {
        dec_c_finish(s, d_st, h_rec, h_conceal);
    } else {
        k_df_finish<<<1, 1, 0, s>>>(d_st, h_rec);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
}

}  // namespace m2v
