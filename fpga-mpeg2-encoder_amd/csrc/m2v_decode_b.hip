// m2v_decode_b.hip — B pictures for m2v_decode_device (option "decode_b_pictures" = 1 on top of "decode_syntax" = M2V_SYNTAX_MAIN).
// m2v_decode.hip tells the whole story and keeps the scan; this unit holds the plan and everything behind the plan's wait.
// decoder.decode_main(b_pictures=True) is the definition; every function that decides a bit or a sample is a bp_ (or main_) function of
// m2v_decode_kernels.hpp.
//
//   k_db_plan    k_dm_plan with picture_coding_type 3 (dec::bp_event).  Per picture it also records the display index, the coded
//                indices of its references and all four f_codes (DecBPic).  The last two anchors in front of every lane's range are a
//                look-back over the lanes in front, as the last I picture is; a B picture with fewer than two anchors in front of it
//                and a P picture without an I picture are found in the same pass.  An anchor's display index needs the next anchor: the
//                lanes note their first anchor and look forward over the lanes behind, then walk their own range backwards.
//   k_db_slices  one slice per lane (dec::bp_slice): an I or P picture's through dec::main_slice, a B picture's with Table B-4 and two
//                predictors.  A record carries both vectors and the directions; a skipped macroblock's carries those it inherits.
//   k_db_recon   one wavefront per macroblock with k_dm_recon's lane mapping; one or two predictions from the slots the picture's
//                table names, the mean of both where both are used.  grid = (macroblocks, pictures of the launch).
//   k_db_out     every picture of the chunk at its display index: grid = (units, pictures); 16-byte stores where the destination is
//                aligned, the first and last unit of a picture byte by byte (out_picture, m2v_decode_device.hpp).
//
// The chunk's buffer: slot 0 = the anchor before the last one in front of the chunk, slot 1 = the last one, slot 2 + k = picture k of
// the chunk.  Within a chunk the anchors run step by step along their chains (a step counts anchors only), then all B pictures of the
// chunk in one launch: nothing depends on a B picture (dec_chunk_schedule, m2v_decode_chunks.hpp, which the units of the later options
// run too; slot, m2v_decode_device.hpp).  The host waits where it did: behind the plan and at the end.
#include "m2v_decode_state.hpp"

static_assert(sizeof(dec::BMb) == sizeof(dec::MbRec), "the B-picture record lies where the module's does");

namespace m2v {

__global__ __launch_bounds__(kDecThreads) void k_db_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecBPic *__restrict__ bp)
{
    __shared__ dec::MainPlan s_P;
    __shared__ unsigned long long s_bad;
    __shared__ uint32_t s_np[kDecThreads], s_ng[kDecThreads], s_nr[kDecThreads], s_ni[kDecThreads], s_na[kDecThreads], s_total;
    __shared__ int s_last[kDecThreads], s_sig[kDecThreads], s_a1[kDecThreads], s_a2[kDecThreads], s_first[kDecThreads];
    const uint32_t tid = threadIdx.x, nev = st->nev;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (st->status == dec::kEvents) {              // the list was too small: the call runs again with the count
        if (tid == 0) { r.status = dec::kEvents; r.pictures = nev; *h_rec = r; }
        return;
    }
    if (tid == 0) s_bad = dec::main_first(es, n, (const uint64_t *)ev, nev, s_P);
    __syncthreads();
    if (s_bad != dec::kNone) {
        if (tid == 0) { st->status = dec::kSyntax; st->err = s_bad; r.status = dec::kSyntax; r.err_offset = s_bad; *h_rec = r; }
        return;
    }
    const dec::MainPlan &P = s_P;
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
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0;
        int last = -1, a1 = -1, a2 = -1;           // the range's last I picture and its last two anchors, counted from its first picture
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dec::bp_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev);
            if (dec::main_significant(dec::main_role(es, n, ev[i]))) prev = (int)i;
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
    }
    __syncthreads();
    if (tid == 0) {                                // exclusive sums; the last I picture and the last two anchors in front of every range (-1: none)
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0;
        int last = -1, a1 = -1, a2 = -1;
        for (int k = 0; k < kDecThreads; ++k) {
            const uint32_t p = s_np[k], i = s_ni[k], c = s_na[k];
            const int l = s_last[k], l1 = s_a1[k], l2 = s_a2[k];
            s_np[k] = np; s_ni[k] = ni; s_na[k] = na; s_last[k] = last; s_a1[k] = a1; s_a2[k] = a2;
            if (l >= 0) last = (int)np + l;
            if (c >= 2) { a2 = (int)np + l2; a1 = (int)np + l1; }
            else if (c == 1) { a2 = a1; a1 = (int)np + l1; }
            np += p; ni += i; na += c; ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = np; r.gops = ng; r.repeated_headers = nr; r.chains = ni;
        s_total = np;
    }
    __syncthreads();
    uint32_t p_end;
    {
        uint32_t p = s_np[tid], chain = s_ni[tid], anchors = s_na[tid];
        int last = s_last[tid], a1 = s_a1[tid], a2 = s_a2[tid], first = -1;
        for (uint32_t i = a; i < b; ++i) {
            if (dec::ev_code(ev[i]) != 0x00) continue;
            const unsigned long long pos = dec::ev_pos(ev[i]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            if (type == 1) { last = (int)p; ++chain; }
            if (last < 0) atomicMin(&s_bad, pos);                      // a P picture without a reference
            if (type == 3 && anchors < 2u) atomicMin(&s_bad, pos);     // a B picture without two anchors in front of it
            if (p < pic_cap) {
                DecBPic q;
                q.params = dec::bp_picture_params(es, n, (const uint64_t *)ev, nev, i, q.slice0);
                q.display = 0;
                q.fwd = type == 2 ? (uint32_t)a1 : type == 3 ? (uint32_t)a2 : kNoPic;
                q.bwd = type == 3 ? (uint32_t)a1 : kNoPic;
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
    *h_rec = r;
}

struct DecBSink {
    dec::BMb *mb_;
    int32_t *dc_;
    int16_t *lv_;
    M2V_HD void mb(int col, const dec::BMb &m, const int32_t (&dc)[6])
    {
        mb_[col] = m;
#pragma unroll
        for (int k = 0; k < 6; ++k) dc_[col * 6 + k] = dc[k];
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { lv_[(col * 6 + blk) * 64 + (int)i] = (int16_t)l; }
};

// as k_dm_slices: pictures [p0, p0 + np) of any type, one slice per lane, the earliest refused slice lowers st->err
__global__ __launch_bounds__(64) void k_db_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                  const DecPic *__restrict__ pics, const DecBPic *__restrict__ bp, uint32_t p0, uint32_t np, dec::BMb *mb,
                                                  int32_t *dc, int16_t *lv)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, nev = st->nev;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x, pic = g / mbh, row = g - pic * mbh;
    if (pic >= np) return;
    const DecPic P = pics[p0 + pic];
    const DecBPic Q = bp[p0 + pic];
    const uint32_t i = Q.slice0 + row;
    if (i >= nev) return;                                              // (the plan accepted the picture: its slices are there)
    const unsigned long long start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : n;
    const size_t first = ((size_t)pic * mbh + row) * mbw;
    DecBSink sink{mb + first, dc + first * 6, lv + first * 384};
    if (!dec::bp_slice(es, start, end, P.type, dec::bp_params_unpack(Q.params), (int)mbw, (int)mbh, (int)row, sink)) atomicMin(&st->err, start);
}

__global__ void k_db_judge(DecState *st)
{
    if (st->status == dec::kOk && st->err != dec::kNone) st->status = dec::kSyntax;
}

// as k_dm_recon: grid = (macroblocks, pictures of the launch); list: their coded indices, all of chunk [p0, ...)
__global__ __launch_bounds__(64) void k_db_recon(const DecState *__restrict__ st, const uint32_t *__restrict__ list, uint32_t p0, uint32_t c1,
                                                 const uint8_t *__restrict__ mats, const DecBPic *__restrict__ bp, const dec::BMb *__restrict__ mb,
                                                 const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf, size_t psz)
{
    __shared__ int32_t F[6][64];
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, mbs = mbw * mbh, W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const uint32_t k = blockIdx.x, l = threadIdx.x, gp = list[blockIdx.y], pic = gp - p0;
    const DecBPic Q = bp[gp];
    const dec::PicParams pp = dec::params_unpack(Q.params);
    const size_t at = (size_t)pic * mbs + k;
    const dec::BMb m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw;
    uint8_t *cur = buf + (size_t)(pic + 2u) * psz;
    const uint8_t *fwd = buf + (size_t)slot(Q.fwd, p0, c1) * psz, *bwd = buf + (size_t)slot(Q.bwd, p0, c1) * psz;
    const bool intra = m.intra != 0;
    const uint32_t dirs = m.dirs;
    const int32_t qscale = dec::main_scale(m.qcode, pp.qst), weight = mats[(intra ? 0u : 64u) + l];
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
        if (!((m.cbp >> (5 - blk)) & 1)) continue;                     // (uniform: the whole wavefront works on one macroblock)
        int32_t f = intra && l == 0 ? dec::main_dequant_dc(dc[at * 6 + blk], pp.prec) : dec::main_dequant(lv[(at * 6 + blk) * 64 + l], weight, intra, qscale);
        const int odd = __popcll(__ballot(f & 1)) & 1;
        if (!odd && l == 63) f = dec::mismatch(f);
        F[blk][l] = f;
    }
    __syncthreads();
    const int blk8 = (int)(l >> 3), r8 = (int)(l & 7u);
    const bool mine = l < 48 && ((m.cbp >> (5 - blk8)) & 1);
    if (mine) {
        int32_t a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = F[blk8][r8 * 8 + j];
        dec::idct_1d(a, true, dec::kIso);
#pragma unroll
        for (int j = 0; j < 8; ++j) F[blk8][r8 * 8 + j] = a[j];
    }
    __syncthreads();
    if (mine) {
        int32_t a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = F[blk8][j * 8 + r8];
        dec::idct_1d(a, false, dec::kIso);
#pragma unroll
        for (int j = 0; j < 8; ++j) F[blk8][j * 8 + r8] = a[j];
    }
    __syncthreads();
    {   // luma: four samples of one row per lane
        const uint32_t y = l >> 2, x0 = (l & 3u) * 4u, blk = (y >> 3) * 2u + (x0 >> 3);
        const bool coded = (m.cbp >> (5 - blk)) & 1;
        const int px = (int)(16u * col + x0), py = (int)(16u * row + y);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t pred = intra ? 128 : dec::bp_predict(fwd, bwd, (int)W, px + j, py, dirs, m.mvx, m.mvy, m.bvx, m.bvy);
            const int32_t res = coded ? F[blk][(y & 7u) * 8u + ((x0 + j) & 7u)] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint32_t *)(cur + (size_t)(16u * row + y) * W + 16u * col + x0) = v;
    }
    {   // chroma: two samples per lane, U in the first half of the wavefront
        const uint32_t pl = l >> 5, y = (l >> 2) & 7u, x0 = (l & 3u) * 2u;
        const bool coded = (m.cbp >> (1 - pl)) & 1;
        const int fx = dec::chroma_vector(m.mvx, dec::kIso), fy = dec::chroma_vector(m.mvy, dec::kIso);
        const int bx = dec::chroma_vector(m.bvx, dec::kIso), by = dec::chroma_vector(m.bvy, dec::kIso);
        const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2u);
        const int px = (int)(8u * col + x0), py = (int)(8u * row + y);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t pred = intra ? 128 : dec::bp_predict(fwd + plane, bwd + plane, (int)CW, px + j, py, dirs, fx, fy, bx, by);
            const int32_t res = coded ? F[4u + pl][y * 8u + x0 + j] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint16_t *)(cur + plane + (size_t)(8u * row + y) * CW + 8u * col + x0) = (uint16_t)v;
    }
}

// picture blockIdx.y of chunk [p0, p0 + np) into dst at its display index: bytes [display * fb, (display + 1) * fb) of the output
__global__ __launch_bounds__(kDecThreads) void k_db_out(const DecState *__restrict__ st, const DecBPic *__restrict__ bp, const uint8_t *__restrict__ buf, size_t psz,
                                                        uint32_t p0, uint8_t *__restrict__ dst, int layout)
{
    if (st->status != dec::kOk) return;
    const uint32_t w = st->width, h = st->height, W = 16u * st->mbw, H = 16u * st->mbh;
    const uint32_t d = bp[p0 + blockIdx.y].display;
    if (d >= st->npics) return;                                        // (an accepted stream's display indices are a permutation)
    const unsigned long long fb = st->frame_bytes, lo = (unsigned long long)d * fb;
    out_picture(buf + (size_t)(blockIdx.y + 2u) * psz, w, h, W, H, lo, lo + fb, dst, layout, kDecThreads);
}

__global__ void k_db_finish(const DecState *st, m2v_decode_stat *h_rec)
{
    if (st->status == dec::kOk) { h_rec->out_bytes = st->frame_bytes * st->npics; return; }
    h_rec->status = st->status; h_rec->err_offset = st->err; h_rec->out_bytes = 0;
}

void dec_b_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main)
{
    k_db_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecBPic *)(d_main + kDecMainMatrices));
    HIPCHK(hipGetLastError());
}

// behind the plan's wait: R is the plan's record (OK, pictures > 0), B the pictures per chunk, types the picture types in coded
// order, h_list pinned room for one uint32 per picture
void dec_b_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t B, const uint8_t *types,
                  uint32_t *h_list, m2v_decode_stat *h_rec)
{
    const size_t np = R.pictures, mbw = (R.width + 15) / 16, mbh = (R.height + 15) / 16, mbs = mbw * mbh, psz = mbs * 384;
    e->d_dec_mb.ensure(B * mbs * sizeof(dec::BMb));
    e->d_dec_dc.ensure(B * mbs * 6);
    e->d_dec_lv.ensure(B * mbs * 384);
    e->d_dec_buf.ensure((B + 2) * psz);
    e->d_dec_list.ensure(np);
    const std::vector<DecChunk> chunks = dec_chunk_schedule(types, np, B, h_list);
    auto *d_st = (DecState *)e->d_dec_st.p;
    auto *d_mb = (dec::BMb *)e->d_dec_mb.p;
    const uint8_t *mats = e->d_dec_main.p;
    const auto *bp = (const DecBPic *)(e->d_dec_main.p + kDecMainMatrices);
    HIPCHK(hipMemcpyAsync(e->d_dec_list.p, h_list, np * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    for (size_t p0 = 0, c = 0; p0 < np; p0 += B, ++c) {
        const size_t nb = std::min(B, np - p0);
        const DecChunk &C = chunks[c];
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, nb * mbs * 768, s));
        k_db_slices<<<(unsigned)((nb * mbh + 63) / 64), 64, 0, s>>>(es, n, e->d_dec_ev.p, d_st, (const DecPic *)e->d_dec_pics.p, bp, (uint32_t)p0, (uint32_t)nb, d_mb,
                                                                    e->d_dec_dc.p, e->d_dec_lv.p);
        HIPCHK(hipGetLastError());
        k_db_judge<<<1, 1, 0, s>>>(d_st);
        HIPCHK(hipGetLastError());
        auto recon = [&](const DecLaunch &l) {
            if (!l.count) return;
            k_db_recon<<<dim3((unsigned)mbs, (unsigned)l.count), 64, 0, s>>>(d_st, e->d_dec_list.p + l.off, (uint32_t)p0, (uint32_t)C.c1, mats, bp, d_mb, e->d_dec_dc.p,
                                                                            e->d_dec_lv.p, e->d_dec_buf.p, psz);
            HIPCHK(hipGetLastError());
        };
        for (const DecLaunch &l : C.steps) recon(l);
        recon(C.b);                                                    // every B picture of the chunk at once: its anchors are done
        const size_t units = (R.frame_bytes + 15) / 16 + 1;
        k_db_out<<<dim3((unsigned)std::min<size_t>((units + kDecThreads - 1) / kDecThreads, 1024), (unsigned)nb), kDecThreads, 0, s>>>(d_st, bp, e->d_dec_buf.p, psz,
                                                                                                                                      (uint32_t)p0, dst, layout);
        HIPCHK(hipGetLastError());
        if (p0 + B < np) {                                             // the next chunk's carried anchors: slot 0 first (it may come from slot 1)
            if (C.carry0 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + (size_t)C.carry0 * psz, psz, hipMemcpyDeviceToDevice, s));
            if (C.carry1 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p + psz, e->d_dec_buf.p + (size_t)C.carry1 * psz, psz, hipMemcpyDeviceToDevice, s));
        }
    }
    k_db_finish<<<1, 1, 0, s>>>(d_st, h_rec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
}

}  // namespace m2v
