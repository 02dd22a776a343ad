// m2v_decode_i.hip — interlaced frame pictures for m2v_decode_device (option "decode_interlaced" = 1 on top of "decode_syntax" =
// M2V_SYNTAX_MAIN, with "decode_b_pictures" 0 or 1).  Modelled on m2v_decode_b.hip: m2v_decode.hip keeps the scan; this unit holds the
// plan and everything behind the plan's wait.  decoder.decode_main(interlaced=True) is the definition; every function that decides a bit
// or a sample is an il_ (or bp_ / main_) function of m2v_decode_kernels.hpp.
//
//   k_di_plan    k_db_plan with dec::il_first (the macroblock rows of a sequence that is not progressive), dec::il_event (a coding
//                extension may say frame_pred_frame_dct 0) and a flag for whether picture_coding_type 3 is accepted ("decode_b_pictures").
//                The macroblock rows go to the host beside the record: the chunk driver takes them from the plan, not from the height.
//   k_di_slices  one slice per lane (dec::il_slice): a picture with frame_pred_frame_dct 1 through dec::bp_slice, one with 0 with
//                macroblock_modes, four predictors and field vectors.  A record is 32 bytes (dec::IMb).
//   k_di_recon   one wavefront per macroblock with k_db_recon's lane mapping.  A lane's luma row y of a field-based macroblock takes
//                vector y & 1 and its field select and reads reference rows of one parity at twice the stride (dec::il_predict); the
//                residual of a field-DCT macroblock comes from block (y & 1) * 2 + (x >> 3), row y >> 1.  Chroma the same with four
//                lines per field; its blocks are frame blocks.  The body is imb_recon (m2v_decode_device.hpp), which the units of the
//                later options and the main-syntax batch entries call too.
//   k_di_out     as k_db_out: the shared output loop (out_picture) for the picture's frame at its display index.
//
// The chunk's buffer, the steps of the anchors and the single launch for a chunk's B pictures are m2v_decode_b.hip's; a stream without
// B pictures has display order = coded order there already.
#include "m2v_decode_state.hpp"

static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

__global__ __launch_bounds__(kDecThreads) void k_di_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecBPic *__restrict__ bp, int b_pictures, uint32_t *h_mbh)
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
    if (tid == 0) s_bad = dec::il_first(es, n, (const uint64_t *)ev, nev, s_P);
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
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0;
        int last = -1, a1 = -1, a2 = -1;           // the range's last I picture and its last two anchors, counted from its first picture
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dec::il_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev, b_pictures != 0);
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
                q.params = dec::il_picture_params(es, n, (const uint64_t *)ev, nev, i, b_pictures != 0, progressive, q.slice0);
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
    *h_mbh = P.mbh;
    *h_rec = r;
}

// as k_db_slices: pictures [p0, p0 + np) of any type, one slice per lane, the earliest refused slice lowers st->err
__global__ __launch_bounds__(64) void k_di_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                  const DecPic *__restrict__ pics, const DecBPic *__restrict__ bp, uint32_t p0, uint32_t np, dec::IMb *mb,
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
    IMbSink sink{mb + first, dc + first * 6, lv + first * 384};
    if (!dec::il_slice(es, start, end, P.type, dec::il_params_unpack(Q.params), (int)mbw, (int)mbh, (int)row, sink)) atomicMin(&st->err, start);
}

__global__ void k_di_judge(DecState *st)
{
    if (st->status == dec::kOk && st->err != dec::kNone) st->status = dec::kSyntax;
}

// as k_db_recon: grid = (macroblocks, pictures of the launch); list: their coded indices, all of chunk [p0, ...).  Every read of a
// reference lies inside its picture: the slice walk refused the slice otherwise (dec::il_inside), and a refused slice stops the call
// before this kernel (k_di_judge)
__global__ __launch_bounds__(64) void k_di_recon(const DecState *__restrict__ st, const uint32_t *__restrict__ list, uint32_t p0, uint32_t c1,
                                                 const uint8_t *__restrict__ mats, const DecBPic *__restrict__ bp, const dec::IMb *__restrict__ mb,
                                                 const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf, size_t psz)
{
    __shared__ int32_t F[6][64];
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, mbs = mbw * mbh, W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const uint32_t k = blockIdx.x, l = threadIdx.x, gp = list[blockIdx.y], pic = gp - p0;
    const DecBPic Q = bp[gp];
    const size_t at = (size_t)pic * mbs + k;
    imb_recon(F, mb[at], dec::params_unpack(Q.params), mats, dc, lv, at, buf + (size_t)(pic + 2u) * psz, buf + (size_t)slot(Q.fwd, p0, c1) * psz,
              buf + (size_t)slot(Q.bwd, p0, c1) * psz, W, H, CW, k % mbw, k / mbw, l);
}

// picture blockIdx.y of chunk [p0, p0 + np) into dst at its display index: bytes [display * fb, (display + 1) * fb) of the output
__global__ __launch_bounds__(kDecThreads) void k_di_out(const DecState *__restrict__ st, const DecBPic *__restrict__ bp, const uint8_t *__restrict__ buf, size_t psz,
                                                        uint32_t p0, uint8_t *__restrict__ dst, int layout)
{
    if (st->status != dec::kOk) return;
    const uint32_t w = st->width, h = st->height, W = 16u * st->mbw, H = 16u * st->mbh;
    const uint32_t d = bp[p0 + blockIdx.y].display;
    if (d >= st->npics) return;                                        // (an accepted stream's display indices are a permutation)
    const unsigned long long fb = st->frame_bytes, lo = (unsigned long long)d * fb;
    out_picture(buf + (size_t)(blockIdx.y + 2u) * psz, w, h, W, H, lo, lo + fb, dst, layout, kDecThreads);
}

__global__ void k_di_finish(const DecState *st, m2v_decode_stat *h_rec)
{
    if (st->status == dec::kOk) { h_rec->out_bytes = st->frame_bytes * st->npics; return; }
    h_rec->status = st->status; h_rec->err_offset = st->err; h_rec->out_bytes = 0;
}

void dec_i_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, uint32_t *h_mbh)
{
    k_di_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecBPic *)(d_main + kDecMainMatrices), b_pictures, h_mbh);
    HIPCHK(hipGetLastError());
}

// dec_b_chunks with the macroblock rows of the plan (mbh), records of 32 bytes and this unit's kernels; decode_batch 0: the default
// batch from these rows
void dec_i_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t mbh, size_t B,
                  const uint8_t *types, uint32_t *h_list, m2v_decode_stat *h_rec)
{
    const size_t np = R.pictures, mbw = (R.width + 15) / 16, mbs = mbw * mbh, psz = mbs * 384;
    e->d_dec_mb.ensure(B * mbs * sizeof(dec::IMb));
    e->d_dec_dc.ensure(B * mbs * 6);
    e->d_dec_lv.ensure(B * mbs * 384);
    e->d_dec_buf.ensure((B + 2) * psz);
    e->d_dec_list.ensure(np);
    const std::vector<DecChunk> chunks = dec_chunk_schedule(types, np, B, h_list);
    auto *d_st = (DecState *)e->d_dec_st.p;
    auto *d_mb = (dec::IMb *)e->d_dec_mb.p;
    const uint8_t *mats = e->d_dec_main.p;
    const auto *bp = (const DecBPic *)(e->d_dec_main.p + kDecMainMatrices);
    HIPCHK(hipMemcpyAsync(e->d_dec_list.p, h_list, np * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    for (size_t p0 = 0, c = 0; p0 < np; p0 += B, ++c) {
        const size_t nb = std::min(B, np - p0);
        const DecChunk &C = chunks[c];
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, nb * mbs * 768, s));
        k_di_slices<<<(unsigned)((nb * mbh + 63) / 64), 64, 0, s>>>(es, n, e->d_dec_ev.p, d_st, (const DecPic *)e->d_dec_pics.p, bp, (uint32_t)p0, (uint32_t)nb, d_mb,
                                                                    e->d_dec_dc.p, e->d_dec_lv.p);
        HIPCHK(hipGetLastError());
        k_di_judge<<<1, 1, 0, s>>>(d_st);
        HIPCHK(hipGetLastError());
        auto recon = [&](const DecLaunch &l) {
            if (!l.count) return;
            k_di_recon<<<dim3((unsigned)mbs, (unsigned)l.count), 64, 0, s>>>(d_st, e->d_dec_list.p + l.off, (uint32_t)p0, (uint32_t)C.c1, mats, bp, d_mb, e->d_dec_dc.p,
                                                                            e->d_dec_lv.p, e->d_dec_buf.p, psz);
            HIPCHK(hipGetLastError());
        };
        for (const DecLaunch &l : C.steps) recon(l);
        recon(C.b);                                                    // every B picture of the chunk at once: its anchors are done
        const size_t units = (R.frame_bytes + 15) / 16 + 1;
        k_di_out<<<dim3((unsigned)std::min<size_t>((units + kDecThreads - 1) / kDecThreads, 1024), (unsigned)nb), kDecThreads, 0, s>>>(d_st, bp, e->d_dec_buf.p, psz,
                                                                                                                                      (uint32_t)p0, dst, layout);
        HIPCHK(hipGetLastError());
        if (p0 + B < np) {                                             // the next chunk's carried anchors: slot 0 first (it may come from slot 1)
            if (C.carry0 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + (size_t)C.carry0 * psz, psz, hipMemcpyDeviceToDevice, s));
            if (C.carry1 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p + psz, e->d_dec_buf.p + (size_t)C.carry1 * psz, psz, hipMemcpyDeviceToDevice, s));
        }
    }
    k_di_finish<<<1, 1, 0, s>>>(d_st, h_rec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
}

}  // namespace m2v
