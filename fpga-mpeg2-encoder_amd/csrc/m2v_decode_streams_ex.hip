// m2v_decode_streams_ex.hip — a batch of main-syntax streams with the extended options in one call (include/m2v_mi355x.h:
// m2v_decode_streams_main_ex_device): the pipeline of m2v_decode_streams_main.hip over the x_ / t_ functions of m2v_decode_kernels.hpp,
// each stream judged alone as m2v_decode_device judges it with "decode_syntax" = main and the four options set as the call's flags say.
// With flags below M2V_DECS_EXTENDED the entry hands the call to m2v_decode_streams_main_device as it stands.  The first
// pass up to the plan's wait and the output kernel are that unit's (ds_main_first, dsm_out); the scan, the judge, the finish and the
// report are m2v_decode_streams.hip's.
//
//   k_dsx_plan    one block per stream: k_dx_plan's grammar with the stream's own segment, events, picture table and record.  flag 8:
//                 dec::t_event / t_picture_params, else dec::x_event / x_picture_params (a packing without the three flags above bit 20
//                 leaves them 0).  256 ranges of ceil(events / 256); carried from range to range: the last significant event, the last I
//                 picture, the anchors, the events that loaded each matrix with the sequence header's reset, the earliest refusal.  Per
//                 picture: its first slice's event, its slices, its packed parameters, the events that loaded its matrices; its type and
//                 its slices to pinned memory.  Per stream: the record, the macroblock rows, the sequence's matrices at mats[stream * 128].
//                 Display indices, references and the slices in front of a picture follow from the types and the counts alone; the host
//                 derives them where it lays the batch out (dec::plan_streams_main_ex).
//   k_dsx_mats    the matrix table, 128 bytes a picture, indexed by the picture's entry in the call's table of chunk pictures: every
//                 picture of every stream in one launch, from its stream's sequence matrices or the extension that loaded each.
//   k_dsx_slices  one lane per slice EVENT of the chunk, across all streams: its picture by binary search over the table's cumulative
//                 slice0, its number inside the picture from there.  dec::t_slice under flag 8, dec::x_slice without, into the row its
//                 code names; the lane leaves its span.  STORE false: the verdict pass over the streams a chunk's edge cuts.
//   k_dsx_cont    one lane per slice again: dec::x_continuous against the span of the slice in front inside its picture; lowers its
//                 stream's err.  Runs in the verdict pass too: a slice that breaks continuity is refused at its own start code.
//   k_dsx_recon   k_dsm_recon with the weights from the picture's row of the matrix table; a P picture's second prediction reads
//                 bwd = fwd (dual prime).  Anchors step by step, then every B picture of the chunk in one launch.
#include "m2v_decode_state.hpp"
#include "m2v_decode_streams.hpp"
#include "m2v_decode_streams_ex.hpp"

static_assert(sizeof(dec::MainChunkPic) == 88, "a chunk's picture is 88 bytes");
static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

constexpr int kDsxThreads = 256;
typedef unsigned long long ull;

// a picture: the event of its first slice, dec::t_params_pack, its slice events, the events that loaded its matrices (kNoEvent: the sequence's)
struct DsxPic { uint32_t slice0, params, nslices, mi, mn; };
constexpr uint32_t kDsxMatrices = 128;

// one block per stream.  Whether the frames fit is the host's to say, behind the wait (the rooms depend on the streams in front)
__global__ __launch_bounds__(kDsxThreads) void k_dsx_plan(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts,
                                                          DsxPic *__restrict__ pics_all, uint8_t *h_types_all, uint32_t *h_sl_all, m2v_decode_stat *h_recs, uint32_t *h_mbh,
                                                          uint8_t *__restrict__ mats_all, unsigned flags)
{
    __shared__ dec::MainPlan s_P;
    __shared__ ull s_bad;
    __shared__ uint32_t s_np[kDsxThreads], s_ng[kDsxThreads], s_nr[kDsxThreads], s_ni[kDsxThreads], s_na[kDsxThreads];
    __shared__ int s_last[kDsxThreads], s_sig[kDsxThreads];
    __shared__ uint32_t s_mi[kDsxThreads], s_mn[kDsxThreads], s_rs[kDsxThreads];      // the events that loaded the matrices; a reset
    const DsIn S = in[blockIdx.x];
    DsState *st = sts + blockIdx.x;
    m2v_decode_stat *h_rec = h_recs + blockIdx.x;
    const uint8_t *es = base + S.off;
    const ull *ev = evs + S.ev_base, n = S.n;
    DsxPic *pics = pics_all + S.pic_base;
    uint8_t *h_types = h_types_all + S.pic_base;
    uint32_t *h_sl = h_sl_all + S.pic_base;
    uint8_t *mats = mats_all + (size_t)blockIdx.x * kDsxMatrices;
    const uint32_t pic_cap = S.pic_cap;
    const uint32_t tid = threadIdx.x, nev = st->nev;
    const bool interlaced = (flags & M2V_DECS_INTERLACED) != 0, b_pictures = (flags & M2V_DECS_B_PICTURES) != 0, tools = (flags & M2V_DECS_MB_TOOLS) != 0;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (tid == 0) h_mbh[blockIdx.x] = 0;
    if (n < 4) {                                   // not one start code
        if (tid == 0) { st->status = dec::kSyntax; st->err = 0; r.status = dec::kSyntax; *h_rec = r; }
        return;
    }
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
    const ull last_nz = st->last_nz;
    const uint32_t per = (nev + kDsxThreads - 1) / kDsxThreads, a = min(nev, tid * per), b = min(nev, a + per);
    {   // the last significant event of every range
        int sig = -1;
        for (uint32_t i = a; i < b; ++i) if (dec::main_significant(dec::main_role(es, n, ev[i]))) sig = (int)i;
        s_sig[tid] = sig;
    }
    __syncthreads();
    {
        int prev = -1;                             // the significant event in front of this range
        for (int k = (int)tid - 1; k >= 0 && prev < 0; --k) prev = s_sig[k];
        ull bad = dec::kNone;
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0, reset = 0;
        dec::XMats xm{dec::kNoEvent, dec::kNoEvent};           // what the range's events loaded behind its last sequence header
        int last = -1;                             // the range's last I picture, counted from its first picture
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = tools ? dec::t_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev, b_pictures, interlaced)
                                        : dec::x_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev, b_pictures, interlaced);
            const int role = dec::main_role(es, n, ev[i]);
            if (dec::main_significant(role)) prev = (int)i;
            reset |= role == dec::rSeq;
            dec::x_mats_event(es, n, (const uint64_t *)ev, nev, i, xm);
            bad = dec::min64(bad, f.bad);
            ng += f.gop; nr += f.rep;
            if (f.pic) {
                if (f.type == 1) { last = (int)np; ++ni; }
                if (f.type != 3) ++na;
                ++np;
            }
        }
        if (bad != dec::kNone) atomicMin(&s_bad, bad);
        s_np[tid] = np; s_ng[tid] = ng; s_nr[tid] = nr; s_ni[tid] = ni; s_na[tid] = na; s_last[tid] = last;
        s_mi[tid] = xm.mi; s_mn[tid] = xm.mn; s_rs[tid] = reset;
    }
    __syncthreads();
    if (tid == 0) {                                // exclusive sums; the last I picture and the matrices in force in front of every range
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0, mi = dec::kNoEvent, mn = dec::kNoEvent;
        int last = -1;
        for (int k = 0; k < kDsxThreads; ++k) {
            const uint32_t p = s_np[k], c = s_na[k], ki = s_mi[k], kn = s_mn[k];
            const int l = s_last[k];
            s_np[k] = np; s_na[k] = na; s_last[k] = last; s_mi[k] = mi; s_mn[k] = mn;
            if (s_rs[k]) { mi = ki; mn = kn; }         // a sequence header in the range: only what was loaded behind it
            else { if (ki != dec::kNoEvent) mi = ki; if (kn != dec::kNoEvent) mn = kn; }
            if (l >= 0) last = (int)np + l;
            np += p; na += c; ni += s_ni[k]; ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = np; r.gops = ng; r.repeated_headers = nr; r.chains = ni;
    }
    __syncthreads();
    {
        uint32_t p = s_np[tid], anchors = s_na[tid];
        int last = s_last[tid];
        dec::XMats xm{s_mi[tid], s_mn[tid]};                   // the matrices in force in front of event i
        for (uint32_t i = a; i < b; ++i) {
            const uint32_t code = dec::ev_code(ev[i]);
            if (code != 0x00) {
                if (code == 0xB3u || code == 0xB5u) dec::x_mats_event(es, n, (const uint64_t *)ev, nev, i, xm);
                continue;
            }
            const ull pos = dec::ev_pos(ev[i]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            if (type == 1) last = (int)p;
            if (last < 0) atomicMin(&s_bad, pos);                      // a P picture without a reference
            if (type == 3 && anchors < 2u) atomicMin(&s_bad, pos);     // a B picture without two anchors in front of it
            if (p < pic_cap) {
                DsxPic q;
                uint32_t quant;
                q.params = tools ? dec::t_picture_params(es, n, (const uint64_t *)ev, nev, i, b_pictures, interlaced, progressive, q.slice0, q.nslices, quant)
                                 : dec::x_picture_params(es, n, (const uint64_t *)ev, nev, i, b_pictures, interlaced, progressive, q.slice0, q.nslices, quant);
                const dec::XMats own = dec::x_mats_picture(es, n, (const uint64_t *)ev, nev, xm, quant);
                q.mi = own.mi; q.mn = own.mn;
                pics[p] = q; h_types[p] = (uint8_t)type; h_sl[p] = q.nslices;
            }
            if (type != 3) ++anchors;
            ++p;
        }
    }
    __syncthreads();
    if (tid) return;
    const dec::SeqHdr &h = P.seq.h;
    r.width = h.width; r.height = h.height;
    r.frame_bytes = dec::frame_bytes(h.width, h.height);
    if (s_bad != dec::kNone) { r.status = dec::kSyntax; r.err_offset = s_bad; }
    else if (r.pictures > pic_cap) { r.status = dec::kSyntax; r.err_offset = 0; }      // (cannot happen: a picture is three events at least)
    st->status = r.status; st->err = s_bad; st->mbw = P.mbw; st->mbh = P.mbh;
    h_mbh[blockIdx.x] = P.mbh;
    *h_rec = r;
}

// the matrix table: entry p of the call's table of chunk pictures gets its picture's 128 weights, raster order - its stream's
// sequence matrices, or those of the extension in force.  One thread per weight, the blocks stride over the table
__global__ __launch_bounds__(128) void k_dsx_mats(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs,
                                                  const DsState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, uint32_t ntab,
                                                  const DsxPic *__restrict__ pics, const uint8_t *__restrict__ mats_all, uint8_t *__restrict__ table)
{
    const uint32_t l = threadIdx.x, m = l >> 6, t = l & 63u;
    for (uint32_t p = blockIdx.x; p < ntab; p += gridDim.x) {
        const dec::MainChunkPic C = tab[p];
        const DsState *st = sts + C.stream;
        if (st->status != dec::kOk) continue;
        const DsIn S = in[C.stream];
        const DsxPic Q = pics[C.gpic];
        table[(size_t)p * 128u + l] = (uint8_t)dec::x_matrix_weight(base + S.off, S.n, (const uint64_t *)(evs + S.ev_base), st->nev, m ? Q.mn : Q.mi, (int)m, t,
                                                                     mats_all + (size_t)C.stream * kDsxMatrices + 64u * m);
    }
}

// the nslices slice events of the table's pictures, one per lane, each into the row its code names.  The lane leaves its span (0: not
// walked); a slice that cannot be read lowers its stream's err, which no lane of the launch reads.  Two slices that overlap write the
// same records - the judge refuses the stream before anything reads them.  STORE false: for the verdict alone
template <bool STORE, bool TOOLS>
__global__ __launch_bounds__(64) void k_dsx_slices(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts,
                                                   const DsxPic *__restrict__ pics, const dec::MainChunkPic *__restrict__ tab, uint32_t ntab, uint32_t nslices,
                                                   dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *__restrict__ spans)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= nslices) return;
    spans[g] = 0u;
    const dec::MainChunkPic C = tab[dec::main_chunk_slice_pic(tab, ntab, g)];
    DsState *st = sts + C.stream;
    if (st->status != dec::kOk) return;
    const DsIn S = in[C.stream];
    const DsxPic Q = pics[C.gpic];
    const uint32_t k = g - C.slice0, nev = st->nev;
    const uint32_t i = Q.slice0 + k;
    if (k >= Q.nslices || i >= nev) return;                            // (the plan accepted the picture: its slices are there)
    const ull *ev = evs + S.ev_base;
    const ull start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : S.n;
    const uint32_t code = dec::ev_code(ev[i]);
    if (code < 1u || code > C.mbh) { atomicMin(&st->err, start); return; }      // (the plan's grammar: 1 <= code <= mbh)
    const uint8_t *es = base + S.off;
    int c0, c1;
    bool ok;
    if (STORE) {
        const size_t first = (size_t)C.mb_base + (size_t)(code - 1u) * C.mbw;
        IMbSink sink{mb + first, dc + first * 6, lv + first * 384};
        ok = TOOLS ? dec::t_slice(es, start, end, C.type, dec::t_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1)
                   : dec::x_slice(es, start, end, C.type, dec::il_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1);
    } else {
        IMbNoSink sink;
        ok = TOOLS ? dec::t_slice(es, start, end, C.type, dec::t_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1)
                   : dec::x_slice(es, start, end, C.type, dec::il_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1);
    }
    spans[g] = dec::x_span_pack(ok, code, c0, c1);
    if (!ok) atomicMin(&st->err, start);
}

// continuity behind the walk: every readable slice against the span of the slice in front of it in its picture
__global__ __launch_bounds__(64) void k_dsx_cont(const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts, const DsxPic *__restrict__ pics,
                                                 const dec::MainChunkPic *__restrict__ tab, uint32_t ntab, uint32_t nslices, const uint32_t *__restrict__ spans)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= nslices) return;
    const dec::MainChunkPic C = tab[dec::main_chunk_slice_pic(tab, ntab, g)];
    DsState *st = sts + C.stream;
    if (st->status != dec::kOk) return;
    const DsxPic Q = pics[C.gpic];
    const uint32_t k = g - C.slice0, cur = spans[g];
    if (!(cur >> 31) || k >= Q.nslices || Q.slice0 + k >= st->nev) return;      // (not readable: reported by its walk)
    if (!dec::x_continuous(cur, k ? spans[g - 1] : 0u, k, Q.nslices, C.mbw)) atomicMin(&st->err, dec::ev_pos(evs[in[C.stream].ev_base + Q.slice0 + k]));
}

// grid = (the most macroblocks of a picture of the launch, its pictures); list: their entries of the chunk's table; table: the chunk's
// rows of the matrix table.  Every read of a reference lies inside its picture: the slice walk refused the slice otherwise
// (dec::il_inside), and a refused slice makes its stream's status not OK before this kernel (k_ds_judge)
__global__ __launch_bounds__(64) void k_dsx_recon(const DsState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, const uint32_t *__restrict__ list,
                                                  const DsxPic *__restrict__ pics, const uint8_t *__restrict__ table, const dec::IMb *__restrict__ mb,
                                                  const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf)
{
    __shared__ int32_t F[6][64];
    const uint32_t entry = list[blockIdx.y];
    const dec::MainChunkPic C = tab[entry];
    const uint32_t mbw = C.mbw, mbh = C.mbh, k = blockIdx.x, l = threadIdx.x;
    if (k >= mbw * mbh) return;                                        // (a smaller picture of the launch; the whole workgroup leaves)
    if (sts[C.stream].status != dec::kOk) return;
    const uint32_t W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const size_t at = (size_t)C.mb_base + k;
    imb_recon(F, mb[at], dec::params_unpack(pics[C.gpic].params), table + (size_t)entry * 128u, dc, lv, at, buf + C.buf_off, buf + C.fwd_off, buf + C.bwd_off, W, H, CW,
              k % mbw, k / mbw, l);
}

}  // namespace m2v

struct DecodeStreamsExArgs { const uint8_t *es; const uint64_t *off, *bytes; size_t n; uint8_t *dst; size_t cap; int layout; unsigned flags; hipStream_t s; };

static int decode_streams_ex_impl(m2v_enc *e, void *argp)
{
    auto *a = (DecodeStreamsExArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    const size_t n = a->n;
    const bool tools = (a->flags & M2V_DECS_MB_TOOLS) != 0;
    e->ds_q.clear();
    // the work buffers are m2v_decode_device's and the other batch entries' (all these calls block; no recorded graph references them)
    e->d_dec_st.recorded = e->d_dec_ev.recorded = e->d_dec_pics.recorded = e->d_dec_mb.recorded = e->d_dec_dc.recorded = false;
    e->d_dec_lv.recorded = e->d_dec_buf.recorded = e->d_dec_tiles.recorded = e->d_dec_list.recorded = e->d_dec_main.recorded = false;
    e->d_ds_in.recorded = e->d_ds_tab.recorded = e->d_dec_x.recorded = false;
    DsMainFirst F;
    const int err = ds_main_first(e, s, "m2v_decode_streams_main_ex_device", a->es, a->off, a->bytes, n, sizeof(DsxPic), true,
                                  [&](const DsIn *d_in, DsState *d_st, uint8_t *h_types, uint32_t *h_sl, m2v_decode_stat *h_rec, uint32_t *h_mbh) {
        k_dsx_plan<<<(unsigned)n, kDsxThreads, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, (DsxPic *)e->d_dec_pics.p, h_types, h_sl, h_rec, h_mbh, e->d_dec_main.p, a->flags);
    }, F);
    if (err != M2V_OK) return err;
    const std::vector<m2v_decode_stat> &rec = F.rec;
    const std::vector<size_t> &pic_base = F.pic_base;
    std::vector<dec::ExStreamInfo> info(n);
    for (size_t b = 0; b < n; ++b) {
        info[b] = dec::ExStreamInfo{dec::MainStreamInfo{rec[b].status, rec[b].pictures, rec[b].width, rec[b].height, F.mbh[b], F.types.data() + pic_base[b]},
                                    F.nsl.data() + pic_base[b]};
    }
    dec::MainStreamsPlan P = dec::plan_streams_main_ex(info.data(), n, a->cap, a->dst == nullptr, e->decode_batch, (a->flags & M2V_DECS_B_PICTURES) != 0, tools);
    for (dec::MainChunkPic &c : P.pics) c.gpic = (uint32_t)(pic_base[c.stream] + c.pic);
    for (dec::MainChunkPic &c : P.pre) c.gpic = (uint32_t)(pic_base[c.stream] + c.pic);
    if (!a->dst || P.pics.empty()) { ds_report(e, a->off, n, P.out_offset, P.overflow, rec, nullptr); return M2V_OK; }
    if (P.pics.size() > 0xFFFFFFFFull) { e->set_err("m2v_decode_streams_main_ex_device: more than 2^32 pictures"); return M2V_E_PARAM; }
    const size_t tab_bytes = ds_up64(P.pics.size() * sizeof(dec::MainChunkPic)), pre_bytes = ds_up64(P.pre.size() * sizeof(dec::MainChunkPic)),
                 list_bytes = ds_up64(P.list.size() * sizeof(uint32_t));
    ensure_pinned(e->h_ds_tab, e->h_ds_tab_cap, tab_bytes + pre_bytes + list_bytes + n * sizeof(DsVerdict) + 64);
    memcpy(e->h_ds_tab, P.pics.data(), P.pics.size() * sizeof(dec::MainChunkPic));
    if (!P.pre.empty()) memcpy(e->h_ds_tab + tab_bytes, P.pre.data(), P.pre.size() * sizeof(dec::MainChunkPic));
    memcpy(e->h_ds_tab + tab_bytes + pre_bytes, P.list.data(), P.list.size() * sizeof(uint32_t));
    auto *h_v = (DsVerdict *)(e->h_ds_tab + tab_bytes + pre_bytes + list_bytes);
    e->d_ds_tab.ensure(tab_bytes + pre_bytes + list_bytes);
    HIPCHK(hipMemcpyAsync(e->d_ds_tab.p, e->h_ds_tab, tab_bytes + pre_bytes + list_bytes, hipMemcpyHostToDevice, s));
    uint64_t most_mbs = 0, most_buf = 0, most_slices = P.pre_slices;
    for (const dec::MainStreamsChunk &C : P.chunks) {
        most_mbs = std::max(most_mbs, C.mbs); most_buf = std::max(most_buf, C.buf_bytes); most_slices = std::max<uint64_t>(most_slices, C.slices);
    }
    const size_t span_off = ds_up64(P.pics.size() * 128);             // the matrix table, then the spans of a launch's slices
    e->d_dec_x.ensure(span_off + std::max<size_t>(most_slices, 1) * sizeof(uint32_t));
    e->d_dec_mb.ensure(most_mbs * sizeof(dec::IMb));
    e->d_dec_dc.ensure(most_mbs * 6);
    e->d_dec_lv.ensure(most_mbs * 384);
    e->d_dec_buf.ensure(most_buf);
    auto *d_in = (const DsIn *)e->d_ds_in.p;
    auto *d_st = (DsState *)e->d_dec_st.p;
    auto *d_mb = (dec::IMb *)e->d_dec_mb.p;
    auto *d_pics = (const DsxPic *)e->d_dec_pics.p;
    auto *d_tab = (const dec::MainChunkPic *)e->d_ds_tab.p;
    auto *d_pre = (const dec::MainChunkPic *)(e->d_ds_tab.p + tab_bytes);
    auto *d_list = (const uint32_t *)(e->d_ds_tab.p + tab_bytes + pre_bytes);
    uint8_t *d_table = e->d_dec_x.p;
    auto *d_spans = (uint32_t *)(e->d_dec_x.p + span_off);
    auto walk = [&](bool store, const dec::MainChunkPic *tab, uint32_t ntab, uint32_t nslices) {
        const unsigned g = (nslices + 63u) / 64u;
        if (store && tools) k_dsx_slices<true, true><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, d_mb, e->d_dec_dc.p, e->d_dec_lv.p, d_spans);
        else if (store) k_dsx_slices<true, false><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, d_mb, e->d_dec_dc.p, e->d_dec_lv.p, d_spans);
        else if (tools) k_dsx_slices<false, true><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, nullptr, nullptr, nullptr, d_spans);
        else k_dsx_slices<false, false><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, nullptr, nullptr, nullptr, d_spans);
        HIPCHK(hipGetLastError());
        k_dsx_cont<<<g, 64, 0, s>>>(d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, d_spans);
        HIPCHK(hipGetLastError());
        ds_judge(s, d_st, n);
    };
    if (P.pre_slices) walk(false, d_pre, (uint32_t)P.pre.size(), P.pre_slices);
    k_dsx_mats<<<(unsigned)std::min<size_t>(P.pics.size(), 1u << 20), 128, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_tab, (uint32_t)P.pics.size(), d_pics, e->d_dec_main.p,
                                                                                 d_table);
    HIPCHK(hipGetLastError());
    for (const dec::MainStreamsChunk &C : P.chunks) {
        const dec::MainChunkPic *tab = d_tab + C.first;
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, C.mbs * 768, s));
        if (C.slices) walk(true, tab, (uint32_t)C.count, C.slices);
        auto recon = [&](const dec::MainStreamsChunk::Step &S) {
            for (size_t y = 0; y < S.count; y += 65535) {             // (a grid's second dimension ends there)
                k_dsx_recon<<<dim3(S.most_mbs, (unsigned)std::min<size_t>(S.count - y, 65535)), 64, 0, s>>>(d_st, tab, d_list + S.off + y, d_pics, d_table + C.first * 128,
                                                                                                          d_mb, e->d_dec_dc.p, e->d_dec_lv.p, e->d_dec_buf.p);
                HIPCHK(hipGetLastError());
            }
        };
        for (const dec::MainStreamsChunk::Step &S : C.steps) recon(S);
        recon(C.b);                                                   // every B picture of the chunk, of all streams, at once: their anchors are done
        dsm_out(s, d_st, tab, C.count, C.most_units, e->d_dec_buf.p, a->dst, a->layout);
        // the next chunk's carried anchors: slot 0 first (it may come from slot 1)
        if (C.carry0_from >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + C.carry0_from, C.carry_bytes, hipMemcpyDeviceToDevice, s));
        if (C.carry1_from >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p + P.carry, e->d_dec_buf.p + C.carry1_from, C.carry_bytes, hipMemcpyDeviceToDevice, s));
    }
    ds_finish(s, d_st, n, h_v);
    HIPCHK(hipStreamSynchronize(s));
    ds_report(e, a->off, n, P.out_offset, P.overflow, rec, h_v);
    return M2V_OK;
}

extern "C" {

int m2v_decode_streams_main_ex_device(m2v_enc *e, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams, void *d_dst, size_t cap,
                                      int layout, unsigned flags, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    if (nstreams < 1 || nstreams > 65535) { e->set_err("m2v_decode_streams_main_ex_device: nstreams is 1 .. 65535, not %zu", nstreams); return M2V_E_PARAM; }
    if (!es_off || !es_bytes) { e->set_err("m2v_decode_streams_main_ex_device: es_off / es_bytes is NULL"); return M2V_E_PARAM; }
    if (!layout420_ok(layout)) { e->set_err("m2v_decode_streams_main_ex_device: unknown layout %d", layout); return M2V_E_PARAM; }
    if (flags & ~(unsigned)(M2V_DECS_B_PICTURES | M2V_DECS_INTERLACED | M2V_DECS_EXTENDED | M2V_DECS_MB_TOOLS)) {
        e->set_err("m2v_decode_streams_main_ex_device: flags are M2V_DECS_B_PICTURES | M2V_DECS_INTERLACED | M2V_DECS_EXTENDED | M2V_DECS_MB_TOOLS, not 0x%x", flags);
        return M2V_E_PARAM;
    }
    if ((flags & M2V_DECS_MB_TOOLS) && !(flags & M2V_DECS_EXTENDED)) {
        e->set_err("m2v_decode_streams_main_ex_device: M2V_DECS_MB_TOOLS needs M2V_DECS_EXTENDED");
        return M2V_E_PARAM;
    }
    if (!d_es) for (size_t b = 0; b < nstreams; ++b) if (es_bytes[b]) { e->set_err("m2v_decode_streams_main_ex_device: d_es is NULL"); return M2V_E_PARAM; }
    if (in_progress(e, "m2v_decode_streams_main_ex_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    // without the extended options: the existing implementation, its kernels and its launches
    if (!(flags & M2V_DECS_EXTENDED)) return m2v_decode_streams_main_device(e, d_es, es_off, es_bytes, nstreams, d_dst, cap, layout, flags, hip_stream);
    DecodeStreamsExArgs a{(const uint8_t *)d_es, es_off, es_bytes, nstreams, (uint8_t *)d_dst, cap, layout, flags, (hipStream_t)hip_stream};
    return guard(e, decode_streams_ex_impl, &a);
}

}  // extern "C"
