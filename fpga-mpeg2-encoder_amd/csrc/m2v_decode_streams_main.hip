// m2v_decode_streams_main.hip — a batch of main-syntax streams back to 4:2:0 frames in one call (include/m2v_mi355x.h:
// m2v_decode_streams_main_device): the pipeline of m2v_decode_streams.hip over the main_ / bp_ / il_ functions of
// m2v_decode_kernels.hpp, each stream judged alone as m2v_decode_device judges it with "decode_syntax" = main and the two options set
// as the call's flags say.  The scan, the judge, the finish and the report are m2v_decode_streams.hip's (ds_scan, ds_judge, ds_finish,
// ds_report); the first pass up to the plan's wait (ds_main_first) and the output kernel (dsm_out) live here and serve
// m2v_decode_streams_ex.hip too.
//
//   k_dsm_plan    one block per stream: k_di_plan's grammar with the stream's own segment, events, picture table and record.  flag 2:
//                 dec::il_first / il_event / il_picture_params; flag 1 alone: main_first / bp_event / bp_picture_params; neither:
//                 main_first / main_event / main_picture_params.  Per picture: its first slice's event and its packed parameters (all
//                 three packings unpack through dec::il_params_unpack: a packing without the field bit or the backward f_codes leaves
//                 them 0), its type to pinned memory.  Per stream: the record, the macroblock rows, the two matrices at
//                 mats[stream * 128].  Display indices and references follow from the types alone; the host derives them where it
//                 lays the batch out (dec::plan_streams_main), since the rooms and the slots need them there anyway.
//   k_dsm_slices  one kernel over dec::il_slice, one slice per lane, every parameter per lane.  il_slice hands a picture without the
//                 field bit to bp_slice, and bp_slice hands one that is not a B picture to main_slice: with flag 2 off no accepted
//                 stream has the field bit (its coding extension was refused), with flag 1 off none has a B picture (its header was
//                 refused), so the walk and its refusals are bp_slice's, or main_slice's, exactly.
//   k_dsm_recon   imb_recon (m2v_decode_device.hpp) per picture of a step: the picture's own slot, the slots of its references
//                 (dec::MainChunkPic), the matrices of its stream.  Anchors step by step, then every B picture of the chunk in one launch.
//   k_dsm_out     out_picture over (units, pictures): every picture to out_offset[stream] + display * frame_bytes - a chunk's frames
//                 are no contiguous range.  16-byte stores where a unit lies inside one frame, bytes at a frame's edges.
#include "m2v_decode_state.hpp"
#include "m2v_decode_streams.hpp"
#include "m2v_decode_streams_main.hpp"

static_assert(sizeof(dec::MainChunkPic) == 88, "a chunk's picture is 88 bytes");
static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

constexpr int kDsmThreads = 256;
typedef unsigned long long ull;

struct DsmPic { uint32_t slice0, params; };
constexpr uint32_t kDsmMatrices = 128;

// event i of a stream by the call's flags
__device__ inline dec::EvInfo dsm_event(const uint8_t *es, ull n, const ull *ev, uint32_t nev, uint32_t i, const dec::MainPlan &P, ull last_nz, int prev, unsigned flags)
{
    if (flags & M2V_DECS_INTERLACED) return dec::il_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev, (flags & M2V_DECS_B_PICTURES) != 0);
    if (flags & M2V_DECS_B_PICTURES) return dec::bp_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev);
    return dec::main_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev);
}

// one block per stream.  Whether the frames fit is the host's to say, behind the wait (the rooms depend on the streams in front)
__global__ __launch_bounds__(kDsmThreads) void k_dsm_plan(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts,
                                                          DsmPic *__restrict__ pics_all, uint8_t *h_types_all, m2v_decode_stat *h_recs, uint32_t *h_mbh,
                                                          uint8_t *__restrict__ mats_all, unsigned flags)
{
    __shared__ dec::MainPlan s_P;
    __shared__ ull s_bad;
    __shared__ uint32_t s_np[kDsmThreads], s_ng[kDsmThreads], s_nr[kDsmThreads], s_ni[kDsmThreads], s_na[kDsmThreads];
    __shared__ int s_last[kDsmThreads], s_sig[kDsmThreads];
    const DsIn S = in[blockIdx.x];
    DsState *st = sts + blockIdx.x;
    m2v_decode_stat *h_rec = h_recs + blockIdx.x;
    const uint8_t *es = base + S.off;
    const ull *ev = evs + S.ev_base, n = S.n;
    DsmPic *pics = pics_all + S.pic_base;
    uint8_t *h_types = h_types_all + S.pic_base;
    uint8_t *mats = mats_all + (size_t)blockIdx.x * kDsmMatrices;
    const uint32_t pic_cap = S.pic_cap;
    const uint32_t tid = threadIdx.x, nev = st->nev;
    const bool interlaced = (flags & M2V_DECS_INTERLACED) != 0, b_pictures = (flags & M2V_DECS_B_PICTURES) != 0;
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
    const uint32_t per = (nev + kDsmThreads - 1) / kDsmThreads, a = min(nev, tid * per), b = min(nev, a + per);
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
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0;
        int last = -1;                             // the range's last I picture, counted from its first picture
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dsm_event(es, n, ev, nev, i, P, last_nz, prev, flags);
            if (dec::main_significant(dec::main_role(es, n, ev[i]))) prev = (int)i;
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
    }
    __syncthreads();
    if (tid == 0) {                                // exclusive sums; the last I picture in front of every range (-1: none)
        uint32_t np = 0, ng = 0, nr = 0, ni = 0, na = 0;
        int last = -1;
        for (int k = 0; k < kDsmThreads; ++k) {
            const uint32_t p = s_np[k], c = s_na[k];
            const int l = s_last[k];
            s_np[k] = np; s_na[k] = na; s_last[k] = last;
            if (l >= 0) last = (int)np + l;
            np += p; na += c; ni += s_ni[k]; ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = np; r.gops = ng; r.repeated_headers = nr; r.chains = ni;
    }
    __syncthreads();
    {
        uint32_t p = s_np[tid], anchors = s_na[tid];
        int last = s_last[tid];
        for (uint32_t i = a; i < b; ++i) {
            if (dec::ev_code(ev[i]) != 0x00) continue;
            const ull pos = dec::ev_pos(ev[i]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            if (type == 1) last = (int)p;
            if (last < 0) atomicMin(&s_bad, pos);                      // a P picture without a reference
            if (type == 3 && anchors < 2u) atomicMin(&s_bad, pos);     // a B picture without two anchors in front of it
            if (p < pic_cap) {
                DsmPic q;
                if (interlaced) q.params = dec::il_picture_params(es, n, (const uint64_t *)ev, nev, i, b_pictures, progressive, q.slice0);
                else if (b_pictures) q.params = dec::bp_picture_params(es, n, (const uint64_t *)ev, nev, i, q.slice0);
                else q.params = dec::main_picture_params(es, n, (const uint64_t *)ev, nev, i, q.slice0);
                pics[p] = q; h_types[p] = (uint8_t)type;
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

// the nslices slices of the table's pictures, one per lane.  Only lowers its stream's err, which no lane of the launch reads.
// STORE false: for the verdict alone
template <bool STORE>
__global__ __launch_bounds__(64) void k_dsm_slices(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts,
                                                   const DsmPic *__restrict__ pics, const dec::MainChunkPic *__restrict__ tab, uint32_t ntab, uint32_t nslices,
                                                   dec::IMb *mb, int32_t *dc, int16_t *lv)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= nslices) return;
    const dec::MainChunkPic C = tab[dec::main_chunk_slice_pic(tab, ntab, g)];
    DsState *st = sts + C.stream;
    if (st->status != dec::kOk) return;
    const DsIn S = in[C.stream];
    const DsmPic Q = pics[C.gpic];
    const uint32_t row = g - C.slice0, nev = st->nev;
    const uint32_t i = Q.slice0 + row;
    if (i >= nev) return;                                              // (the plan accepted the picture: its slices are there)
    const ull *ev = evs + S.ev_base;
    const ull start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : S.n;
    const dec::IPicParams pp = dec::il_params_unpack(Q.params);
    bool ok;
    if (STORE) {
        const size_t first = (size_t)C.mb_base + (size_t)row * C.mbw;
        IMbSink sink{mb + first, dc + first * 6, lv + first * 384};
        ok = dec::il_slice(base + S.off, start, end, C.type, pp, (int)C.mbw, (int)C.mbh, (int)row, sink);
    } else {
        IMbNoSink sink;
        ok = dec::il_slice(base + S.off, start, end, C.type, pp, (int)C.mbw, (int)C.mbh, (int)row, sink);
    }
    if (!ok) atomicMin(&st->err, start);
}

// grid = (the most macroblocks of a picture of the launch, its pictures); list: their entries of the chunk's table.  Every read of a
// reference lies inside its picture: the slice walk refused the slice otherwise (dec::il_inside), and a refused slice makes its stream's
// status not OK before this kernel (k_ds_judge)
__global__ __launch_bounds__(64) void k_dsm_recon(const DsState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, const uint32_t *__restrict__ list,
                                                  const DsmPic *__restrict__ pics, const uint8_t *__restrict__ mats_all, const dec::IMb *__restrict__ mb,
                                                  const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf)
{
    __shared__ int32_t F[6][64];
    const dec::MainChunkPic C = tab[list[blockIdx.y]];
    const uint32_t mbw = C.mbw, mbh = C.mbh, k = blockIdx.x, l = threadIdx.x;
    if (k >= mbw * mbh) return;                                        // (a smaller picture of the launch; the whole workgroup leaves)
    if (sts[C.stream].status != dec::kOk) return;
    const uint32_t W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const size_t at = (size_t)C.mb_base + k;
    imb_recon(F, mb[at], dec::params_unpack(pics[C.gpic].params), mats_all + (size_t)C.stream * kDsmMatrices, dc, lv, at, buf + C.buf_off, buf + C.fwd_off,
              buf + C.bwd_off, W, H, CW, k % mbw, k / mbw, l);
}

// picture first + blockIdx.y of the chunk's table into dst: bytes [out_off, out_off + fb) of the output, iff its stream is OK.  A
// 16-byte unit of the destination that lies inside the frame is one aligned store; the units at the frame's edges go byte by byte, so
// two frames that share a unit never write each other's bytes
__global__ __launch_bounds__(kDsmThreads) void k_dsm_out(const DsState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, uint32_t first,
                                                         const uint8_t *__restrict__ buf, uint8_t *__restrict__ dst, int layout)
{
    const dec::MainChunkPic C = tab[first + blockIdx.y];
    if (sts[C.stream].status != dec::kOk) return;
    out_picture(buf + C.buf_off, C.w, C.h, 16u * C.mbw, 16u * C.mbh, C.out_off, C.out_off + C.fb, dst, layout, kDsmThreads);
}

void dsm_out(hipStream_t s, const DsState *d_st, const dec::MainChunkPic *tab, size_t count, uint32_t most_units, const uint8_t *buf, uint8_t *dst, int layout)
{
    const unsigned gx = (unsigned)std::min<size_t>(((size_t)most_units + kDsmThreads - 1) / kDsmThreads, 1024);
    for (size_t y = 0; y < count; y += 65535) {                       // (a grid's second dimension ends there)
        k_dsm_out<<<dim3(gx, (unsigned)std::min<size_t>(count - y, 65535)), kDsmThreads, 0, s>>>(d_st, tab, (uint32_t)y, buf, dst, layout);
        HIPCHK(hipGetLastError());
    }
}

int ds_main_first(m2v_enc *e, hipStream_t s, const char *entry, const uint8_t *es, const uint64_t *off, const uint64_t *bytes, size_t n, size_t pic_bytes,
                  bool slices, const DsPlanLaunch &plan, DsMainFirst &out)
{
    std::vector<size_t> ev_cap(n);
    for (size_t b = 0; b < n; ++b) ev_cap[b] = std::max<size_t>(256, bytes[b] / 16 + 64);      // a guess per stream: a second run takes the counts of the first
    out.rec.resize(n); out.mbh.resize(n); out.pic_base.resize(n);
    timer_break(e);
    for (int run = 0; run < 2; ++run) {
        size_t tiles = 0, evs = 0, pics = 0;
        const size_t in_bytes = ds_up64(n * sizeof(DsIn)), st_bytes = ds_up64(n * sizeof(DsState)), rec_bytes = ds_up64(n * sizeof(m2v_decode_stat)),
                     mbh_bytes = ds_up64(n * sizeof(uint32_t));
        for (size_t b = 0; b < n; ++b) pics += ev_cap[b] / 3 + 2;
        const size_t sl_bytes = slices ? ds_up64(pics * sizeof(uint32_t)) : 0;
        ensure_pinned(e->h_ds, e->h_ds_cap, in_bytes + st_bytes + rec_bytes + mbh_bytes + sl_bytes + pics + 64);
        auto *h_in = (DsIn *)e->h_ds;
        auto *h_st = (DsState *)(e->h_ds + in_bytes);
        auto *h_rec = (m2v_decode_stat *)(e->h_ds + in_bytes + st_bytes);
        auto *h_mbh = (uint32_t *)(e->h_ds + in_bytes + st_bytes + rec_bytes);
        auto *h_sl = slices ? (uint32_t *)(e->h_ds + in_bytes + st_bytes + rec_bytes + mbh_bytes) : nullptr;
        uint8_t *h_types = e->h_ds + in_bytes + st_bytes + rec_bytes + mbh_bytes + sl_bytes;
        pics = 0;
        for (size_t b = 0; b < n; ++b) {
            const size_t nb = bytes[b], nt = nb < 4 ? 0 : (nb + dec::kScanTile - 1) / dec::kScanTile;
            if (ev_cap[b] > 0x7FFFFFFFu) { e->set_err("%s: stream %zu holds more than 2^31 start codes", entry, b); return M2V_E_PARAM; }
            if (tiles + nt > 0x7FFFFFFFu) { e->set_err("%s: the streams are longer than 2^31 scan tiles", entry); return M2V_E_PARAM; }
            const size_t pic_cap = ev_cap[b] / 3 + 2;
            h_in[b] = DsIn{off[b], nb, evs, pics, (uint32_t)tiles, (uint32_t)nt, (uint32_t)ev_cap[b], (uint32_t)pic_cap};
            h_st[b] = DsState{dec::kNone, 0, 0, dec::kOk, 0, 0};
            out.pic_base[b] = pics;
            tiles += nt; evs += ev_cap[b]; pics += pic_cap;
        }
        if (pics > 0xFFFFFFFFull) { e->set_err("%s: more than 2^32 pictures", entry); return M2V_E_PARAM; }
        e->d_ds_in.ensure(in_bytes);
        e->d_dec_st.ensure(st_bytes);
        e->d_dec_tiles.ensure(std::max<size_t>(tiles, 1));
        e->d_dec_ev.ensure(evs);
        e->d_dec_pics.ensure(pics * pic_bytes);
        e->d_dec_main.ensure(n * kDsmMatrices);
        auto *d_in = (const DsIn *)e->d_ds_in.p;
        auto *d_st = (DsState *)e->d_dec_st.p;
        HIPCHK(hipMemcpyAsync(e->d_ds_in.p, h_in, in_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_st, h_st, st_bytes, hipMemcpyHostToDevice, s));
        ds_scan(s, es, d_in, n, tiles, d_st, e->d_dec_tiles.p, e->d_dec_ev.p);
        plan(d_in, d_st, h_types, h_sl, h_rec, h_mbh);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                              // the call's one wait for the plan: every stream's pictures, size, rows, types, slices
        bool again = false;
        for (size_t b = 0; b < n; ++b) {
            out.rec[b] = h_rec[b];
            out.mbh[b] = h_mbh[b];
            if (out.rec[b].status == dec::kEvents) { again = true; ev_cap[b] = out.rec[b].pictures; }      // (the count of events travels there)
        }
        out.types.assign(h_types, h_types + pics);
        if (slices) out.nsl.assign(h_sl, h_sl + pics);
        if (!again) break;
    }
    for (m2v_decode_stat &r : out.rec)                                // still too small behind the second run: refused
        if (r.status == dec::kEvents) { const uint64_t nb = r.es_bytes; r = m2v_decode_stat{}; r.es_bytes = nb; r.status = M2V_DEC_SYNTAX; }
    return M2V_OK;
}

}  // namespace m2v

struct DecodeStreamsMainArgs { const uint8_t *es; const uint64_t *off, *bytes; size_t n; uint8_t *dst; size_t cap; int layout; unsigned flags; hipStream_t s; };

static int decode_streams_main_impl(m2v_enc *e, void *argp)
{
    auto *a = (DecodeStreamsMainArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    const size_t n = a->n;
    e->ds_q.clear();
    // the work buffers are m2v_decode_device's and m2v_decode_streams_device's (all three calls block; no recorded graph references them)
    e->d_dec_st.recorded = e->d_dec_ev.recorded = e->d_dec_pics.recorded = e->d_dec_mb.recorded = e->d_dec_dc.recorded = false;
    e->d_dec_lv.recorded = e->d_dec_buf.recorded = e->d_dec_tiles.recorded = e->d_dec_list.recorded = e->d_dec_main.recorded = false;
    e->d_ds_in.recorded = e->d_ds_tab.recorded = false;
    DsMainFirst F;
    const int err = ds_main_first(e, s, "m2v_decode_streams_main_device", a->es, a->off, a->bytes, n, sizeof(DsmPic), false,
                                  [&](const DsIn *d_in, DsState *d_st, uint8_t *h_types, uint32_t *, m2v_decode_stat *h_rec, uint32_t *h_mbh) {
        k_dsm_plan<<<(unsigned)n, kDsmThreads, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, (DsmPic *)e->d_dec_pics.p, h_types, h_rec, h_mbh, e->d_dec_main.p, a->flags);
    }, F);
    if (err != M2V_OK) return err;
    const std::vector<m2v_decode_stat> &rec = F.rec;
    const std::vector<size_t> &pic_base = F.pic_base;
    std::vector<dec::MainStreamInfo> info(n);
    for (size_t b = 0; b < n; ++b) info[b] = dec::MainStreamInfo{rec[b].status, rec[b].pictures, rec[b].width, rec[b].height, F.mbh[b], F.types.data() + pic_base[b]};
    dec::MainStreamsPlan P = dec::plan_streams_main(info.data(), n, a->cap, a->dst == nullptr, e->decode_batch, (a->flags & M2V_DECS_B_PICTURES) != 0);
    for (dec::MainChunkPic &c : P.pics) c.gpic = (uint32_t)(pic_base[c.stream] + c.pic);
    for (dec::MainChunkPic &c : P.pre) c.gpic = (uint32_t)(pic_base[c.stream] + c.pic);
    if (!a->dst || P.pics.empty()) { ds_report(e, a->off, n, P.out_offset, P.overflow, rec, nullptr); return M2V_OK; }
    const size_t tab_bytes = ds_up64(P.pics.size() * sizeof(dec::MainChunkPic)), pre_bytes = ds_up64(P.pre.size() * sizeof(dec::MainChunkPic)),
                 list_bytes = ds_up64(P.list.size() * sizeof(uint32_t));
    ensure_pinned(e->h_ds_tab, e->h_ds_tab_cap, tab_bytes + pre_bytes + list_bytes + n * sizeof(DsVerdict) + 64);
    memcpy(e->h_ds_tab, P.pics.data(), P.pics.size() * sizeof(dec::MainChunkPic));
    if (!P.pre.empty()) memcpy(e->h_ds_tab + tab_bytes, P.pre.data(), P.pre.size() * sizeof(dec::MainChunkPic));
    memcpy(e->h_ds_tab + tab_bytes + pre_bytes, P.list.data(), P.list.size() * sizeof(uint32_t));
    auto *h_v = (DsVerdict *)(e->h_ds_tab + tab_bytes + pre_bytes + list_bytes);
    e->d_ds_tab.ensure(tab_bytes + pre_bytes + list_bytes);
    HIPCHK(hipMemcpyAsync(e->d_ds_tab.p, e->h_ds_tab, tab_bytes + pre_bytes + list_bytes, hipMemcpyHostToDevice, s));
    uint64_t most_mbs = 0, most_buf = 0;
    for (const dec::MainStreamsChunk &C : P.chunks) { most_mbs = std::max(most_mbs, C.mbs); most_buf = std::max(most_buf, C.buf_bytes); }
    e->d_dec_mb.ensure(most_mbs * sizeof(dec::IMb));
    e->d_dec_dc.ensure(most_mbs * 6);
    e->d_dec_lv.ensure(most_mbs * 384);
    e->d_dec_buf.ensure(most_buf);
    auto *d_in = (const DsIn *)e->d_ds_in.p;
    auto *d_st = (DsState *)e->d_dec_st.p;
    auto *d_mb = (dec::IMb *)e->d_dec_mb.p;
    auto *d_pics = (const DsmPic *)e->d_dec_pics.p;
    auto *d_tab = (const dec::MainChunkPic *)e->d_ds_tab.p;
    auto *d_pre = (const dec::MainChunkPic *)(e->d_ds_tab.p + tab_bytes);
    auto *d_list = (const uint32_t *)(e->d_ds_tab.p + tab_bytes + pre_bytes);
    const uint8_t *d_mats = e->d_dec_main.p;
    if (P.pre_slices) {
        k_dsm_slices<false><<<(P.pre_slices + 63u) / 64u, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, d_pre, (uint32_t)P.pre.size(), P.pre_slices, nullptr,
                                                                    nullptr, nullptr);
        HIPCHK(hipGetLastError());
        ds_judge(s, d_st, n);
    }
    for (const dec::MainStreamsChunk &C : P.chunks) {
        const dec::MainChunkPic *tab = d_tab + C.first;
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, C.mbs * 768, s));
        k_dsm_slices<true><<<(C.slices + 63u) / 64u, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, (uint32_t)C.count, C.slices, d_mb, e->d_dec_dc.p,
                                                               e->d_dec_lv.p);
        HIPCHK(hipGetLastError());
        ds_judge(s, d_st, n);
        auto recon = [&](const dec::MainStreamsChunk::Step &S) {
            for (size_t y = 0; y < S.count; y += 65535) {             // (a grid's second dimension ends there)
                k_dsm_recon<<<dim3(S.most_mbs, (unsigned)std::min<size_t>(S.count - y, 65535)), 64, 0, s>>>(d_st, tab, d_list + S.off + y, d_pics, d_mats, d_mb,
                                                                                                          e->d_dec_dc.p, e->d_dec_lv.p, e->d_dec_buf.p);
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

int m2v_decode_streams_main_device(m2v_enc *e, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams, void *d_dst, size_t cap,
                                   int layout, unsigned flags, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    if (nstreams < 1 || nstreams > 65535) { e->set_err("m2v_decode_streams_main_device: nstreams is 1 .. 65535, not %zu", nstreams); return M2V_E_PARAM; }
    if (!es_off || !es_bytes) { e->set_err("m2v_decode_streams_main_device: es_off / es_bytes is NULL"); return M2V_E_PARAM; }
    if (!layout420_ok(layout)) { e->set_err("m2v_decode_streams_main_device: unknown layout %d", layout); return M2V_E_PARAM; }
    if (flags & ~(unsigned)(M2V_DECS_B_PICTURES | M2V_DECS_INTERLACED)) {
        e->set_err("m2v_decode_streams_main_device: flags are M2V_DECS_B_PICTURES | M2V_DECS_INTERLACED, not 0x%x", flags);
        return M2V_E_PARAM;
    }
    if (!d_es) for (size_t b = 0; b < nstreams; ++b) if (es_bytes[b]) { e->set_err("m2v_decode_streams_main_device: d_es is NULL"); return M2V_E_PARAM; }
    if (in_progress(e, "m2v_decode_streams_main_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    DecodeStreamsMainArgs a{(const uint8_t *)d_es, es_off, es_bytes, nstreams, (uint8_t *)d_dst, cap, layout, flags, (hipStream_t)hip_stream};
    return guard(e, decode_streams_main_impl, &a);
}

}  // extern "C"
