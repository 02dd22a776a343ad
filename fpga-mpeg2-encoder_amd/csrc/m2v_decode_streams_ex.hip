// m2v_decode_streams_ex.hip — a batch of main-syntax streams with the extended options in one call (include/m2v_mi355x.h:
// m2v_decode_streams_main_ex_device): the pipeline of m2v_decode_streams_main.hip over the x_ / t_ functions of m2v_decode_kernels.hpp,
// each stream judged alone as m2v_decode_device judges it with "decode_syntax" = main and the four options set as the call's flags say.
// With flags below M2V_DECS_EXTENDED the entry hands the call to m2v_decode_streams_main_device as it stands.  No other unit changes its
// text, so every other kernel comes out of the compiler as it did.
//
//   k_dsx_scan    copies of k_dsm_scan / k_dsm_tiles (a kernel is launched from the unit that holds it; the syntax does not matter to
//   k_dsx_tiles   them).
//   k_dsx_plan    one block per stream: k_dt_plan's grammar with the stream's own segment, events, picture table and record.  flag 8:
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
//   k_dsx_out / k_dsx_judge / k_dsx_finish   as k_dsm_*.
#include "m2v_host.hpp"
#include "m2v_decode_kernels.hpp"
#include "m2v_decode_streams.hpp"
#include "m2v_decode_streams_ex.hpp"

static_assert(sizeof(dec::MainChunkPic) == 88, "a chunk's picture is 88 bytes");
static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

constexpr int kDsxThreads = 256;
static_assert(dec::kScanTile == (uint32_t)kDsxThreads * 16u, "a tile is one pass of a block");
typedef unsigned long long ull;

struct DsxIn { ull off, n, ev_base, pic_base; uint32_t tile0, ntiles, ev_cap, pic_cap; };
struct DsxState { ull err, last_nz; uint32_t nev; int32_t status; uint32_t mbw, mbh; };
// a picture: the event of its first slice, dec::t_params_pack, its slice events, the events that loaded its matrices (kNoEvent: the sequence's)
struct DsxPic { uint32_t slice0, params, nslices, mi, mn; };
struct DsxVerdict { ull err; int32_t status; uint32_t pad; };
constexpr uint32_t kDsxMatrices = 128;

__device__ inline uint32_t dsx_stream_of(const DsxIn *__restrict__ in, uint32_t n, uint32_t t)
{
    uint32_t a = 0, b = n;
    while (b - a > 1u) { const uint32_t m = (a + b) / 2u; if (in[m].tile0 <= t) a = m; else b = m; }
    return a;
}

template <bool EMIT>
__global__ __launch_bounds__(kDsxThreads) void k_dsx_scan(const uint8_t *__restrict__ base, const DsxIn *__restrict__ in, uint32_t nstreams, uint32_t ntiles,
                                                          DsxState *st, uint32_t *__restrict__ tiles, ull *__restrict__ evs)
{
    __shared__ uint32_t s_w[kDsxThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t b = dsx_stream_of(in, nstreams, t);
        const DsxIn S = in[b];
        const uint8_t *es = base + S.off;
        const ull n = S.n, p0 = (ull)(t - S.tile0) * dec::kScanTile + (ull)tid * 16u;
        uint64_t w0 = 0, w1 = 0, w2 = 0, nz = 0;
        uint32_t cand = 0;
        if (p0 < n) {
            mux::load24(es, p0, n, w0, w1, w2);              // (clamped to the segment: what lies behind it reads as FF)
            cand = dec::scan16(p0, n, w0, w1, w2, nz);
        }
        const uint32_t c = (uint32_t)__popc(cand);
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += v;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kDsxThreads / 64; ++k) { if (k < wave) before += s_w[k]; total += s_w[k]; }
        if (!EMIT) {
            if (tid == 0) tiles[t] = total;
#pragma unroll
            for (int d = 32; d; d >>= 1) nz = mux::max64(nz, __shfl_xor(nz, d));
            if (lane == 0 && nz) atomicMax(&st[b].last_nz, (ull)nz);
        } else {
            ull *ev = evs + S.ev_base;
            uint32_t at = tiles[t] + before + incl - c;
            while (cand) {
                const uint32_t j = (uint32_t)__builtin_ctz(cand);
                cand &= cand - 1u;
                if (at < S.ev_cap) ev[at] = (p0 + j) << 8 | mux::byte24(w0, w1, w2, j + 3);
                ++at;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kDsxThreads) void k_dsx_tiles(const DsxIn *__restrict__ in, uint32_t *tiles_all, DsxState *sts)
{
    __shared__ uint32_t s_sum[kDsxThreads];
    const DsxIn S = in[blockIdx.x];
    DsxState *st = sts + blockIdx.x;
    uint32_t *tiles = tiles_all + S.tile0;
    const uint32_t ntiles = S.ntiles, tid = threadIdx.x, per = (ntiles + kDsxThreads - 1) / kDsxThreads;
    const uint32_t a = min(ntiles, tid * per), b = min(ntiles, a + per);
    uint32_t sum = 0;
    for (uint32_t t = a; t < b; ++t) sum += tiles[t];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kDsxThreads; ++k) { const uint32_t v = s_sum[k]; s_sum[k] = run; run += v; }
        st->nev = run;
        if (run > S.ev_cap) st->status = dec::kEvents;
    }
    __syncthreads();
    uint32_t run = s_sum[tid];
    for (uint32_t t = a; t < b; ++t) { const uint32_t v = tiles[t]; tiles[t] = run; run += v; }
}

// one block per stream.  Whether the frames fit is the host's to say, behind the wait (the rooms depend on the streams in front)
__global__ __launch_bounds__(kDsxThreads) void k_dsx_plan(const uint8_t *__restrict__ base, const DsxIn *__restrict__ in, const ull *__restrict__ evs, DsxState *sts,
                                                          DsxPic *__restrict__ pics_all, uint8_t *h_types_all, uint32_t *h_sl_all, m2v_decode_stat *h_recs, uint32_t *h_mbh,
                                                          uint8_t *__restrict__ mats_all, unsigned flags)
{
    __shared__ dec::MainPlan s_P;
    __shared__ ull s_bad;
    __shared__ uint32_t s_np[kDsxThreads], s_ng[kDsxThreads], s_nr[kDsxThreads], s_ni[kDsxThreads], s_na[kDsxThreads];
    __shared__ int s_last[kDsxThreads], s_sig[kDsxThreads];
    __shared__ uint32_t s_mi[kDsxThreads], s_mn[kDsxThreads], s_rs[kDsxThreads];      // the events that loaded the matrices; a reset
    const DsxIn S = in[blockIdx.x];
    DsxState *st = sts + blockIdx.x;
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
__global__ __launch_bounds__(128) void k_dsx_mats(const uint8_t *__restrict__ base, const DsxIn *__restrict__ in, const ull *__restrict__ evs,
                                                  const DsxState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, uint32_t ntab,
                                                  const DsxPic *__restrict__ pics, const uint8_t *__restrict__ mats_all, uint8_t *__restrict__ table)
{
    const uint32_t l = threadIdx.x, m = l >> 6, t = l & 63u;
    for (uint32_t p = blockIdx.x; p < ntab; p += gridDim.x) {
        const dec::MainChunkPic C = tab[p];
        const DsxState *st = sts + C.stream;
        if (st->status != dec::kOk) continue;
        const DsxIn S = in[C.stream];
        const DsxPic Q = pics[C.gpic];
        table[(size_t)p * 128u + l] = (uint8_t)dec::x_matrix_weight(base + S.off, S.n, (const uint64_t *)(evs + S.ev_base), st->nev, m ? Q.mn : Q.mi, (int)m, t,
                                                                     mats_all + (size_t)C.stream * kDsxMatrices + 64u * m);
    }
}

struct DsxSink {
    dec::IMb *mb_;
    int32_t *dc_;
    int16_t *lv_;
    M2V_HD void mb(int col, const dec::IMb &m, const int32_t (&dc)[6])
    {
        mb_[col] = m;
#pragma unroll
        for (int k = 0; k < 6; ++k) dc_[col * 6 + k] = dc[k];
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { lv_[(col * 6 + blk) * 64 + (int)i] = (int16_t)l; }
};
struct DsxNoSink {
    M2V_HD void mb(int, const dec::IMb &, const int32_t (&)[6]) {}
    M2V_HD void level(int, int, uint32_t, int32_t) {}
};

// the nslices slice events of the table's pictures, one per lane, each into the row its code names.  The lane leaves its span (0: not
// walked); a slice that cannot be read lowers its stream's err, which no lane of the launch reads.  Two slices that overlap write the
// same records - the judge refuses the stream before anything reads them.  STORE false: for the verdict alone
template <bool STORE, bool TOOLS>
__global__ __launch_bounds__(64) void k_dsx_slices(const uint8_t *__restrict__ base, const DsxIn *__restrict__ in, const ull *__restrict__ evs, DsxState *sts,
                                                   const DsxPic *__restrict__ pics, const dec::MainChunkPic *__restrict__ tab, uint32_t ntab, uint32_t nslices,
                                                   dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *__restrict__ spans)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= nslices) return;
    spans[g] = 0u;
    const dec::MainChunkPic C = tab[dec::main_chunk_slice_pic(tab, ntab, g)];
    DsxState *st = sts + C.stream;
    if (st->status != dec::kOk) return;
    const DsxIn S = in[C.stream];
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
        DsxSink sink{mb + first, dc + first * 6, lv + first * 384};
        ok = TOOLS ? dec::t_slice(es, start, end, C.type, dec::t_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1)
                   : dec::x_slice(es, start, end, C.type, dec::il_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1);
    } else {
        DsxNoSink sink;
        ok = TOOLS ? dec::t_slice(es, start, end, C.type, dec::t_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1)
                   : dec::x_slice(es, start, end, C.type, dec::il_params_unpack(Q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1);
    }
    spans[g] = dec::x_span_pack(ok, code, c0, c1);
    if (!ok) atomicMin(&st->err, start);
}

// continuity behind the walk: every readable slice against the span of the slice in front of it in its picture
__global__ __launch_bounds__(64) void k_dsx_cont(const DsxIn *__restrict__ in, const ull *__restrict__ evs, DsxState *sts, const DsxPic *__restrict__ pics,
                                                 const dec::MainChunkPic *__restrict__ tab, uint32_t ntab, uint32_t nslices, const uint32_t *__restrict__ spans)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= nslices) return;
    const dec::MainChunkPic C = tab[dec::main_chunk_slice_pic(tab, ntab, g)];
    DsxState *st = sts + C.stream;
    if (st->status != dec::kOk) return;
    const DsxPic Q = pics[C.gpic];
    const uint32_t k = g - C.slice0, cur = spans[g];
    if (!(cur >> 31) || k >= Q.nslices || Q.slice0 + k >= st->nev) return;      // (not readable: reported by its walk)
    if (!dec::x_continuous(cur, k ? spans[g - 1] : 0u, k, Q.nslices, C.mbw)) atomicMin(&st->err, dec::ev_pos(evs[in[C.stream].ev_base + Q.slice0 + k]));
}

__global__ void k_dsx_judge(DsxState *sts, uint32_t n)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n && sts[b].status == dec::kOk && sts[b].err != dec::kNone) sts[b].status = dec::kSyntax;
}

// grid = (the most macroblocks of a picture of the launch, its pictures); list: their entries of the chunk's table; table: the chunk's
// rows of the matrix table.  Every read of a reference lies inside its picture: the slice walk refused the slice otherwise
// (dec::il_inside), and a refused slice makes its stream's status not OK before this kernel (k_dsx_judge)
__global__ __launch_bounds__(64) void k_dsx_recon(const DsxState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, const uint32_t *__restrict__ list,
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
    const dec::PicParams pp = dec::params_unpack(pics[C.gpic].params);
    const uint8_t *mats = table + (size_t)entry * 128u;
    const size_t at = (size_t)C.mb_base + k;
    const dec::IMb m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw;
    uint8_t *cur = buf + C.buf_off;
    const uint8_t *fwd = buf + C.fwd_off, *bwd = buf + C.bwd_off;
    const bool intra = m.intra != 0;
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
    {   // luma: four samples of one row per lane; the row's block and the row inside it through the field-DCT map
        const uint32_t y = l >> 2, x0 = (l & 3u) * 4u, blk = dec::il_luma_block(x0, y, m.dct_type), brow = dec::il_luma_row(y, m.dct_type);
        const bool coded = (m.cbp >> (5 - blk)) & 1;
        const int px = (int)(16u * col + x0), py = (int)(16u * row + y);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t pred = intra ? 128 : dec::il_predict(fwd, bwd, (int)W, px + j, py, m, false);
            const int32_t res = coded ? F[blk][brow * 8u + ((x0 + j) & 7u)] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint32_t *)(cur + (size_t)(16u * row + y) * W + 16u * col + x0) = v;
    }
    {   // chroma: two samples per lane, U in the first half of the wavefront; frame blocks always
        const uint32_t pl = l >> 5, y = (l >> 2) & 7u, x0 = (l & 3u) * 2u;
        const bool coded = (m.cbp >> (1 - pl)) & 1;
        const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2u);
        const int px = (int)(8u * col + x0), py = (int)(8u * row + y);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t pred = intra ? 128 : dec::il_predict(fwd + plane, bwd + plane, (int)CW, px + j, py, m, true);
            const int32_t res = coded ? F[4u + pl][y * 8u + x0 + j] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint16_t *)(cur + plane + (size_t)(8u * row + y) * CW + 8u * col + x0) = (uint16_t)v;
    }
}

typedef uint32_t dsx_store_t __attribute__((ext_vector_type(4)));

// picture first + blockIdx.y of the chunk's table into dst: bytes [out_off, out_off + fb) of the output, iff its stream is OK.  A
// 16-byte unit of the destination that lies inside the frame is one aligned store; the units at the frame's edges go byte by byte, so
// two frames that share a unit never write each other's bytes
__global__ __launch_bounds__(kDsxThreads) void k_dsx_out(const DsxState *__restrict__ sts, const dec::MainChunkPic *__restrict__ tab, uint32_t first,
                                                         const uint8_t *__restrict__ buf, uint8_t *__restrict__ dst, int layout)
{
    const dec::MainChunkPic C = tab[first + blockIdx.y];
    if (sts[C.stream].status != dec::kOk) return;
    const uint32_t w = C.w, h = C.h, W = 16u * C.mbw, H = 16u * C.mbh;
    const uint8_t *pic = buf + C.buf_off;
    const ull lo = C.out_off, hi = lo + C.fb;
    const ull lead = (ull)(uintptr_t)dst & 15ull;
    const ull u0 = (lo + lead) >> 4, u1 = (hi + lead + 15ull) >> 4;
    for (ull g = u0 + (ull)blockIdx.x * kDsxThreads + threadIdx.x; g < u1; g += (ull)gridDim.x * kDsxThreads) {
        const long long o0 = (long long)(g << 4) - (long long)lead;
        const int k0 = o0 < (long long)lo ? (int)((long long)lo - o0) : 0, k1 = (long long)hi - o0 < 16 ? (int)((long long)hi - o0) : 16;
        if (k0 >= k1) continue;
        uint32_t q = (uint32_t)((ull)(o0 + k0) - lo);
        dec::OutAt at = dec::out_locate(q, w, h, layout);
        uint32_t v[4] = {0, 0, 0, 0};
        for (int k = k0; k < k1; ++k) {
            v[k >> 2] |= (uint32_t)dec::pic_sample(pic, W, H, at) << (8 * (k & 3));
            if (k + 1 == k1) break;
            ++q;
            if (at.run > 1) dec::out_step(at, layout);
            else at = dec::out_locate(q, w, h, layout);
        }
        if (k0 == 0 && k1 == 16) {
            *(__attribute__((address_space(1))) dsx_store_t *)(dst + o0) = dsx_store_t{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = k0; k < k1; ++k) dst[o0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

__global__ void k_dsx_finish(const DsxState *sts, uint32_t n, DsxVerdict *h_v)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) h_v[b] = DsxVerdict{sts[b].err, sts[b].status, 0};
}

}  // namespace m2v

struct DecodeStreamsExArgs { const uint8_t *es; const uint64_t *off, *bytes; size_t n; uint8_t *dst; size_t cap; int layout; unsigned flags; hipStream_t s; };

static size_t dsx_up64(size_t v) { return (v + 63) & ~(size_t)63; }

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
    std::vector<size_t> ev_cap(n);
    for (size_t b = 0; b < n; ++b) ev_cap[b] = std::max<size_t>(256, a->bytes[b] / 16 + 64);      // a guess per stream: a second run takes the counts of the first
    std::vector<m2v_decode_stat> rec(n);
    std::vector<uint8_t> types;
    std::vector<uint32_t> mbh(n), nsl;
    std::vector<size_t> pic_base(n);
    timer_break(e);
    for (int run = 0; run < 2; ++run) {
        size_t tiles = 0, evs = 0, pics = 0;
        const size_t in_bytes = dsx_up64(n * sizeof(DsxIn)), st_bytes = dsx_up64(n * sizeof(DsxState)), rec_bytes = dsx_up64(n * sizeof(m2v_decode_stat)),
                     mbh_bytes = dsx_up64(n * sizeof(uint32_t));
        for (size_t b = 0; b < n; ++b) pics += ev_cap[b] / 3 + 2;
        const size_t sl_bytes = dsx_up64(pics * sizeof(uint32_t));
        ensure_pinned(e->h_ds, e->h_ds_cap, in_bytes + st_bytes + rec_bytes + mbh_bytes + sl_bytes + pics + 64);
        auto *h_in = (DsxIn *)e->h_ds;
        auto *h_st = (DsxState *)(e->h_ds + in_bytes);
        auto *h_rec = (m2v_decode_stat *)(e->h_ds + in_bytes + st_bytes);
        auto *h_mbh = (uint32_t *)(e->h_ds + in_bytes + st_bytes + rec_bytes);
        auto *h_sl = (uint32_t *)(e->h_ds + in_bytes + st_bytes + rec_bytes + mbh_bytes);
        uint8_t *h_types = e->h_ds + in_bytes + st_bytes + rec_bytes + mbh_bytes + sl_bytes;
        pics = 0;
        for (size_t b = 0; b < n; ++b) {
            const size_t nb = a->bytes[b], nt = nb < 4 ? 0 : (nb + dec::kScanTile - 1) / dec::kScanTile;
            if (ev_cap[b] > 0x7FFFFFFFu) { e->set_err("m2v_decode_streams_main_ex_device: stream %zu holds more than 2^31 start codes", b); return M2V_E_PARAM; }
            if (tiles + nt > 0x7FFFFFFFu) { e->set_err("m2v_decode_streams_main_ex_device: the streams are longer than 2^31 scan tiles"); return M2V_E_PARAM; }
            const size_t pic_cap = ev_cap[b] / 3 + 2;
            h_in[b] = DsxIn{a->off[b], nb, evs, pics, (uint32_t)tiles, (uint32_t)nt, (uint32_t)ev_cap[b], (uint32_t)pic_cap};
            h_st[b] = DsxState{dec::kNone, 0, 0, dec::kOk, 0, 0};
            pic_base[b] = pics;
            tiles += nt; evs += ev_cap[b]; pics += pic_cap;
        }
        if (pics > 0xFFFFFFFFull) { e->set_err("m2v_decode_streams_main_ex_device: more than 2^32 pictures"); return M2V_E_PARAM; }
        e->d_ds_in.ensure(in_bytes);
        e->d_dec_st.ensure(st_bytes);
        e->d_dec_tiles.ensure(std::max<size_t>(tiles, 1));
        e->d_dec_ev.ensure(evs);
        e->d_dec_pics.ensure(pics * sizeof(DsxPic));
        e->d_dec_main.ensure(n * kDsxMatrices);
        auto *d_in = (const DsxIn *)e->d_ds_in.p;
        auto *d_st = (DsxState *)e->d_dec_st.p;
        HIPCHK(hipMemcpyAsync(e->d_ds_in.p, h_in, in_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_st, h_st, st_bytes, hipMemcpyHostToDevice, s));
        if (tiles) {
            const unsigned gx = (unsigned)std::min<size_t>(tiles, 4096);
            k_dsx_scan<false><<<gx, kDsxThreads, 0, s>>>(a->es, d_in, (uint32_t)n, (uint32_t)tiles, d_st, e->d_dec_tiles.p, e->d_dec_ev.p);
            HIPCHK(hipGetLastError());
            k_dsx_tiles<<<(unsigned)n, kDsxThreads, 0, s>>>(d_in, e->d_dec_tiles.p, d_st);
            HIPCHK(hipGetLastError());
            k_dsx_scan<true><<<gx, kDsxThreads, 0, s>>>(a->es, d_in, (uint32_t)n, (uint32_t)tiles, d_st, e->d_dec_tiles.p, e->d_dec_ev.p);
            HIPCHK(hipGetLastError());
        }
        k_dsx_plan<<<(unsigned)n, kDsxThreads, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, (DsxPic *)e->d_dec_pics.p, h_types, h_sl, h_rec, h_mbh, e->d_dec_main.p, a->flags);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                              // the call's one wait for the plan: every stream's pictures, size, rows, types, slices
        bool again = false;
        for (size_t b = 0; b < n; ++b) {
            rec[b] = h_rec[b];
            mbh[b] = h_mbh[b];
            if (rec[b].status == dec::kEvents) { again = true; ev_cap[b] = rec[b].pictures; }      // (the count of events travels there)
        }
        types.assign(h_types, h_types + pics);
        nsl.assign(h_sl, h_sl + pics);
        if (!again) break;
    }
    std::vector<dec::ExStreamInfo> info(n);
    for (size_t b = 0; b < n; ++b) {
        if (rec[b].status == dec::kEvents) { const uint64_t nb = rec[b].es_bytes; rec[b] = m2v_decode_stat{}; rec[b].es_bytes = nb; rec[b].status = M2V_DEC_SYNTAX; }
        info[b] = dec::ExStreamInfo{dec::MainStreamInfo{rec[b].status, rec[b].pictures, rec[b].width, rec[b].height, mbh[b], types.data() + pic_base[b]},
                                    nsl.data() + pic_base[b]};
    }
    dec::MainStreamsPlan P = dec::plan_streams_main_ex(info.data(), n, a->cap, a->dst == nullptr, e->decode_batch, (a->flags & M2V_DECS_B_PICTURES) != 0, tools);
    for (dec::MainChunkPic &c : P.pics) c.gpic = (uint32_t)(pic_base[c.stream] + c.pic);
    for (dec::MainChunkPic &c : P.pre) c.gpic = (uint32_t)(pic_base[c.stream] + c.pic);
    auto report = [&](const DsxVerdict *v) {
        for (size_t b = 0; b < n; ++b) {
            m2v_decode_stream_stat r{a->off[b], P.out_offset[b], rec[b]};
            if (r.rec.status == M2V_DEC_OK) {
                if (P.overflow[b]) r.rec.status = M2V_DEC_OVERFLOW;
                else if (v && v[b].status != dec::kOk) { r.rec.status = v[b].status; r.rec.err_offset = v[b].err; }
                else r.rec.out_bytes = r.rec.frame_bytes * r.rec.pictures;
            }
            e->ds_q.push(&r, &r + 1);
        }
    };
    if (!a->dst || P.pics.empty()) { report(nullptr); return M2V_OK; }
    if (P.pics.size() > 0xFFFFFFFFull) { e->set_err("m2v_decode_streams_main_ex_device: more than 2^32 pictures"); return M2V_E_PARAM; }
    const size_t tab_bytes = dsx_up64(P.pics.size() * sizeof(dec::MainChunkPic)), pre_bytes = dsx_up64(P.pre.size() * sizeof(dec::MainChunkPic)),
                 list_bytes = dsx_up64(P.list.size() * sizeof(uint32_t));
    ensure_pinned(e->h_ds_tab, e->h_ds_tab_cap, tab_bytes + pre_bytes + list_bytes + n * sizeof(DsxVerdict) + 64);
    memcpy(e->h_ds_tab, P.pics.data(), P.pics.size() * sizeof(dec::MainChunkPic));
    if (!P.pre.empty()) memcpy(e->h_ds_tab + tab_bytes, P.pre.data(), P.pre.size() * sizeof(dec::MainChunkPic));
    memcpy(e->h_ds_tab + tab_bytes + pre_bytes, P.list.data(), P.list.size() * sizeof(uint32_t));
    auto *h_v = (DsxVerdict *)(e->h_ds_tab + tab_bytes + pre_bytes + list_bytes);
    e->d_ds_tab.ensure(tab_bytes + pre_bytes + list_bytes);
    HIPCHK(hipMemcpyAsync(e->d_ds_tab.p, e->h_ds_tab, tab_bytes + pre_bytes + list_bytes, hipMemcpyHostToDevice, s));
    uint64_t most_mbs = 0, most_buf = 0, most_slices = P.pre_slices;
    for (const dec::MainStreamsChunk &C : P.chunks) {
        most_mbs = std::max(most_mbs, C.mbs); most_buf = std::max(most_buf, C.buf_bytes); most_slices = std::max<uint64_t>(most_slices, C.slices);
    }
    const size_t span_off = dsx_up64(P.pics.size() * 128);             // the matrix table, then the spans of a launch's slices
    e->d_dec_x.ensure(span_off + std::max<size_t>(most_slices, 1) * sizeof(uint32_t));
    e->d_dec_mb.ensure(most_mbs * sizeof(dec::IMb));
    e->d_dec_dc.ensure(most_mbs * 6);
    e->d_dec_lv.ensure(most_mbs * 384);
    e->d_dec_buf.ensure(most_buf);
    auto *d_in = (const DsxIn *)e->d_ds_in.p;
    auto *d_st = (DsxState *)e->d_dec_st.p;
    auto *d_mb = (dec::IMb *)e->d_dec_mb.p;
    auto *d_pics = (const DsxPic *)e->d_dec_pics.p;
    auto *d_tab = (const dec::MainChunkPic *)e->d_ds_tab.p;
    auto *d_pre = (const dec::MainChunkPic *)(e->d_ds_tab.p + tab_bytes);
    auto *d_list = (const uint32_t *)(e->d_ds_tab.p + tab_bytes + pre_bytes);
    uint8_t *d_table = e->d_dec_x.p;
    auto *d_spans = (uint32_t *)(e->d_dec_x.p + span_off);
    const unsigned gj = (unsigned)((n + 63) / 64);
    auto walk = [&](bool store, const dec::MainChunkPic *tab, uint32_t ntab, uint32_t nslices) {
        const unsigned g = (nslices + 63u) / 64u;
        if (store && tools) k_dsx_slices<true, true><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, d_mb, e->d_dec_dc.p, e->d_dec_lv.p, d_spans);
        else if (store) k_dsx_slices<true, false><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, d_mb, e->d_dec_dc.p, e->d_dec_lv.p, d_spans);
        else if (tools) k_dsx_slices<false, true><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, nullptr, nullptr, nullptr, d_spans);
        else k_dsx_slices<false, false><<<g, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, nullptr, nullptr, nullptr, d_spans);
        HIPCHK(hipGetLastError());
        k_dsx_cont<<<g, 64, 0, s>>>(d_in, e->d_dec_ev.p, d_st, d_pics, tab, ntab, nslices, d_spans);
        HIPCHK(hipGetLastError());
        k_dsx_judge<<<gj, 64, 0, s>>>(d_st, (uint32_t)n);
        HIPCHK(hipGetLastError());
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
        const unsigned gx = (unsigned)std::min<size_t>(((size_t)C.most_units + kDsxThreads - 1) / kDsxThreads, 1024);
        for (size_t y = 0; y < C.count; y += 65535) {
            k_dsx_out<<<dim3(gx, (unsigned)std::min<size_t>(C.count - y, 65535)), kDsxThreads, 0, s>>>(d_st, tab, (uint32_t)y, e->d_dec_buf.p, a->dst, a->layout);
            HIPCHK(hipGetLastError());
        }
        // the next chunk's carried anchors: slot 0 first (it may come from slot 1)
        if (C.carry0_from >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + C.carry0_from, C.carry_bytes, hipMemcpyDeviceToDevice, s));
        if (C.carry1_from >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p + P.carry, e->d_dec_buf.p + C.carry1_from, C.carry_bytes, hipMemcpyDeviceToDevice, s));
    }
    k_dsx_finish<<<gj, 64, 0, s>>>(d_st, (uint32_t)n, h_v);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    report(h_v);
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
