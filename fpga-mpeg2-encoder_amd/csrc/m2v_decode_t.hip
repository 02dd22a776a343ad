// m2v_decode_t.hip — Table B-15, concealment motion vectors and dual prime for m2v_decode_device (option "decode_mb_tools" = 1 on top of
// "decode_extended" = 1, with "decode_b_pictures" and "decode_interlaced" 0 or 1 each).  Modelled on m2v_decode_x.hip, whose plan, tables
// and launches these are: m2v_decode.hip keeps the scan; this unit holds the plan and everything behind the plan's wait, in kernels of
// its own so that those of the other five units come out of the compiler exactly as they did.
// decoder.decode_main(extended=True, mb_tools=True) is the definition; every function that decides a bit, a column or a verdict is a t_
// (or x_ / il_ / bp_ / main_) function of m2v_decode_kernels.hpp.
//
//   k_dt_plan    k_dx_plan with dec::t_event and dec::t_picture_params: the coding extension's intra_vlc_format,
//                concealment_motion_vectors and top_field_first are kept in bits 21 .. 23 of the packed parameters, and a P picture's
//                "backward" picture is its forward reference - a dual-prime macroblock's record is a field-based one with both
//                directions, and the reconstruction reads it as such.
//   k_dt_slices  one lane per slice EVENT of the chunk, as k_dx_slices, walking with dec::t_slice: one macroblock function for every
//                picture kind, Table B-15 by dec::vlc_ac15 - two dependent table loads a code, as dec::vlc_ac.
//   k_dt_mats, k_dt_cont, k_dt_judge, k_dt_recon, k_dt_out, k_dt_finish   k_dx_*'s text (a kernel is launched from the unit that holds it).
//
// The chunk's buffer, the steps of the anchors and the single launch for a chunk's B pictures are m2v_decode_b.hip's.  Records and
// levels stay indexed by macroblock address: nothing behind the walk knows how a row was cut.
#include "m2v_decode_state.hpp"

static_assert(sizeof(dec::IMb) == 32, "the interlaced record is two of the module's");

namespace m2v {

constexpr uint32_t kNoPic = 0xFFFFFFFFu;

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

struct DecTSink {
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

// pictures [p0, p0 + np) of any type with `total` slices: one slice EVENT per lane, into the row its code names.  The lane leaves its
// span; a slice that cannot be read lowers st->err.  Two slices that overlap write the same records - the judge refuses the stream
// before anything reads them
__global__ __launch_bounds__(64) void k_dt_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                  const DecPic *__restrict__ pics, const DecXPic *__restrict__ xp, uint32_t p0, uint32_t np, uint32_t total,
                                                  dec::IMb *mb, int32_t *dc, int16_t *lv, uint32_t *__restrict__ spans)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, nev = st->nev;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= total) return;
    uint32_t k;
    const uint32_t pic = dec::x_slice_pic(xp + p0, np, g, k);
    const DecPic P = pics[p0 + pic];
    const DecXPic Q = xp[p0 + pic];
    const uint32_t i = Q.slice0 + k;
    spans[g] = 0u;
    if (k >= Q.nslices || i >= nev) return;                            // (the plan accepted the picture: its slices are there)
    const unsigned long long start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : n;
    const uint32_t code = dec::ev_code(ev[i]);
    if (code < 1u || code > mbh) { atomicMin(&st->err, start); return; }      // (the plan's grammar: 1 <= code <= mbh)
    const size_t first = ((size_t)pic * mbh + (code - 1u)) * mbw;
    DecTSink sink{mb + first, dc + first * 6, lv + first * 384};
    int c0, c1;
    const bool ok = dec::t_slice(es, start, end, P.type, dec::t_params_unpack(Q.params), (int)mbw, (int)mbh, (int)code - 1, sink, c0, c1);
    spans[g] = dec::x_span_pack(ok, code, c0, c1);
    if (!ok) atomicMin(&st->err, start);
}

// continuity behind the walk: every readable slice against the span of the slice in front of it in its picture
__global__ __launch_bounds__(64) void k_dt_cont(const unsigned long long *__restrict__ ev, DecState *st, const DecXPic *__restrict__ xp, uint32_t p0, uint32_t np,
                                                uint32_t total, const uint32_t *__restrict__ spans)
{
    if (st->status != dec::kOk) return;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= total) return;
    uint32_t k;
    const uint32_t pic = dec::x_slice_pic(xp + p0, np, g, k);
    const DecXPic Q = xp[p0 + pic];
    const uint32_t cur = spans[g];
    if (!(cur >> 31) || k >= Q.nslices || Q.slice0 + k >= st->nev) return;      // (not readable: reported by its walk)
    if (!dec::x_continuous(cur, k ? spans[g - 1] : 0u, k, Q.nslices, st->mbw)) atomicMin(&st->err, dec::ev_pos(ev[Q.slice0 + k]));
}

__global__ void k_dt_judge(DecState *st)
{
    if (st->status == dec::kOk && st->err != dec::kNone) st->status = dec::kSyntax;
}

// the matrix table: block p writes picture p's 128 weights, raster order - the sequence's, or those of the extension in force
__global__ __launch_bounds__(128) void k_dt_mats(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, const DecState *__restrict__ st,
                                                 const uint8_t *__restrict__ mats, const DecXPic *__restrict__ xp, uint8_t *__restrict__ table)
{
    if (st->status != dec::kOk || blockIdx.x >= st->npics) return;
    const uint32_t p = blockIdx.x, l = threadIdx.x, m = l >> 6, t = l & 63u;
    const uint32_t src = m ? xp[p].mn : xp[p].mi;
    table[(size_t)p * 128u + l] = (uint8_t)dec::x_matrix_weight(es, n, (const uint64_t *)ev, st->nev, src, (int)m, t, mats + 64u * m);
}

// the chunk's slot of the picture with coded index r, as m2v_decode_b.hip's
__device__ inline uint32_t dt_slot(uint32_t r, uint32_t p0, uint32_t c1) { return r == kNoPic ? 0u : r >= p0 ? 2u + (r - p0) : r == c1 ? 1u : 0u; }

// as k_di_recon, the weights from the picture's row of the matrix table: grid = (macroblocks, pictures of the launch); list: their coded indices, all of chunk [p0, ...).  Every read of a
// reference lies inside its picture: the slice walk refused the slice otherwise (dec::il_inside), and a refused slice stops the call
// before this kernel (k_dt_judge)
__global__ __launch_bounds__(64) void k_dt_recon(const DecState *__restrict__ st, const uint32_t *__restrict__ list, uint32_t p0, uint32_t c1,
                                                 const uint8_t *__restrict__ mats, const DecXPic *__restrict__ bp, const dec::IMb *__restrict__ mb,
                                                 const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf, size_t psz)
{
    __shared__ int32_t F[6][64];
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, mbs = mbw * mbh, W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const uint32_t k = blockIdx.x, l = threadIdx.x, gp = list[blockIdx.y], pic = gp - p0;
    const DecXPic Q = bp[gp];
    const dec::PicParams pp = dec::params_unpack(Q.params);
    const size_t at = (size_t)pic * mbs + k;
    const dec::IMb m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw;
    uint8_t *cur = buf + (size_t)(pic + 2u) * psz;
    const uint8_t *fwd = buf + (size_t)dt_slot(Q.fwd, p0, c1) * psz, *bwd = buf + (size_t)dt_slot(Q.bwd, p0, c1) * psz;
    const bool intra = m.intra != 0;
    const int32_t qscale = dec::main_scale(m.qcode, pp.qst), weight = mats[(size_t)gp * 128u + (intra ? 0u : 64u) + l];
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

typedef uint32_t dt_store_t __attribute__((ext_vector_type(4)));

// picture blockIdx.y of chunk [p0, p0 + np) into dst at its display index: bytes [display * fb, (display + 1) * fb) of the output
__global__ __launch_bounds__(kDecThreads) void k_dt_out(const DecState *__restrict__ st, const DecXPic *__restrict__ bp, const uint8_t *__restrict__ buf, size_t psz,
                                                        uint32_t p0, uint8_t *__restrict__ dst, int layout)
{
    if (st->status != dec::kOk) return;
    const uint32_t w = st->width, h = st->height, W = 16u * st->mbw, H = 16u * st->mbh;
    const uint32_t d = bp[p0 + blockIdx.y].display;
    if (d >= st->npics) return;                                        // (an accepted stream's display indices are a permutation)
    const uint8_t *pic = buf + (size_t)(blockIdx.y + 2u) * psz;
    const unsigned long long fb = st->frame_bytes, lo = (unsigned long long)d * fb, hi = lo + fb;
    const unsigned long long lead = (unsigned long long)(uintptr_t)dst & 15ull;
    const unsigned long long u0 = (lo + lead) >> 4, u1 = (hi + lead + 15ull) >> 4;
    for (unsigned long long g = u0 + (unsigned long long)blockIdx.x * kDecThreads + threadIdx.x; g < u1; g += (unsigned long long)gridDim.x * kDecThreads) {
        const long long o0 = (long long)(g << 4) - (long long)lead;
        const int k0 = o0 < (long long)lo ? (int)((long long)lo - o0) : 0, k1 = (long long)hi - o0 < 16 ? (int)((long long)hi - o0) : 16;
        if (k0 >= k1) continue;
        uint32_t q = (uint32_t)((unsigned long long)(o0 + k0) - lo);
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
            *(__attribute__((address_space(1))) dt_store_t *)(dst + o0) = dt_store_t{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = k0; k < k1; ++k) dst[o0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

__global__ void k_dt_finish(const DecState *st, m2v_decode_stat *h_rec)
{
    if (st->status == dec::kOk) { h_rec->out_bytes = st->frame_bytes * st->npics; return; }
    h_rec->status = st->status; h_rec->err_offset = st->err; h_rec->out_bytes = 0;
}

void dec_t_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main, int b_pictures, int interlaced, uint32_t *h_mbh, uint32_t *h_sl)
{
    k_dt_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecXPic *)(d_main + kDecMainMatrices), b_pictures, interlaced,
                                        h_mbh, h_sl);
    HIPCHK(hipGetLastError());
}

// dec_x_chunks with this unit's kernels: the matrix table once, then per chunk the walk and the continuity judge over the chunk's slices
// (h_sl[p]: the slices in front of picture p; h_sl[pictures]: all of them) in front of the reconstruction
void dec_t_chunks(m2v_enc *e, hipStream_t s, const uint8_t *es, size_t n, uint8_t *dst, int layout, const m2v_decode_stat &R, size_t mbh, size_t B,
                  const uint8_t *types, uint32_t *h_list, const uint32_t *h_sl, m2v_decode_stat *h_rec)
{
    const size_t np = R.pictures, mbw = (R.width + 15) / 16, mbs = mbw * mbh, psz = mbs * 384;
    size_t most = 1;                                                   // the most slices of a chunk
    for (size_t p0 = 0; p0 < np; p0 += B) most = std::max<size_t>(most, h_sl[std::min(p0 + B, np)] - h_sl[p0]);
    const size_t span_off = (np * 128 + 3) & ~(size_t)3;
    e->d_dec_x.ensure(span_off + most * sizeof(uint32_t));
    e->d_dec_mb.ensure(B * mbs * sizeof(dec::IMb));
    e->d_dec_dc.ensure(B * mbs * 6);
    e->d_dec_lv.ensure(B * mbs * 384);
    e->d_dec_buf.ensure((B + 2) * psz);
    e->d_dec_list.ensure(np);
    // every chunk's anchors ordered by their step inside the chunk - a chain starts at its I picture, or at the chunk's first anchor -,
    // then its B pictures; and what the chunk leaves in slots 0 and 1 for the next
    struct Launch { size_t off, count; };
    struct Chunk { std::vector<Launch> steps; Launch b; long c1, carry0, carry1; };      // carry: the chunk's slot to copy into slot 0 / 1 (-1: nothing)
    std::vector<Chunk> chunks;
    long a1 = -1, a2 = -1;                                             // the last two anchors in front of the chunk, coded indices
    for (size_t p0 = 0; p0 < np; p0 += B) {
        const size_t nb = std::min(B, np - p0);
        Chunk C;
        C.c1 = a1;
        std::vector<long> step(nb, -1);
        long deepest = -1, prev = -1;
        for (size_t k = 0; k < nb; ++k) {
            if (types[p0 + k] == 3) continue;
            step[k] = prev >= 0 && types[p0 + k] != 1 ? step[prev] + 1 : 0;
            deepest = std::max(deepest, step[k]);
            prev = (long)k;
        }
        size_t at = p0;
        for (long j = 0; j <= deepest; ++j) {
            const size_t first = at;
            for (size_t k = 0; k < nb; ++k) if (step[k] == j) h_list[at++] = (uint32_t)(p0 + k);
            C.steps.push_back(Launch{first, at - first});
        }
        C.b.off = at;
        for (size_t k = 0; k < nb; ++k) if (types[p0 + k] == 3) h_list[at++] = (uint32_t)(p0 + k);
        C.b.count = at - C.b.off;
        auto slot = [&](long r) { return r >= (long)p0 ? 2 + (r - (long)p0) : r == C.c1 ? 1L : 0L; };
        long n1 = a1, n2 = a2;
        for (size_t k = 0; k < nb; ++k) if (types[p0 + k] != 3) { n2 = n1; n1 = (long)(p0 + k); }
        C.carry0 = n2 >= 0 && slot(n2) != 0 ? slot(n2) : -1;
        C.carry1 = n1 >= 0 && slot(n1) != 1 ? slot(n1) : -1;
        a1 = n1; a2 = n2;
        chunks.push_back(C);
    }
    auto *d_st = (DecState *)e->d_dec_st.p;
    auto *d_mb = (dec::IMb *)e->d_dec_mb.p;
    const uint8_t *mats = e->d_dec_x.p;                                // the matrix table: 128 bytes a picture
    auto *spans = (uint32_t *)(e->d_dec_x.p + span_off);
    const auto *bp = (const DecXPic *)(e->d_dec_main.p + kDecMainMatrices);
    HIPCHK(hipMemcpyAsync(e->d_dec_list.p, h_list, np * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    k_dt_mats<<<(unsigned)np, 128, 0, s>>>(es, n, e->d_dec_ev.p, d_st, e->d_dec_main.p, bp, e->d_dec_x.p);
    HIPCHK(hipGetLastError());
    for (size_t p0 = 0, c = 0; p0 < np; p0 += B, ++c) {
        const size_t nb = std::min(B, np - p0);
        const Chunk &C = chunks[c];
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, nb * mbs * 768, s));
        const size_t total = h_sl[p0 + nb] - h_sl[p0];                 // (every picture the plan accepted has a slice)
        if (total) {
            k_dt_slices<<<(unsigned)((total + 63) / 64), 64, 0, s>>>(es, n, e->d_dec_ev.p, d_st, (const DecPic *)e->d_dec_pics.p, bp, (uint32_t)p0, (uint32_t)nb,
                                                                     (uint32_t)total, d_mb, e->d_dec_dc.p, e->d_dec_lv.p, spans);
            HIPCHK(hipGetLastError());
            k_dt_cont<<<(unsigned)((total + 63) / 64), 64, 0, s>>>(e->d_dec_ev.p, d_st, bp, (uint32_t)p0, (uint32_t)nb, (uint32_t)total, spans);
            HIPCHK(hipGetLastError());
        }
        k_dt_judge<<<1, 1, 0, s>>>(d_st);
        HIPCHK(hipGetLastError());
        auto recon = [&](const Launch &l) {
            if (!l.count) return;
            k_dt_recon<<<dim3((unsigned)mbs, (unsigned)l.count), 64, 0, s>>>(d_st, e->d_dec_list.p + l.off, (uint32_t)p0, (uint32_t)C.c1, mats, bp, d_mb, e->d_dec_dc.p,
                                                                            e->d_dec_lv.p, e->d_dec_buf.p, psz);
            HIPCHK(hipGetLastError());
        };
        for (const Launch &l : C.steps) recon(l);
        recon(C.b);                                                    // every B picture of the chunk at once: its anchors are done
        const size_t units = (R.frame_bytes + 15) / 16 + 1;
        k_dt_out<<<dim3((unsigned)std::min<size_t>((units + kDecThreads - 1) / kDecThreads, 1024), (unsigned)nb), kDecThreads, 0, s>>>(d_st, bp, e->d_dec_buf.p, psz,
                                                                                                                                      (uint32_t)p0, dst, layout);
        HIPCHK(hipGetLastError());
        if (p0 + B < np) {                                             // the next chunk's carried anchors: slot 0 first (it may come from slot 1)
            if (C.carry0 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + (size_t)C.carry0 * psz, psz, hipMemcpyDeviceToDevice, s));
            if (C.carry1 >= 0) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p + psz, e->d_dec_buf.p + (size_t)C.carry1 * psz, psz, hipMemcpyDeviceToDevice, s));
        }
    }
    k_dt_finish<<<1, 1, 0, s>>>(d_st, h_rec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
}

}  // namespace m2v
