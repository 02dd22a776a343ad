// m2v_decode_main.hip — the main syntax of m2v_decode_device (option "decode_syntax" = M2V_SYNTAX_MAIN): the three kernels in which a
// syntax is hard-wired, in their main-syntax form.  m2v_decode.hip tells the whole story and keeps everything else - the scan, the
// tiles, the chunks, k_dec_judge, k_dec_out, k_dec_finish, the error protocol - and launches these where it launches its own
// k_dec_plan, k_dec_slices and k_dec_recon.  They live in a translation unit of their own so that the module-syntax kernels come out
// of the compiler exactly as they did.  decoder.decode_main is the definition; every function that decides a bit or a sample is a
// main_ function of m2v_decode_kernels.hpp.
//
//   k_dm_plan    one block.  Start codes are significant or transparent (user_data, copyright_extension, picture_display_extension) by
//                what they are; a rule looks at an event and at the significant event in front of it.  Every lane notes the last
//                significant event of its range in LDS, looks back over the lanes in front for the one that precedes its range, and
//                then judges its events on its own as k_dec_plan does.  The picture table gains, per picture, the event of its first
//                slice (transparent units may stand in front of it) and its parameters - both f_codes, DC precision, scale type, scan;
//                the two matrices go to the call's state, 128 bytes in raster order.
//   k_dm_slices  one slice per lane (dec::main_slice): address increments with escapes, skipped macroblocks, all of tables B-2 / B-3,
//                macroblock quantisers, vectors with residuals and the wrap of the picture's f_codes, either scan.  A skipped or No-MC
//                macroblock leaves a record with mc = 0 and the zero vector.  The loops are bounded by mbw, 64 coefficients and the
//                unit's bits; the bit reader ends where the next start code begins.
//   k_dm_recon   one wavefront per macroblock as k_dec_recon: lane l dequantises coefficient l with the stream's weight for it (one
//                byte per lane and matrix from the call's state: no table in registers), the picture's scale table and DC multiplier.
#include "m2v_decode_state.hpp"

static_assert(sizeof(dec::MainMb) == sizeof(dec::MbRec), "the main syntax's record lies where the module's does");

namespace m2v {

__global__ __launch_bounds__(kDecThreads) void k_dm_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                         DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                         m2v_decode_stat *h_rec, uint8_t *__restrict__ mats, DecMainPic *__restrict__ mp)
{
    __shared__ dec::MainPlan s_P;
    __shared__ unsigned long long s_bad;
    __shared__ uint32_t s_np[kDecThreads], s_ng[kDecThreads], s_nr[kDecThreads], s_ni[kDecThreads];
    __shared__ int s_last[kDecThreads], s_sig[kDecThreads];
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
        uint32_t np = 0, ng = 0, nr = 0, ni = 0;
        int last = -1;
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dec::main_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz, prev);
            if (dec::main_significant(dec::main_role(es, n, ev[i]))) prev = (int)i;
            bad = dec::min64(bad, f.bad);
            ng += f.gop; nr += f.rep;
            if (f.pic) { if (f.type == 1) { last = (int)np; ++ni; } ++np; }
        }
        if (bad != dec::kNone) atomicMin(&s_bad, bad);
        s_np[tid] = np; s_ng[tid] = ng; s_nr[tid] = nr; s_ni[tid] = ni; s_last[tid] = last;
    }
    __syncthreads();
    if (tid == 0) {                                // exclusive sums, and the last I picture in front of every range (-1: none)
        uint32_t np = 0, ng = 0, nr = 0, ni = 0;
        int last = -1;
        for (int k = 0; k < kDecThreads; ++k) {
            const uint32_t p = s_np[k], i = s_ni[k];
            const int l = s_last[k];
            s_np[k] = np; s_ni[k] = ni; s_last[k] = last;
            if (l >= 0) last = (int)np + l;
            np += p; ni += i; ng += s_ng[k]; nr += s_nr[k];
        }
        r.pictures = np; r.gops = ng; r.repeated_headers = nr; r.chains = ni;
    }
    __syncthreads();
    {
        uint32_t p = s_np[tid], chain = s_ni[tid];
        int last = s_last[tid];
        for (uint32_t i = a; i < b; ++i) {
            if (dec::ev_code(ev[i]) != 0x00) continue;
            const unsigned long long pos = dec::ev_pos(ev[i]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            if (type == 1) { last = (int)p; ++chain; }
            if (last < 0) atomicMin(&s_bad, pos);                      // a P picture without a reference
            if (p < pic_cap) {
                DecMainPic q;
                q.params = dec::main_picture_params(es, n, (const uint64_t *)ev, nev, i, q.slice0);
                pics[p] = DecPic{i, type, chain - 1u, (uint32_t)((int)p - last)}; h_types[p] = (uint8_t)type;
                mp[p] = q;
            }
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
    else if (!probe && r.frame_bytes * r.pictures > cap) r.status = dec::kOverflow;
    else if (probe) r.out_bytes = r.frame_bytes * r.pictures;
    st->status = r.status; st->err = s_bad; st->npics = r.pictures; st->gops = r.gops; st->reps = r.repeated_headers; st->chains = r.chains;
    st->width = r.width; st->height = r.height; st->mbw = P.mbw; st->mbh = P.mbh; st->frame_bytes = r.frame_bytes;
    *h_rec = r;
}

struct DecMainSink {
    dec::MainMb *mb_;
    int32_t *dc_;
    int16_t *lv_;
    M2V_HD void mb(int col, const dec::MainMb &m, const int32_t (&dc)[6])
    {
        mb_[col] = m;
#pragma unroll
        for (int k = 0; k < 6; ++k) dc_[col * 6 + k] = dc[k];
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { lv_[(col * 6 + blk) * 64 + (int)i] = (int16_t)l; }
};

// as k_dec_slices: pictures [p0, p0 + np), one slice per lane, the earliest refused slice lowers st->err
__global__ __launch_bounds__(64) void k_dm_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                  const DecPic *__restrict__ pics, const DecMainPic *__restrict__ mp, uint32_t p0, uint32_t np, dec::MainMb *mb,
                                                  int32_t *dc, int16_t *lv)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, nev = st->nev;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x, pic = g / mbh, row = g - pic * mbh;
    if (pic >= np) return;
    const DecPic P = pics[p0 + pic];
    const DecMainPic Q = mp[p0 + pic];
    const uint32_t i = Q.slice0 + row;
    if (i >= nev) return;                                              // (the plan accepted the picture: its slices are there)
    const unsigned long long start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : n;
    const size_t first = ((size_t)pic * mbh + row) * mbw;
    DecMainSink sink{mb + first, dc + first * 6, lv + first * 384};
    if (!dec::main_slice(es, start, end, P.type, dec::params_unpack(Q.params), (int)mbw, (int)mbh, (int)row, sink)) atomicMin(&st->err, start);
}

// as k_dec_recon, in M2V_DEC_ISO's arithmetic: grid = (macroblocks, pictures of the step)
__global__ __launch_bounds__(64) void k_dm_recon(const DecState *__restrict__ st, const uint32_t *__restrict__ list, uint32_t p0, const uint8_t *__restrict__ mats,
                                                 const DecMainPic *__restrict__ mp, const dec::MainMb *__restrict__ mb, const int32_t *__restrict__ dc,
                                                 const int16_t *__restrict__ lv, uint8_t *buf, size_t psz)
{
    __shared__ int32_t F[6][64];
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, mbs = mbw * mbh, W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const uint32_t k = blockIdx.x, l = threadIdx.x, gp = list[blockIdx.y], pic = gp - p0;
    const dec::PicParams pp = dec::params_unpack(mp[gp].params);
    const size_t at = (size_t)pic * mbs + k;
    const dec::MainMb m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw;
    uint8_t *cur = buf + (size_t)(pic + 1u) * psz;
    const uint8_t *ref = buf + (size_t)pic * psz;
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
    {   // luma: four samples of one row per lane
        const uint32_t y = l >> 2, x0 = (l & 3u) * 4u, blk = (y >> 3) * 2u + (x0 >> 3);
        const bool coded = (m.cbp >> (5 - blk)) & 1;
        const int px = (int)(16u * col + x0) + (m.mvx >> 1), py = (int)(16u * row + y) + (m.mvy >> 1);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t pred = intra ? 128 : dec::predict(ref, (int)W, px + j, py, m.mvx & 1, m.mvy & 1, dec::kIso);
            const int32_t res = coded ? F[blk][(y & 7u) * 8u + ((x0 + j) & 7u)] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint32_t *)(cur + (size_t)(16u * row + y) * W + 16u * col + x0) = v;
    }
    {   // chroma: two samples per lane, U in the first half of the wavefront
        const uint32_t pl = l >> 5, y = (l >> 2) & 7u, x0 = (l & 3u) * 2u;
        const bool coded = (m.cbp >> (1 - pl)) & 1;
        const int cx = dec::chroma_vector(m.mvx, dec::kIso), cy = dec::chroma_vector(m.mvy, dec::kIso);
        const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2u);
        const int px = (int)(8u * col + x0) + (cx >> 1), py = (int)(8u * row + y) + (cy >> 1);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t pred = intra ? 128 : dec::predict(ref + plane, (int)CW, px + j, py, cx & 1, cy & 1, dec::kIso);
            const int32_t res = coded ? F[4u + pl][y * 8u + x0 + j] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint16_t *)(cur + plane + (size_t)(8u * row + y) * CW + 8u * col + x0) = (uint16_t)v;
    }
}

void dec_main_plan(hipStream_t s, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, DecPic *pics, uint32_t pic_cap, uint8_t *h_types,
                   unsigned long long cap, int probe, m2v_decode_stat *h_rec, uint8_t *d_main)
{
    k_dm_plan<<<1, kDecThreads, 0, s>>>(es, n, ev, st, pics, pic_cap, h_types, cap, probe, h_rec, d_main, (DecMainPic *)(d_main + kDecMainMatrices));
    HIPCHK(hipGetLastError());
}

void dec_main_slices(hipStream_t s, unsigned blocks, const uint8_t *es, size_t n, const unsigned long long *ev, DecState *st, const DecPic *pics, const uint8_t *d_main,
                     uint32_t p0, uint32_t np, dec::MbRec *mb, int32_t *dc, int16_t *lv)
{
    k_dm_slices<<<blocks, 64, 0, s>>>(es, n, ev, st, pics, (const DecMainPic *)(d_main + kDecMainMatrices), p0, np, (dec::MainMb *)mb, dc, lv);
    HIPCHK(hipGetLastError());
}

void dec_main_recon(hipStream_t s, unsigned mbs, unsigned count, const DecState *st, const uint32_t *list, uint32_t p0, const uint8_t *d_main, const dec::MbRec *mb,
                    const int32_t *dc, const int16_t *lv, uint8_t *buf, size_t psz)
{
    k_dm_recon<<<dim3(mbs, count), 64, 0, s>>>(st, list, p0, d_main, (const DecMainPic *)(d_main + kDecMainMatrices), (const dec::MainMb *)mb, dc, lv, buf, psz);
    HIPCHK(hipGetLastError());
}

}  // namespace m2v
