// m2v_decode.hip — MPEG-2 I / P streams back to 4:2:0 frames, on the device (include/m2v_mi355x.h: m2v_decode_device).  Reading a stream
// is decoder.py on one CPU core; here it is a handful of kernels over a stream that stays in HBM, and the bytes are those of
// decoder.decode exactly (decoder.py is the specification; m2v_decode_kernels.hpp holds every function that decides a bit or a sample,
// and compiles for the host too).
//
//   k_dec_scan    all blocks, 16 stream bytes per lane, a tile of dec::kScanTile bytes per block: 00 00 01 xx at any position is a start
//                 code, slices included.  First launch: the count of every tile.  k_dec_tiles: one block, the prefix sum over the tiles.
//                 Second launch: the same scan emits position << 8 | code at tile offset + the lane's place inside the block (a
//                 wavefront prefix and four wave totals in LDS).  The list is in stream order by construction: no sort, and nothing
//                 depends on the order of atomics.  The one atomic is a maximum, the last byte that is not zero.
//   k_dec_plan    one block.  decoder.decode's grammar over the ordered codes is local - a rule looks at an event and the three in front
//                 of it (dec::plan_event) - so every lane judges a contiguous range of events on its own: header parsers, the repeated
//                 sequence headers against the first, slices one per macroblock row in order.  Counts (pictures, GOPs, repeats, I
//                 pictures) and the last I picture in front of a range are a 256-entry scan in LDS; a second pass writes the picture
//                 table (event, type, chain, step).  The earliest error is a minimum over offsets.  The record and every picture's type
//                 go straight into pinned memory: the host's one wait is behind this kernel.
//   k_dec_slices  the serial part, one slice per lane over every picture of the chunk at once (dec::parse_slice): type, vector deltas
//                 with the wrap, pattern, DC sizes, run / level with the first-coefficient form, escape, end of block, the zero stuffing
//                 up to the next start code.  Leaves a 16-byte record and six DC values per macroblock and the quantised levels as dense
//                 int16 [6][64], raster order, zeroed beforehand.  The bit reader ends where the next start code begins; every loop is
//                 bounded by mbw, 64 coefficients and the unit's bits.  Vectors are checked against the picture here.
//   k_dec_recon   one launch per step j over the j-th picture of every chain of the chunk, one wavefront per macroblock: a lane per
//                 coefficient dequantises (mismatch control through one ballot), 48 lanes run the Chen-Wang rows and then the columns
//                 through LDS, then a lane per four luma and two chroma samples predicts from the picture before, clips and stores.
//   k_dec_out     the chunk's pictures cropped and packed into the caller's buffer: one lane per 16 bytes at a 16-byte boundary of the
//                 destination, one aligned store; the first and last unit of the chunk's range go byte by byte.
//
// A chunk's pictures stay in the handle's buffer as planar frames of whole macroblocks (slot 0: the last picture of the chunk before), so
// a P picture's reference is the slot in front of it and the output is one pass per chunk instead of one per step.  An error that
// k_dec_slices finds stays on the device: its lanes lower the error offset with a minimum and none of them reads it, so all slices of
// the chunk are walked and the offset is the earliest whatever the scheduling; k_dec_judge, one lane behind them, turns it into the
// status, the later kernels of the call read the status and return at once (a later chunk holds later offsets only), and k_dec_finish
// copies the verdict into the pinned record behind the last chunk.  No encoder kernel is touched; a handle that never decodes allocates nothing here.
//
// Option "decode_syntax" = M2V_SYNTAX_MAIN puts the main-syntax variants of k_dec_plan, k_dec_slices and k_dec_recon in their places
// (m2v_decode_main.hip, a translation unit of its own: the three kernels here are what they were); the rest of the call is shared.
// Option "decode_b_pictures" = 1 on top of that: B pictures, frames in display order.  The scan stays; the plan and everything behind
// its wait are m2v_decode_b.hip's (dec_b_plan, dec_b_chunks), again a translation unit of its own.  Option "decode_interlaced" = 1,
// with "decode_b_pictures" either way: frame pictures with frame_pred_frame_dct 0; the same two places go to m2v_decode_i.hip
// (dec_i_plan, dec_i_chunks).  Option "decode_extended" = 1, with the other two either way: several slices a row, slice header extras,
// quant_matrix_extension, composite_display_flag 1; the same two places go to m2v_decode_x.hip (dec_x_plan, dec_x_chunks).  Option
// "decode_mb_tools" = 1 on top of "decode_extended": Table B-15, concealment motion vectors, dual prime; the plan is m2v_decode_t.hip's
// (dec_t_plan), and dec_x_chunks takes the option as `tools`.
// "decode_field_pictures" = 1 on top of "decode_interlaced", "decode_extended" and "decode_mb_tools": picture_structure 1 / 2, two field
// pictures a frame; from the same two places to m2v_decode_f.hip (dec_f_plan, dec_f_chunks), whose chunks are whole frames.
// "decode_join" = 1 .. 3 on top of all of them: a stream that begins in front of its first sequence header, whose first B pictures lack
// their anchors, or that breaks off inside a picture; the plan is m2v_decode_j.hip's (dec_j_plan), the chunks stay dec_f_chunks.
// "decode_conceal" = 1 on top of "decode_field_pictures" and what it needs, "decode_join" 0 .. 3: damaged slices are dropped, their rows
// patched from the frame in front; the plan is dec_c_plan, dec_f_chunks hands the walk to m2v_decode_c.hip (dec_c_walk, dec_c_finish).
#include "m2v_decode_state.hpp"

static_assert(sizeof(m2v_decode_stat) == 72, "the record of include/m2v_mi355x.h is 72 bytes");
static_assert(sizeof(m2v_decode_join) == 32, "the join record of include/m2v_mi355x.h is 32 bytes");
static_assert(sizeof(m2v_decode_conceal) == 32, "the concealment report of include/m2v_mi355x.h is 32 bytes");
static_assert(sizeof(dec::MbRec) == 16, "a macroblock's record is 16 bytes");
static_assert(M2V_DEC_ISO == dec::kIso && M2V_DEC_MODULE == dec::kModule && M2V_DEC_SYNTAX == dec::kSyntax && M2V_DEC_OVERFLOW == dec::kOverflow,
              "m2v_decode_kernels.hpp repeats the values of include/m2v_mi355x.h");

namespace m2v {

constexpr size_t kDecLevelBytes = 256u << 20;      // the default "decode_batch" keeps the chunk's levels within this
constexpr size_t kDecBatchMax = 256;
static_assert(dec::kScanTile == (uint32_t)kDecThreads * 16u, "a tile is one pass of a block");

template <bool EMIT>
__global__ __launch_bounds__(kDecThreads) void k_dec_scan(const uint8_t *__restrict__ es, unsigned long long n, DecState *st, uint32_t *__restrict__ tiles,
                                                          unsigned long long *__restrict__ ev)
{
    __shared__ uint32_t s_w[kDecThreads / 64];
    const unsigned long long ntiles = (n + dec::kScanTile - 1) / dec::kScanTile;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t ev_cap = st->ev_cap;
    uint64_t nz = 0;                                                   // over all of the block's tiles: one atomic per wavefront at the end
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned long long p0 = t * dec::kScanTile + (unsigned long long)tid * 16u;
        uint64_t w0 = 0, w1 = 0, w2 = 0;
        uint32_t cand = 0;
        if (p0 < n) {
            mux::load24(es, p0, n, w0, w1, w2);
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
        uint32_t base = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kDecThreads / 64; ++k) { if (k < wave) base += s_w[k]; total += s_w[k]; }
        if (!EMIT) {
            if (tid == 0) tiles[t] = total;
        } else {
            uint32_t at = tiles[t] + base + incl - c;
            while (cand) {
                const uint32_t j = (uint32_t)__builtin_ctz(cand);
                cand &= cand - 1u;
                if (at < ev_cap) ev[at] = (p0 + j) << 8 | mux::byte24(w0, w1, w2, j + 3);
                ++at;
            }
        }
        __syncthreads();
    }
    if (!EMIT) {
#pragma unroll
        for (int d = 32; d; d >>= 1) nz = mux::max64(nz, __shfl_xor(nz, d));
        if (lane == 0 && nz) atomicMax(&st->last_nz, (unsigned long long)nz);
    }
}

// counts -> offsets in place; the total is the number of events
__global__ __launch_bounds__(kDecThreads) void k_dec_tiles(uint32_t *tiles, uint32_t ntiles, DecState *st)
{
    __shared__ uint32_t s_sum[kDecThreads];
    const uint32_t tid = threadIdx.x, per = (ntiles + kDecThreads - 1) / kDecThreads;
    const uint32_t a = min(ntiles, tid * per), b = min(ntiles, a + per);
    uint32_t sum = 0;
    for (uint32_t t = a; t < b; ++t) sum += tiles[t];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kDecThreads; ++k) { const uint32_t v = s_sum[k]; s_sum[k] = run; run += v; }
        st->nev = run;
        if (run > st->ev_cap) st->status = dec::kEvents;
    }
    __syncthreads();
    uint32_t run = s_sum[tid];
    for (uint32_t t = a; t < b; ++t) { const uint32_t v = tiles[t]; tiles[t] = run; run += v; }
}

__global__ __launch_bounds__(kDecThreads) void k_dec_plan(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                          DecPic *__restrict__ pics, uint32_t pic_cap, uint8_t *h_types, unsigned long long cap, int probe,
                                                          m2v_decode_stat *h_rec)
{
    __shared__ dec::Plan s_P;
    __shared__ unsigned long long s_bad;
    __shared__ uint32_t s_np[kDecThreads], s_ng[kDecThreads], s_nr[kDecThreads], s_ni[kDecThreads];
    __shared__ int s_last[kDecThreads];
    const uint32_t tid = threadIdx.x, nev = st->nev;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (st->status == dec::kEvents) {              // the list was too small: the call runs again with the count
        if (tid == 0) { r.status = dec::kEvents; r.pictures = nev; *h_rec = r; }
        return;
    }
    if (tid == 0) {
        dec::Plan P{};
        s_bad = dec::plan_first(es, n, (const uint64_t *)ev, nev, P);
        s_P = P;
    }
    __syncthreads();
    if (s_bad != dec::kNone) {
        if (tid == 0) { st->status = dec::kSyntax; st->err = s_bad; r.status = dec::kSyntax; r.err_offset = s_bad; *h_rec = r; }
        return;
    }
    const dec::Plan P = s_P;
    const unsigned long long last_nz = st->last_nz;
    const uint32_t per = (nev + kDecThreads - 1) / kDecThreads, a = min(nev, tid * per), b = min(nev, a + per);
    {
        unsigned long long bad = dec::kNone;
        uint32_t np = 0, ng = 0, nr = 0, ni = 0;
        int last = -1;
        for (uint32_t i = a; i < b; ++i) {
            const dec::EvInfo f = dec::plan_event(es, n, (const uint64_t *)ev, nev, i, P, last_nz);
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
            if (p < pic_cap) { pics[p] = DecPic{i, type, chain - 1u, (uint32_t)((int)p - last)}; h_types[p] = (uint8_t)type; }
            ++p;
        }
    }
    __syncthreads();
    if (tid) return;
    r.width = P.seq.width; r.height = P.seq.height;
    r.frame_bytes = dec::frame_bytes(P.seq.width, P.seq.height);
    if (s_bad != dec::kNone) { r.status = dec::kSyntax; r.err_offset = s_bad; }
    else if (r.pictures > pic_cap) { r.status = dec::kSyntax; r.err_offset = 0; }      // (cannot happen: a picture is three events at least)
    else if (!probe && r.frame_bytes * r.pictures > cap) r.status = dec::kOverflow;
    else if (probe) r.out_bytes = r.frame_bytes * r.pictures;
    st->status = r.status; st->err = s_bad; st->npics = r.pictures; st->gops = r.gops; st->reps = r.repeated_headers; st->chains = r.chains;
    st->width = r.width; st->height = r.height; st->mbw = P.mbw; st->mbh = P.mbh; st->frame_bytes = r.frame_bytes;
    *h_rec = r;
}

struct DecSink {
    dec::MbRec *mb_;
    int32_t *dc_;
    int16_t *lv_;
    M2V_HD void mb(int col, const dec::MbRec &m, const int32_t (&dc)[6])
    {
        mb_[col] = m;
#pragma unroll
        for (int k = 0; k < 6; ++k) dc_[col * 6 + k] = dc[k];
    }
    M2V_HD void level(int col, int blk, uint32_t i, int32_t l) { lv_[(col * 6 + blk) * 64 + (int)i] = (int16_t)l; }
};

// pictures [p0, p0 + np) of the stream; mb / dc / lv: the chunk's records, [np][mbs] macroblocks.  The status read here is what the
// launches in front wrote (the plan, k_dec_judge behind the chunk before); this launch only lowers st->err, which none of its lanes
// reads: every slice of the chunk is walked whatever the others find, so the minimum is over all of them
__global__ __launch_bounds__(64) void k_dec_slices(const uint8_t *__restrict__ es, unsigned long long n, const unsigned long long *__restrict__ ev, DecState *st,
                                                   const DecPic *__restrict__ pics, uint32_t p0, uint32_t np, int mode, dec::MbRec *mb, int32_t *dc, int16_t *lv)
{
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, nev = st->nev;
    const uint32_t g = blockIdx.x * 64u + threadIdx.x, pic = g / mbh, row = g - pic * mbh;
    if (pic >= np) return;
    const DecPic P = pics[p0 + pic];
    const uint32_t i = P.ev + 2u + row;
    if (i >= nev) return;                                              // (the plan accepted the picture: its slices are there)
    const unsigned long long start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : n;
    const size_t first = ((size_t)pic * mbh + row) * mbw;
    DecSink sink{mb + first, dc + first * 6, lv + first * 384};
    if (!dec::parse_slice(es, start, end, P.type, (int)mbw, (int)mbh, (int)row, mode, sink)) atomicMin(&st->err, start);
}

// behind a chunk's k_dec_slices, one lane: what the slices found becomes the status that every later kernel of the call reads
__global__ void k_dec_judge(DecState *st)
{
    if (st->status == dec::kOk && st->err != dec::kNone) st->status = dec::kSyntax;
}

// grid = (macroblocks, pictures of the step); list: their picture numbers.  buf: the chunk's planar pictures, slot 0 the picture in
// front of picture p0
__global__ __launch_bounds__(64) void k_dec_recon(const DecState *__restrict__ st, const uint32_t *__restrict__ list, uint32_t p0, int mode,
                                                  const dec::MbRec *__restrict__ mb, const int32_t *__restrict__ dc, const int16_t *__restrict__ lv,
                                                  uint8_t *buf, size_t psz)
{
    __shared__ int32_t F[6][64];
    if (st->status != dec::kOk) return;
    const uint32_t mbw = st->mbw, mbh = st->mbh, mbs = mbw * mbh, W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const uint32_t k = blockIdx.x, l = threadIdx.x, pic = list[blockIdx.y] - p0;
    const size_t at = (size_t)pic * mbs + k;
    const dec::MbRec m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw;
    uint8_t *cur = buf + (size_t)(pic + 1u) * psz;
    const uint8_t *ref = buf + (size_t)pic * psz;
    const bool intra = m.intra != 0;
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
        if (!((m.cbp >> (5 - blk)) & 1)) continue;                     // (uniform: the whole wavefront works on one macroblock)
        int32_t f = intra && l == 0 ? dec::dequant_dc(dc[at * 6 + blk], mode) : dec::dequant(lv[(at * 6 + blk) * 64 + l], l, intra, 2 * m.qcode, mode);
        if (mode == dec::kIso) {
            const int odd = __popcll(__ballot(f & 1)) & 1;
            if (!odd && l == 63) f = dec::mismatch(f);
        }
        F[blk][l] = f;
    }
    __syncthreads();
    const int blk8 = (int)(l >> 3), r8 = (int)(l & 7u);
    const bool mine = l < 48 && ((m.cbp >> (5 - blk8)) & 1);
    if (mine) {
        int32_t a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = F[blk8][r8 * 8 + j];
        dec::idct_1d(a, true, mode);
#pragma unroll
        for (int j = 0; j < 8; ++j) F[blk8][r8 * 8 + j] = a[j];
    }
    __syncthreads();
    if (mine) {
        int32_t a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = F[blk8][j * 8 + r8];
        dec::idct_1d(a, false, mode);
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
            const int32_t pred = intra ? 128 : dec::predict(ref, (int)W, px + j, py, m.mvx & 1, m.mvy & 1, mode);
            const int32_t res = coded ? F[blk][(y & 7u) * 8u + ((x0 + j) & 7u)] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint32_t *)(cur + (size_t)(16u * row + y) * W + 16u * col + x0) = v;
    }
    {   // chroma: two samples per lane, U in the first half of the wavefront
        const uint32_t pl = l >> 5, y = (l >> 2) & 7u, x0 = (l & 3u) * 2u;
        const bool coded = (m.cbp >> (1 - pl)) & 1;
        const int cx = dec::chroma_vector(m.mvx, mode), cy = dec::chroma_vector(m.mvy, mode);
        const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2u);
        const int px = (int)(8u * col + x0) + (cx >> 1), py = (int)(8u * row + y) + (cy >> 1);
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t pred = intra ? 128 : dec::predict(ref + plane, (int)CW, px + j, py, cx & 1, cy & 1, mode);
            const int32_t res = coded ? F[4u + pl][y * 8u + x0 + j] : 0;
            v |= (uint32_t)dec::clip255(pred + res) << (8 * j);
        }
        *(uint16_t *)(cur + plane + (size_t)(8u * row + y) * CW + 8u * col + x0) = (uint16_t)v;
    }
}

typedef uint32_t dec_store_t __attribute__((ext_vector_type(4)));

// the frames of pictures [p0, p0 + np) into dst: bytes [p0 * fb, (p0 + np) * fb) of the output
__global__ __launch_bounds__(kDecThreads) void k_dec_out(const DecState *__restrict__ st, const uint8_t *__restrict__ buf, size_t psz, uint32_t p0, uint32_t np,
                                                         uint8_t *__restrict__ dst, int layout)
{
    if (st->status != dec::kOk) return;
    const uint32_t w = st->width, h = st->height, W = 16u * st->mbw, H = 16u * st->mbh;
    const unsigned long long fb = st->frame_bytes, lo = (unsigned long long)p0 * fb, hi = lo + (unsigned long long)np * fb;
    const unsigned long long lead = (unsigned long long)(uintptr_t)dst & 15ull;
    const unsigned long long u0 = (lo + lead) >> 4, u1 = (hi + lead + 15ull) >> 4;
    for (unsigned long long g = u0 + (unsigned long long)blockIdx.x * kDecThreads + threadIdx.x; g < u1; g += (unsigned long long)gridDim.x * kDecThreads) {
        const long long o0 = (long long)(g << 4) - (long long)lead;
        const int k0 = o0 < (long long)lo ? (int)((long long)lo - o0) : 0, k1 = (long long)hi - o0 < 16 ? (int)((long long)hi - o0) : 16;
        if (k0 >= k1) continue;
        unsigned long long o = (unsigned long long)(o0 + k0);
        unsigned long long frame = o / fb;
        uint32_t q = (uint32_t)(o - frame * fb);
        const uint8_t *pic = buf + (size_t)(frame - p0 + 1u) * psz;
        dec::OutAt at = dec::out_locate(q, w, h, layout);
        uint32_t v[4] = {0, 0, 0, 0};
        for (int k = k0; k < k1; ++k) {
            v[k >> 2] |= (uint32_t)dec::pic_sample(pic, W, H, at) << (8 * (k & 3));
            if (k + 1 == k1) break;
            if (++q == (uint32_t)fb) { q = 0; pic += psz; at = dec::out_locate(0, w, h, layout); }
            else if (at.run > 1) dec::out_step(at, layout);
            else at = dec::out_locate(q, w, h, layout);
        }
        if (k0 == 0 && k1 == 16) {
            *(__attribute__((address_space(1))) dec_store_t *)(dst + o0) = dec_store_t{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = k0; k < k1; ++k) dst[o0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

__global__ void k_dec_finish(const DecState *st, m2v_decode_stat *h_rec)
{
    if (st->status == dec::kOk) { h_rec->out_bytes = st->frame_bytes * st->npics; return; }
    h_rec->status = st->status; h_rec->err_offset = st->err; h_rec->out_bytes = 0;
}

void dec_release(m2v_enc *e)
{
    e->d_dec_st.release(); e->d_dec_tiles.release(); e->d_dec_ev.release(); e->d_dec_pics.release(); e->d_dec_mb.release(); e->d_dec_dc.release();
    e->d_dec_lv.release(); e->d_dec_buf.release(); e->d_dec_list.release(); e->d_dec_main.release(); e->d_dec_x.release();
    if (e->h_dec) (void)hipHostFree(e->h_dec);
    e->h_dec = nullptr; e->h_dec_cap = 0;
}

}  // namespace m2v

struct DecodeArgs { const uint8_t *es; size_t n; uint8_t *dst; size_t cap; int layout, mode; hipStream_t s; };

static int decode_impl(m2v_enc *e, void *argp)
{
    auto *a = (DecodeArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    const size_t n = a->n;
    m2v_decode_stat &R = e->dec_rec;
    R = m2v_decode_stat{};
    R.es_bytes = n;
    e->dec_join = m2v_decode_join{0, n, 0, 0, {0, 0}};
    e->dec_conceal = m2v_decode_conceal{n, 0, 0, 0, 0, {0, 0}};
    if (n < 4) { R.status = M2V_DEC_SYNTAX; return M2V_OK; }          // not one start code
    e->d_dec_st.recorded = e->d_dec_ev.recorded = e->d_dec_pics.recorded = e->d_dec_mb.recorded = e->d_dec_dc.recorded = false;     // (no recorded graph references them)
    e->d_dec_lv.recorded = e->d_dec_buf.recorded = e->d_dec_tiles.recorded = e->d_dec_list.recorded = e->d_dec_main.recorded = false;
    const bool main_syntax = e->decode_syntax == M2V_SYNTAX_MAIN;      // the main-syntax kernels in the places of k_dec_plan, k_dec_slices, k_dec_recon
    const bool b_pictures = e->decode_b_pictures != 0;                 // m2v_decode_b.hip: its plan, and everything behind the plan's wait
    const bool interlaced = e->decode_interlaced != 0;                 // m2v_decode_i.hip: the same two places, with b_pictures either way
    const bool extended = e->decode_extended != 0;                     // m2v_decode_x.hip: the same two places, with the other two either way
    const bool mb_tools = e->decode_mb_tools != 0;                     // m2v_decode_t.hip: its plan in the place of dec_x_plan; dec_x_chunks takes it
    const bool field_pictures = e->decode_field_pictures != 0;         // m2v_decode_f.hip: in the places of dec_t_plan and dec_x_chunks
    const int join = e->decode_join;                                   // m2v_decode_j.hip: its plan in the place of dec_f_plan, dec_f_chunks behind it
    const bool conceal = e->decode_conceal != 0;                       // m2v_decode_c.hip: dec_c_plan in the place of either, dec_f_chunks with its walk
    e->d_dec_x.recorded = false;
    const size_t ntiles = (n + dec::kScanTile - 1) / dec::kScanTile;
    if (ntiles > 0x7FFFFFFFu) { e->set_err("m2v_decode_device: the stream is longer than 2^31 scan tiles"); return M2V_E_PARAM; }
    size_t ev_cap = std::max<size_t>(1024, n / 16 + 64);              // a guess: a second run takes the count of the first
    size_t pic_cap = 0, rec_off = 0;
    const m2v_decode_stat *h_rec = nullptr;
    timer_break(e);
    for (int run = 0; run < 2; ++run) {
        if (ev_cap > 0x7FFFFFFFu) { e->set_err("m2v_decode_device: the stream holds more than 2^31 start codes"); return M2V_E_PARAM; }
        pic_cap = conceal ? ev_cap / 2 + 2 : ev_cap / 3 + 2;          // (a picture is three events at least - two where its slices may be gone)
        e->d_dec_st.ensure(sizeof(DecState));
        e->d_dec_tiles.ensure(ntiles);
        e->d_dec_ev.ensure(ev_cap);
        e->d_dec_pics.ensure(pic_cap * sizeof(DecPic));
        rec_off = (sizeof(DecState) + 63) & ~(size_t)63;
        ensure_pinned(e->h_dec, e->h_dec_cap, rec_off + 128 + pic_cap + 4 * pic_cap + 16 + (extended ? 4 * (pic_cap + 1) : 0) +
                      (conceal ? 8 + 4 * kDecConcealWords : 0));      // extended: the slices in front of every picture; conceal: the report behind them
        auto *init = (DecState *)e->h_dec;
        *init = DecState{};
        init->err = dec::kNone; init->ev_cap = (uint32_t)ev_cap; init->c_first = dec::kNone;
        auto *d_st = (DecState *)e->d_dec_st.p;
        HIPCHK(hipMemcpyAsync(d_st, init, sizeof(DecState), hipMemcpyHostToDevice, s));
        const unsigned gx = (unsigned)std::min<size_t>(ntiles, 512);
        k_dec_scan<false><<<gx, kDecThreads, 0, s>>>(a->es, n, d_st, e->d_dec_tiles.p, e->d_dec_ev.p);
        HIPCHK(hipGetLastError());
        k_dec_tiles<<<1, kDecThreads, 0, s>>>(e->d_dec_tiles.p, (uint32_t)ntiles, d_st);
        HIPCHK(hipGetLastError());
        k_dec_scan<true><<<gx, kDecThreads, 0, s>>>(a->es, n, d_st, e->d_dec_tiles.p, e->d_dec_ev.p);
        HIPCHK(hipGetLastError());
        if (conceal) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecFPic));
            dec_c_plan(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap, a->dst ? 0 : 1,
                       (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p, b_pictures ? 1 : 0, join, (uint32_t *)(e->h_dec + rec_off + kDecPlanWords),
                       (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3) + 4 * pic_cap));
        } else if (join) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecFPic));
            dec_j_plan(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap, a->dst ? 0 : 1,
                       (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p, b_pictures ? 1 : 0, join, (uint32_t *)(e->h_dec + rec_off + kDecPlanWords),
                       (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3) + 4 * pic_cap));
        } else if (field_pictures) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecFPic));
            dec_f_plan(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap, a->dst ? 0 : 1,
                       (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p, b_pictures ? 1 : 0, (uint32_t *)(e->h_dec + rec_off + 96),
                       (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3) + 4 * pic_cap));
        } else if (extended) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecXPic));
            (mb_tools ? dec_t_plan : dec_x_plan)(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap,
                       a->dst ? 0 : 1, (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p, b_pictures ? 1 : 0, interlaced ? 1 : 0,
                       (uint32_t *)(e->h_dec + rec_off + 96), (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3) + 4 * pic_cap));
        } else if (interlaced) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecBPic));
            dec_i_plan(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap,
                       a->dst ? 0 : 1, (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p, b_pictures ? 1 : 0, (uint32_t *)(e->h_dec + rec_off + 96));
        } else if (b_pictures) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecBPic));
            dec_b_plan(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap,
                       a->dst ? 0 : 1, (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p);
        } else if (main_syntax) {
            e->d_dec_main.ensure(kDecMainMatrices + pic_cap * sizeof(DecMainPic));
            dec_main_plan(s, a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128, (unsigned long long)a->cap,
                          a->dst ? 0 : 1, (m2v_decode_stat *)(e->h_dec + rec_off), e->d_dec_main.p);
        } else {
            k_dec_plan<<<1, kDecThreads, 0, s>>>(a->es, n, e->d_dec_ev.p, d_st, (DecPic *)e->d_dec_pics.p, (uint32_t)pic_cap, e->h_dec + rec_off + 128,
                                                 (unsigned long long)a->cap, a->dst ? 0 : 1, (m2v_decode_stat *)(e->h_dec + rec_off));
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(s));                              // the call's one wait for the plan: pictures, size, types
        h_rec = (const m2v_decode_stat *)(e->h_dec + rec_off);
        if (h_rec->status != dec::kEvents) break;
        ev_cap = h_rec->pictures;                                     // (the count of events travels there)
    }
    R = *h_rec;
    if (R.status == dec::kEvents) R.status = M2V_DEC_SYNTAX;
    if (join && R.status != M2V_DEC_SYNTAX) {                          // the plan's join record, behind the macroblock rows and the coded pictures
        const uint32_t *j = (const uint32_t *)(e->h_dec + rec_off + kDecPlanWords) + kDecJoinWord;
        e->dec_join = m2v_decode_join{(uint64_t)j[1] << 32 | j[0], (uint64_t)j[3] << 32 | j[2], j[4], j[5], {0, 0}};
    }
    if (R.status != M2V_DEC_OK || !a->dst || !R.pictures) return M2V_OK;
    // the chunks
    const uint8_t *types = e->h_dec + rec_off + 128;
    const size_t np = R.pictures, mbw = (R.width + 15) / 16, mbh = (R.height + 15) / 16, mbs = mbw * mbh, psz = mbs * 384;
    size_t B = e->decode_batch ? e->decode_batch : std::max<size_t>(1, std::min(kDecBatchMax, kDecLevelBytes / (mbs * 768)));
    B = std::min(B, np);
    if (field_pictures) {                                              // m2v_decode_f.hip; the record's pictures are frames, and so is "decode_batch"
        const size_t rows = *(const uint32_t *)(e->h_dec + rec_off + 96), ncp = *(const uint32_t *)(e->h_dec + rec_off + 100);
        if (!e->decode_batch) B = std::min(np, std::max<size_t>(1, std::min(kDecBatchMax, kDecLevelBytes / (mbw * rows * 768))));
        auto *h_list = (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3));
        // the report's words: behind the slices in front of every picture, on an 8-byte boundary
        uint32_t *h_conceal = conceal ? (uint32_t *)(e->h_dec + ((rec_off + 128 + ((pic_cap + 3) & ~(size_t)3) + 4 * pic_cap + 4 * (pic_cap + 1) + 7) & ~(size_t)7)) : nullptr;
        dec_f_chunks(e, s, a->es, n, a->dst, a->layout, R, rows, B, types, ncp, h_list, h_list + pic_cap, (m2v_decode_stat *)(e->h_dec + rec_off), h_conceal);
        R = *h_rec;
        if (conceal && R.status == M2V_DEC_OK)                         // (it came with the record: one wait)
            e->dec_conceal = m2v_decode_conceal{(uint64_t)h_conceal[1] << 32 | h_conceal[0], h_conceal[2], h_conceal[3], h_conceal[4], h_conceal[5], {0, 0}};
        if (R.status == M2V_DEC_SYNTAX) e->dec_join = m2v_decode_join{0, n, 0, 0, {0, 0}};      // a slice refused the stream
        return M2V_OK;
    }
    if (extended) {                                                    // m2v_decode_x.hip; the macroblock rows and the slices in front of every picture are the plan's
        const size_t rows = *(const uint32_t *)(e->h_dec + rec_off + 96);
        if (!e->decode_batch) B = std::min(np, std::max<size_t>(1, std::min(kDecBatchMax, kDecLevelBytes / (mbw * rows * 768))));
        auto *h_list = (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3));
        dec_x_chunks(e, s, a->es, n, a->dst, a->layout, R, rows, B, types, mb_tools, h_list, h_list + pic_cap, (m2v_decode_stat *)(e->h_dec + rec_off));
        R = *h_rec;
        return M2V_OK;
    }
    if (interlaced) {                                                  // m2v_decode_i.hip; the macroblock rows are the plan's (behind the record), not the height's
        const size_t rows = *(const uint32_t *)(e->h_dec + rec_off + 96);
        if (!e->decode_batch) B = std::min(np, std::max<size_t>(1, std::min(kDecBatchMax, kDecLevelBytes / (mbw * rows * 768))));
        dec_i_chunks(e, s, a->es, n, a->dst, a->layout, R, rows, B, types, (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3)), (m2v_decode_stat *)(e->h_dec + rec_off));
        R = *h_rec;
        return M2V_OK;
    }
    if (b_pictures) {                                                 // chunks of B pictures each, scheduled and run by m2v_decode_b.hip
        dec_b_chunks(e, s, a->es, n, a->dst, a->layout, R, B, types, (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3)), (m2v_decode_stat *)(e->h_dec + rec_off));
        R = *h_rec;
        return M2V_OK;
    }
    e->d_dec_mb.ensure(B * mbs * sizeof(dec::MbRec));
    e->d_dec_dc.ensure(B * mbs * 6);
    e->d_dec_lv.ensure(B * mbs * 384);
    e->d_dec_buf.ensure((B + 1) * psz);
    e->d_dec_list.ensure(np);
    // every chunk's pictures ordered by their step inside the chunk: a chain starts at its I picture, or at the chunk's first picture
    auto *h_list = (uint32_t *)(e->h_dec + rec_off + 128 + ((pic_cap + 3) & ~(size_t)3));
    struct Launch { size_t off, count; };
    std::vector<std::vector<Launch>> steps;
    for (size_t p0 = 0; p0 < np; p0 += B) {
        const size_t nb = std::min(B, np - p0);
        std::vector<uint32_t> step(nb);
        size_t deepest = 0;
        for (size_t k = 0; k < nb; ++k) { step[k] = k && types[p0 + k] != 1 ? step[k - 1] + 1 : 0; deepest = std::max<size_t>(deepest, step[k]); }
        std::vector<Launch> ls;
        size_t at = p0;
        for (size_t j = 0; j <= deepest; ++j) {
            const size_t first = at;
            for (size_t k = 0; k < nb; ++k) if (step[k] == j) h_list[at++] = (uint32_t)(p0 + k);
            ls.push_back(Launch{first, at - first});
        }
        steps.push_back(ls);
    }
    auto *d_st = (DecState *)e->d_dec_st.p;
    auto *d_mb = (dec::MbRec *)e->d_dec_mb.p;
    HIPCHK(hipMemcpyAsync(e->d_dec_list.p, h_list, np * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    for (size_t p0 = 0, c = 0; p0 < np; p0 += B, ++c) {
        const size_t nb = std::min(B, np - p0);
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, nb * mbs * 768, s));
        if (main_syntax) {
            dec_main_slices(s, (unsigned)((nb * mbh + 63) / 64), a->es, n, e->d_dec_ev.p, d_st, (const DecPic *)e->d_dec_pics.p, e->d_dec_main.p, (uint32_t)p0,
                            (uint32_t)nb, d_mb, e->d_dec_dc.p, e->d_dec_lv.p);
        } else {
            k_dec_slices<<<(unsigned)((nb * mbh + 63) / 64), 64, 0, s>>>(a->es, n, e->d_dec_ev.p, d_st, (const DecPic *)e->d_dec_pics.p, (uint32_t)p0, (uint32_t)nb,
                                                                         a->mode, d_mb, e->d_dec_dc.p, e->d_dec_lv.p);
            HIPCHK(hipGetLastError());
        }
        k_dec_judge<<<1, 1, 0, s>>>(d_st);
        HIPCHK(hipGetLastError());
        for (const Launch &l : steps[c]) {
            if (main_syntax) {
                dec_main_recon(s, (unsigned)mbs, (unsigned)l.count, d_st, e->d_dec_list.p + l.off, (uint32_t)p0, e->d_dec_main.p, d_mb, e->d_dec_dc.p, e->d_dec_lv.p,
                               e->d_dec_buf.p, psz);
                continue;
            }
            k_dec_recon<<<dim3((unsigned)mbs, (unsigned)l.count), 64, 0, s>>>(d_st, e->d_dec_list.p + l.off, (uint32_t)p0, a->mode, d_mb, e->d_dec_dc.p,
                                                                             e->d_dec_lv.p, e->d_dec_buf.p, psz);
            HIPCHK(hipGetLastError());
        }
        const size_t units = (nb * R.frame_bytes + 15) / 16 + 1;
        k_dec_out<<<(unsigned)std::min<size_t>((units + kDecThreads - 1) / kDecThreads, 8192), kDecThreads, 0, s>>>(d_st, e->d_dec_buf.p, psz, (uint32_t)p0,
                                                                                                                   (uint32_t)nb, a->dst, a->layout);
        HIPCHK(hipGetLastError());
        if (p0 + B < np) HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + nb * psz, psz, hipMemcpyDeviceToDevice, s));      // the next chunk's reference
    }
    k_dec_finish<<<1, 1, 0, s>>>(d_st, (m2v_decode_stat *)(e->h_dec + rec_off));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    R = *h_rec;
    return M2V_OK;
}

extern "C" {

int m2v_decode_scan_tile(void) { return (int)dec::kScanTile; }

int m2v_decode_device(m2v_enc *e, const void *d_es, size_t es_bytes, void *d_dst, size_t cap, int layout, int mode, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    if (!layout420_ok(layout)) { e->set_err("m2v_decode_device: unknown layout %d", layout); return M2V_E_PARAM; }
    if (mode != M2V_DEC_ISO && mode != M2V_DEC_MODULE) { e->set_err("m2v_decode_device: unknown mode %d", mode); return M2V_E_PARAM; }
    if (!d_es && es_bytes) { e->set_err("m2v_decode_device: d_es is NULL"); return M2V_E_PARAM; }
    if (e->decode_conceal && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO || !e->decode_interlaced || !e->decode_extended || !e->decode_mb_tools ||
                              !e->decode_field_pictures)) {
        e->set_err("m2v_decode_device: \"decode_conceal\" = 1 needs \"decode_syntax\" = main, the mode M2V_DEC_ISO and \"decode_interlaced\", "
                   "\"decode_extended\", \"decode_mb_tools\" and \"decode_field_pictures\" = 1");
        return M2V_E_PARAM;
    }
    if (e->decode_join && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO || !e->decode_interlaced || !e->decode_extended || !e->decode_mb_tools ||
                           !e->decode_field_pictures)) {
        e->set_err("m2v_decode_device: \"decode_join\" = 1 .. 3 needs \"decode_syntax\" = main, the mode M2V_DEC_ISO and \"decode_interlaced\", "
                   "\"decode_extended\", \"decode_mb_tools\" and \"decode_field_pictures\" = 1");
        return M2V_E_PARAM;
    }
    if (e->decode_field_pictures && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO || !e->decode_interlaced || !e->decode_extended || !e->decode_mb_tools)) {
        e->set_err("m2v_decode_device: \"decode_field_pictures\" = 1 needs \"decode_syntax\" = main, the mode M2V_DEC_ISO and \"decode_interlaced\", "
                   "\"decode_extended\" and \"decode_mb_tools\" = 1");
        return M2V_E_PARAM;
    }
    if (e->decode_b_pictures && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO)) {
        e->set_err("m2v_decode_device: \"decode_b_pictures\" = 1 needs \"decode_syntax\" = main and the mode M2V_DEC_ISO");
        return M2V_E_PARAM;
    }
    if (e->decode_interlaced && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO)) {
        e->set_err("m2v_decode_device: \"decode_interlaced\" = 1 needs \"decode_syntax\" = main and the mode M2V_DEC_ISO");
        return M2V_E_PARAM;
    }
    if (e->decode_extended && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO)) {
        e->set_err("m2v_decode_device: \"decode_extended\" = 1 needs \"decode_syntax\" = main and the mode M2V_DEC_ISO");
        return M2V_E_PARAM;
    }
    if (e->decode_mb_tools && (e->decode_syntax != M2V_SYNTAX_MAIN || mode != M2V_DEC_ISO || !e->decode_extended)) {
        e->set_err("m2v_decode_device: \"decode_mb_tools\" = 1 needs \"decode_syntax\" = main, the mode M2V_DEC_ISO and \"decode_extended\" = 1");
        return M2V_E_PARAM;
    }
    if (e->decode_syntax == M2V_SYNTAX_MAIN && mode != M2V_DEC_ISO) {
        e->set_err("m2v_decode_device: with \"decode_syntax\" = main the mode is M2V_DEC_ISO (the module's deviations belong to its own syntax)");
        return M2V_E_PARAM;
    }
    if (in_progress(e, "m2v_decode_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    DecodeArgs a{(const uint8_t *)d_es, es_bytes, (uint8_t *)d_dst, cap, layout, mode, (hipStream_t)hip_stream};
    return guard(e, decode_impl, &a);
}

int m2v_decode_report(m2v_enc *e, m2v_decode_stat *out)
{
    if (!e || !out) return M2V_E_PARAM;
    *out = e->dec_rec;
    return M2V_OK;
}

int m2v_decode_join_report(m2v_enc *e, m2v_decode_join *out)
{
    if (!e || !out) return M2V_E_PARAM;
    *out = e->dec_join;
    return M2V_OK;
}

int m2v_decode_conceal_report(m2v_enc *e, m2v_decode_conceal *out)
{
    if (!e || !out) return M2V_E_PARAM;
    *out = e->dec_conceal;
    return M2V_OK;
}

}  // extern "C"
