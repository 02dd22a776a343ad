// m2v_decode_streams.hip — a batch of MPEG-2 I / P streams back to 4:2:0 frames in one call (include/m2v_mi355x.h:
// m2v_decode_streams_device): the pipeline of m2v_decode.hip over a table of streams, of any sizes, each judged alone.  Every function
// that decides a bit or a sample is the one m2v_decode.hip uses (m2v_decode_kernels.hpp); the kernels here are loops of their own over
// them.  The scan, the judge, the finish and the report do not read the syntax: the two main-syntax batch units launch them through
// ds_scan, ds_judge, ds_finish and ds_report (m2v_decode_state.hpp).
//
//   k_ds_scan     the tiles of all streams in one grid; a tile belongs to one stream (found by its number in the streams' table, as
//                 m2v_demux.hip finds a workgroup's container), and its loads are clamped to the segment: a start code in a gap, or one
//                 that straddles a segment's edge, does not exist.  Counts, then - behind k_ds_tiles, one block per stream - the events,
//                 each stream's at its own base.  last_nz is the stream's.
//   k_ds_plan     one block per stream: k_dec_plan's body.  The stream's record and picture types go to pinned memory, its picture
//                 table to its own base.  The host waits once behind it and lays the batch out (dec::plan_streams): output offsets,
//                 which streams do not fit cap, the chunks, every chunk's picture table and step lists - one upload.
//   k_ds_slices   one launch per chunk over every slice of every picture of every stream in the chunk, one slice per lane; the lane
//                 finds its picture in the chunk's table (dec::chunk_slice_pic).  An error lowers the error offset OF ITS STREAM;
//                 k_ds_judge, a lane per stream, turns it into that stream's status, which the later kernels read per picture.  The
//                 slices of a stream that lies in several chunks are walked once more in front of all chunks, without storing (<false>):
//                 a stream refused in its last chunk must not have had its first pictures written.
//   k_ds_recon    step j of every chain of every stream of the chunk, one wavefront per macroblock: a (most macroblocks, pictures) grid,
//                 and a workgroup beyond its picture's macroblocks returns at once - no search per workgroup, and the launch is as wide
//                 as its widest picture whatever the mix.  The reference is the slot of the picture in front in ITS stream (ref_off).
//   k_ds_out      one lane per 16 destination bytes of the chunk's range, one aligned store; a unit that holds a byte outside the range or
//                 of a refused stream's room goes byte by byte for the part that may be written (dec::streams_out_locate).
//   k_ds_finish   every stream's verdict to pinned memory, behind the last chunk.  Two host waits, whatever the number of streams.
#include "m2v_decode_state.hpp"
#include "m2v_decode_streams.hpp"

static_assert(sizeof(m2v_decode_stream_stat) == 88, "the record of include/m2v_mi355x.h is 88 bytes");
static_assert(sizeof(dec::ChunkPic) == 72, "a chunk's picture is 72 bytes");

namespace m2v {

constexpr int kDsThreads = 256;
static_assert(dec::kScanTile == (uint32_t)kDsThreads * 16u, "a tile is one pass of a block");
typedef unsigned long long ull;

struct DsPic { uint32_t ev, type; };

// the stream tile t belongs to: the last one whose first tile is not behind t (a stream without tiles shares its number with the next)
__device__ inline uint32_t ds_stream_of(const DsIn *__restrict__ in, uint32_t n, uint32_t t)
{
    uint32_t a = 0, b = n;
    while (b - a > 1u) { const uint32_t m = (a + b) / 2u; if (in[m].tile0 <= t) a = m; else b = m; }
    return a;
}

template <bool EMIT>
__global__ __launch_bounds__(kDsThreads) void k_ds_scan(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, uint32_t nstreams, uint32_t ntiles,
                                                        DsState *st, uint32_t *__restrict__ tiles, ull *__restrict__ evs)
{
    __shared__ uint32_t s_w[kDsThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t b = ds_stream_of(in, nstreams, t);
        const DsIn S = in[b];
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
        for (uint32_t k = 0; k < (uint32_t)kDsThreads / 64; ++k) { if (k < wave) before += s_w[k]; total += s_w[k]; }
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

// one block per stream: its tiles' counts -> offsets in place; the total is the number of its events
__global__ __launch_bounds__(kDsThreads) void k_ds_tiles(const DsIn *__restrict__ in, uint32_t *tiles_all, DsState *sts)
{
    __shared__ uint32_t s_sum[kDsThreads];
    const DsIn S = in[blockIdx.x];
    DsState *st = sts + blockIdx.x;
    uint32_t *tiles = tiles_all + S.tile0;
    const uint32_t ntiles = S.ntiles, tid = threadIdx.x, per = (ntiles + kDsThreads - 1) / kDsThreads;
    const uint32_t a = min(ntiles, tid * per), b = min(ntiles, a + per);
    uint32_t sum = 0;
    for (uint32_t t = a; t < b; ++t) sum += tiles[t];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kDsThreads; ++k) { const uint32_t v = s_sum[k]; s_sum[k] = run; run += v; }
        st->nev = run;
        if (run > S.ev_cap) st->status = dec::kEvents;
    }
    __syncthreads();
    uint32_t run = s_sum[tid];
    for (uint32_t t = a; t < b; ++t) { const uint32_t v = tiles[t]; tiles[t] = run; run += v; }
}

// one block per stream: k_dec_plan (m2v_decode.hip) with the stream's own segment, events, picture table and record.  Whether the frames
// fit is the host's to say, behind the wait (the rooms depend on the streams in front)
__global__ __launch_bounds__(kDsThreads) void k_ds_plan(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts,
                                                        DsPic *__restrict__ pics_all, uint8_t *h_types_all, m2v_decode_stat *h_recs)
{
    __shared__ dec::Plan s_P;
    __shared__ ull s_bad;
    __shared__ uint32_t s_np[kDsThreads], s_ng[kDsThreads], s_nr[kDsThreads], s_ni[kDsThreads];
    __shared__ int s_last[kDsThreads];
    const DsIn S = in[blockIdx.x];
    DsState *st = sts + blockIdx.x;
    m2v_decode_stat *h_rec = h_recs + blockIdx.x;
    const uint8_t *es = base + S.off;
    const ull *ev = evs + S.ev_base, n = S.n;
    DsPic *pics = pics_all + S.pic_base;
    uint8_t *h_types = h_types_all + S.pic_base;
    const uint32_t pic_cap = S.pic_cap;
    const uint32_t tid = threadIdx.x, nev = st->nev;
    m2v_decode_stat r{};
    r.es_bytes = n;
    if (n < 4) {                                   // not one start code
        if (tid == 0) { st->status = dec::kSyntax; st->err = 0; r.status = dec::kSyntax; *h_rec = r; }
        return;
    }
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
    const ull last_nz = st->last_nz;
    const uint32_t per = (nev + kDsThreads - 1) / kDsThreads, a = min(nev, tid * per), b = min(nev, a + per);
    {
        ull bad = dec::kNone;
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
        for (int k = 0; k < kDsThreads; ++k) {
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
        uint32_t p = s_np[tid];
        int last = s_last[tid];
        for (uint32_t i = a; i < b; ++i) {
            if (dec::ev_code(ev[i]) != 0x00) continue;
            const ull pos = dec::ev_pos(ev[i]);
            const uint32_t type = pos + 5 < n ? (es[pos + 5] >> 3) & 7u : 0u;
            if (type == 1) last = (int)p;
            if (last < 0) atomicMin(&s_bad, pos);                      // a P picture without a reference
            if (p < pic_cap) { pics[p] = DsPic{i, type}; h_types[p] = (uint8_t)type; }
            ++p;
        }
    }
    __syncthreads();
    if (tid) return;
    r.width = P.seq.width; r.height = P.seq.height;
    r.frame_bytes = dec::frame_bytes(P.seq.width, P.seq.height);
    if (s_bad != dec::kNone) { r.status = dec::kSyntax; r.err_offset = s_bad; }
    else if (r.pictures > pic_cap) { r.status = dec::kSyntax; r.err_offset = 0; }      // (cannot happen: a picture is three events at least)
    st->status = r.status; st->err = s_bad; st->mbw = P.mbw; st->mbh = P.mbh;
    *h_rec = r;
}

struct DsSink {
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
struct DsNoSink {
    M2V_HD void mb(int, const dec::MbRec &, const int32_t (&)[6]) {}
    M2V_HD void level(int, int, uint32_t, int32_t) {}
};

// the nslices slices of the table's pictures, one per lane.  Only lowers its stream's err, which no lane of the launch reads: every
// slice is walked whatever the others find, so a stream's minimum is over all of its slices.  STORE false: for the verdict alone
template <bool STORE>
__global__ __launch_bounds__(64) void k_ds_slices(const uint8_t *__restrict__ base, const DsIn *__restrict__ in, const ull *__restrict__ evs, DsState *sts,
                                                  const DsPic *__restrict__ pics, const dec::ChunkPic *__restrict__ tab, uint32_t ntab, uint32_t nslices,
                                                  int mode, dec::MbRec *mb, int32_t *dc, int16_t *lv)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= nslices) return;
    const dec::ChunkPic C = tab[dec::chunk_slice_pic(tab, ntab, g)];
    DsState *st = sts + C.stream;
    if (st->status != dec::kOk) return;
    const DsIn S = in[C.stream];
    const uint32_t row = g - C.slice0, nev = st->nev;
    const uint32_t i = pics[S.pic_base + C.pic].ev + 2u + row;
    if (i >= nev) return;                                              // (the plan accepted the picture: its slices are there)
    const ull *ev = evs + S.ev_base;
    const ull start = dec::ev_pos(ev[i]), end = i + 1 < nev ? dec::ev_pos(ev[i + 1]) : S.n;
    bool ok;
    if (STORE) {
        const size_t first = (size_t)C.mb_base + (size_t)row * C.mbw;
        DsSink sink{mb + first, dc + first * 6, lv + first * 384};
        ok = dec::parse_slice(base + S.off, start, end, C.type, (int)C.mbw, (int)C.mbh, (int)row, mode, sink);
    } else {
        DsNoSink sink;
        ok = dec::parse_slice(base + S.off, start, end, C.type, (int)C.mbw, (int)C.mbh, (int)row, mode, sink);
    }
    if (!ok) atomicMin(&st->err, start);
}

// behind a walk, one lane per stream: what its slices found becomes the status every later kernel of the call reads
__global__ void k_ds_judge(DsState *sts, uint32_t n)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n && sts[b].status == dec::kOk && sts[b].err != dec::kNone) sts[b].status = dec::kSyntax;
}

// grid = (the most macroblocks of a picture of the step, pictures of the step); list: their entries of the chunk's table
__global__ __launch_bounds__(64) void k_ds_recon(const DsState *__restrict__ sts, const dec::ChunkPic *__restrict__ tab, const uint32_t *__restrict__ list, int mode,
                                                 const dec::MbRec *__restrict__ mb, const int32_t *__restrict__ dc, const int16_t *__restrict__ lv, uint8_t *buf)
{
    __shared__ int32_t F[6][64];
    const dec::ChunkPic C = tab[list[blockIdx.y]];
    const uint32_t mbw = C.mbw, mbh = C.mbh, k = blockIdx.x, l = threadIdx.x;
    if (k >= mbw * mbh) return;                                        // (a smaller picture of the step; the whole workgroup leaves)
    if (sts[C.stream].status != dec::kOk) return;
    const uint32_t W = 16u * mbw, H = 16u * mbh, CW = W / 2u;
    const size_t at = (size_t)C.mb_base + k;
    const dec::MbRec m = mb[at];
    const uint32_t col = k % mbw, row = k / mbw;
    uint8_t *cur = buf + C.buf_off;
    const uint8_t *ref = buf + C.ref_off;
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

typedef uint32_t ds_store_t __attribute__((ext_vector_type(4)));

// bytes [lo, hi) of the output: the frames of the table's pictures, one behind the other.  A byte is written iff its picture's stream
// is OK; a 16-byte unit of the destination whose bytes may all be written is one aligned store
__global__ __launch_bounds__(kDsThreads) void k_ds_out(const DsState *__restrict__ sts, const dec::ChunkPic *__restrict__ tab, uint32_t ntab,
                                                       const uint8_t *__restrict__ buf, ull lo, ull hi, uint8_t *__restrict__ dst, int layout)
{
    const ull lead = (ull)(uintptr_t)dst & 15ull;
    const ull u0 = (lo + lead) >> 4, u1 = (hi + lead + 15ull) >> 4;
    for (ull g = u0 + (ull)blockIdx.x * kDsThreads + threadIdx.x; g < u1; g += (ull)gridDim.x * kDsThreads) {
        const long long o0 = (long long)(g << 4) - (long long)lead;
        const int k0 = o0 < (long long)lo ? (int)((long long)lo - o0) : 0, k1 = (long long)hi - o0 < 16 ? (int)((long long)hi - o0) : 16;
        if (k0 >= k1) continue;
        const dec::OutByte first = dec::streams_out_locate(tab, ntab, (ull)(o0 + k0), layout);
        uint32_t idx = first.pic, q = first.q;
        dec::OutAt at = first.at;
        dec::ChunkPic C = tab[idx];
        bool ok = sts[C.stream].status == dec::kOk;
        uint32_t v[4] = {0, 0, 0, 0}, mask = 0;
        for (int k = k0; k < k1; ++k) {
            if (ok) {
                v[k >> 2] |= (uint32_t)dec::pic_sample(buf + C.buf_off, 16u * C.mbw, 16u * C.mbh, at) << (8 * (k & 3));
                mask |= 1u << k;
            }
            if (k + 1 == k1) break;
            if (++q == (uint32_t)C.fb) {                               // the next frame: of this stream, or the first of the next (idx + 1 < ntab: o < hi)
                C = tab[++idx]; q = 0;
                ok = sts[C.stream].status == dec::kOk;
                at = dec::out_locate(0, C.w, C.h, layout);
            }
            else if (at.run > 1) dec::out_step(at, layout);
            else at = dec::out_locate(q, C.w, C.h, layout);
        }
        if (mask == 0xFFFFu) {
            *(__attribute__((address_space(1))) ds_store_t *)(dst + o0) = ds_store_t{v[0], v[1], v[2], v[3]};
        } else {
            for (int k = k0; k < k1; ++k) if ((mask >> k) & 1u) dst[o0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

__global__ void k_ds_finish(const DsState *sts, uint32_t n, DsVerdict *h_v)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) h_v[b] = DsVerdict{sts[b].err, sts[b].status, 0};
}

void ds_scan(hipStream_t s, const uint8_t *es, const DsIn *d_in, size_t n, size_t tiles, DsState *d_st, uint32_t *d_tiles, ull *d_ev)
{
    if (!tiles) return;
    const unsigned gx = (unsigned)std::min<size_t>(tiles, 4096);
    k_ds_scan<false><<<gx, kDsThreads, 0, s>>>(es, d_in, (uint32_t)n, (uint32_t)tiles, d_st, d_tiles, d_ev);
    HIPCHK(hipGetLastError());
    k_ds_tiles<<<(unsigned)n, kDsThreads, 0, s>>>(d_in, d_tiles, d_st);
    HIPCHK(hipGetLastError());
    k_ds_scan<true><<<gx, kDsThreads, 0, s>>>(es, d_in, (uint32_t)n, (uint32_t)tiles, d_st, d_tiles, d_ev);
    HIPCHK(hipGetLastError());
}

void ds_judge(hipStream_t s, DsState *d_st, size_t n)
{
    k_ds_judge<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(d_st, (uint32_t)n);
    HIPCHK(hipGetLastError());
}

void ds_finish(hipStream_t s, const DsState *d_st, size_t n, DsVerdict *h_v)
{
    k_ds_finish<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(d_st, (uint32_t)n, h_v);
    HIPCHK(hipGetLastError());
}

void ds_report(m2v_enc *e, const uint64_t *off, size_t n, const std::vector<uint64_t> &out_offset, const std::vector<uint8_t> &overflow,
               const std::vector<m2v_decode_stat> &rec, const DsVerdict *v)
{
    for (size_t b = 0; b < n; ++b) {
        m2v_decode_stream_stat r{off[b], out_offset[b], rec[b]};
        if (r.rec.status == M2V_DEC_OK) {
            if (overflow[b]) r.rec.status = M2V_DEC_OVERFLOW;
            else if (v && v[b].status != dec::kOk) { r.rec.status = v[b].status; r.rec.err_offset = v[b].err; }
            else r.rec.out_bytes = r.rec.frame_bytes * r.rec.pictures;
        }
        e->ds_q.push(&r, &r + 1);
    }
}

void ds_release(m2v_enc *e)
{
    e->d_ds_in.release(); e->d_ds_tab.release();
    if (e->h_ds) (void)hipHostFree(e->h_ds);
    if (e->h_ds_tab) (void)hipHostFree(e->h_ds_tab);
    e->h_ds = e->h_ds_tab = nullptr; e->h_ds_cap = e->h_ds_tab_cap = 0;
}

}  // namespace m2v

struct DecodeStreamsArgs { const uint8_t *es; const uint64_t *off, *bytes; size_t n; uint8_t *dst; size_t cap; int layout, mode; hipStream_t s; };

static int decode_streams_impl(m2v_enc *e, void *argp)
{
    auto *a = (DecodeStreamsArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    const size_t n = a->n;
    e->ds_q.clear();
    // the work buffers are m2v_decode_device's (both calls block; no recorded graph references them), and two tables of this unit's own
    e->d_dec_st.recorded = e->d_dec_ev.recorded = e->d_dec_pics.recorded = e->d_dec_mb.recorded = e->d_dec_dc.recorded = false;
    e->d_dec_lv.recorded = e->d_dec_buf.recorded = e->d_dec_tiles.recorded = e->d_dec_list.recorded = false;
    e->d_ds_in.recorded = e->d_ds_tab.recorded = false;
    std::vector<size_t> ev_cap(n);
    for (size_t b = 0; b < n; ++b) ev_cap[b] = std::max<size_t>(256, a->bytes[b] / 16 + 64);      // a guess per stream: a second run takes the counts of the first
    std::vector<m2v_decode_stat> rec(n);
    std::vector<uint8_t> types;
    std::vector<size_t> pic_base(n);
    timer_break(e);
    for (int run = 0; run < 2; ++run) {
        size_t tiles = 0, evs = 0, pics = 0;
        const size_t in_bytes = ds_up64(n * sizeof(DsIn)), st_bytes = ds_up64(n * sizeof(DsState)), rec_bytes = ds_up64(n * sizeof(m2v_decode_stat));
        for (size_t b = 0; b < n; ++b) pics += ev_cap[b] / 3 + 2;
        ensure_pinned(e->h_ds, e->h_ds_cap, in_bytes + st_bytes + rec_bytes + pics + 64);
        auto *h_in = (DsIn *)e->h_ds;
        auto *h_st = (DsState *)(e->h_ds + in_bytes);
        auto *h_rec = (m2v_decode_stat *)(e->h_ds + in_bytes + st_bytes);
        uint8_t *h_types = e->h_ds + in_bytes + st_bytes + rec_bytes;
        pics = 0;
        for (size_t b = 0; b < n; ++b) {
            const size_t nb = a->bytes[b], nt = nb < 4 ? 0 : (nb + dec::kScanTile - 1) / dec::kScanTile;
            if (ev_cap[b] > 0x7FFFFFFFu) { e->set_err("m2v_decode_streams_device: stream %zu holds more than 2^31 start codes", b); return M2V_E_PARAM; }
            if (tiles + nt > 0x7FFFFFFFu) { e->set_err("m2v_decode_streams_device: the streams are longer than 2^31 scan tiles"); return M2V_E_PARAM; }
            const size_t pic_cap = ev_cap[b] / 3 + 2;
            h_in[b] = DsIn{a->off[b], nb, evs, pics, (uint32_t)tiles, (uint32_t)nt, (uint32_t)ev_cap[b], (uint32_t)pic_cap};
            h_st[b] = DsState{dec::kNone, 0, 0, dec::kOk, 0, 0};
            pic_base[b] = pics;
            tiles += nt; evs += ev_cap[b]; pics += pic_cap;
        }
        e->d_ds_in.ensure(in_bytes);
        e->d_dec_st.ensure(st_bytes);
        e->d_dec_tiles.ensure(std::max<size_t>(tiles, 1));
        e->d_dec_ev.ensure(evs);
        e->d_dec_pics.ensure(pics * sizeof(DsPic));
        auto *d_in = (const DsIn *)e->d_ds_in.p;
        auto *d_st = (DsState *)e->d_dec_st.p;
        HIPCHK(hipMemcpyAsync(e->d_ds_in.p, h_in, in_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_st, h_st, st_bytes, hipMemcpyHostToDevice, s));
        ds_scan(s, a->es, d_in, n, tiles, d_st, e->d_dec_tiles.p, e->d_dec_ev.p);
        k_ds_plan<<<(unsigned)n, kDsThreads, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, (DsPic *)e->d_dec_pics.p, h_types, h_rec);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                              // the call's one wait for the plan: every stream's pictures, size, types
        bool again = false;
        for (size_t b = 0; b < n; ++b) {
            rec[b] = h_rec[b];
            if (rec[b].status == dec::kEvents) { again = true; ev_cap[b] = rec[b].pictures; }      // (the count of events travels there)
        }
        types.assign(h_types, h_types + pics);
        if (!again) break;
    }
    std::vector<dec::StreamInfo> info(n);
    for (size_t b = 0; b < n; ++b) {
        if (rec[b].status == dec::kEvents) { const uint64_t nb = rec[b].es_bytes; rec[b] = m2v_decode_stat{}; rec[b].es_bytes = nb; rec[b].status = M2V_DEC_SYNTAX; }
        info[b] = dec::StreamInfo{rec[b].status, rec[b].pictures, rec[b].width, rec[b].height, types.data() + pic_base[b]};
    }
    const dec::StreamsPlan P = dec::plan_streams(info.data(), n, a->cap, a->dst == nullptr, e->decode_batch);
    if (!a->dst || P.pics.empty()) { ds_report(e, a->off, n, P.out_offset, P.overflow, rec, nullptr); return M2V_OK; }
    // the tables: every chunk's pictures, the cut streams' pictures, the step lists; the verdicts come back behind them
    const size_t tab_bytes = ds_up64(P.pics.size() * sizeof(dec::ChunkPic)), pre_bytes = ds_up64(P.pre.size() * sizeof(dec::ChunkPic)),
                 list_bytes = ds_up64(P.list.size() * sizeof(uint32_t));
    ensure_pinned(e->h_ds_tab, e->h_ds_tab_cap, tab_bytes + pre_bytes + list_bytes + n * sizeof(DsVerdict) + 64);
    memcpy(e->h_ds_tab, P.pics.data(), P.pics.size() * sizeof(dec::ChunkPic));
    if (!P.pre.empty()) memcpy(e->h_ds_tab + tab_bytes, P.pre.data(), P.pre.size() * sizeof(dec::ChunkPic));
    memcpy(e->h_ds_tab + tab_bytes + pre_bytes, P.list.data(), P.list.size() * sizeof(uint32_t));
    auto *h_v = (DsVerdict *)(e->h_ds_tab + tab_bytes + pre_bytes + list_bytes);
    e->d_ds_tab.ensure(tab_bytes + pre_bytes + list_bytes);
    HIPCHK(hipMemcpyAsync(e->d_ds_tab.p, e->h_ds_tab, tab_bytes + pre_bytes + list_bytes, hipMemcpyHostToDevice, s));
    uint64_t most_mbs = 0, most_buf = 0;
    for (const dec::StreamsChunk &C : P.chunks) { most_mbs = std::max(most_mbs, C.mbs); most_buf = std::max(most_buf, C.buf_bytes); }
    e->d_dec_mb.ensure(most_mbs * sizeof(dec::MbRec));
    e->d_dec_dc.ensure(most_mbs * 6);
    e->d_dec_lv.ensure(most_mbs * 384);
    e->d_dec_buf.ensure(most_buf);
    auto *d_in = (const DsIn *)e->d_ds_in.p;
    auto *d_st = (DsState *)e->d_dec_st.p;
    auto *d_mb = (dec::MbRec *)e->d_dec_mb.p;
    auto *d_pics = (const DsPic *)e->d_dec_pics.p;
    auto *d_tab = (const dec::ChunkPic *)e->d_ds_tab.p;
    auto *d_pre = (const dec::ChunkPic *)(e->d_ds_tab.p + tab_bytes);
    auto *d_list = (const uint32_t *)(e->d_ds_tab.p + tab_bytes + pre_bytes);
    if (P.pre_slices) {
        k_ds_slices<false><<<(P.pre_slices + 63u) / 64u, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, d_pre, (uint32_t)P.pre.size(), P.pre_slices, a->mode,
                                                                   nullptr, nullptr, nullptr);
        HIPCHK(hipGetLastError());
        ds_judge(s, d_st, n);
    }
    for (const dec::StreamsChunk &C : P.chunks) {
        const dec::ChunkPic *tab = d_tab + C.first;
        HIPCHK(hipMemsetAsync(e->d_dec_lv.p, 0, C.mbs * 768, s));
        k_ds_slices<true><<<(C.slices + 63u) / 64u, 64, 0, s>>>(a->es, d_in, e->d_dec_ev.p, d_st, d_pics, tab, (uint32_t)C.count, C.slices, a->mode, d_mb,
                                                              e->d_dec_dc.p, e->d_dec_lv.p);
        HIPCHK(hipGetLastError());
        ds_judge(s, d_st, n);
        for (const dec::StreamsChunk::Step &S : C.steps) {
            for (size_t y = 0; y < S.count; y += 65535) {             // (a grid's second dimension ends there)
                k_ds_recon<<<dim3(S.most_mbs, (unsigned)std::min<size_t>(S.count - y, 65535)), 64, 0, s>>>(d_st, tab, d_list + S.off + y, a->mode, d_mb, e->d_dec_dc.p,
                                                                                                         e->d_dec_lv.p, e->d_dec_buf.p);
                HIPCHK(hipGetLastError());
            }
        }
        const size_t units = (size_t)((C.hi - C.lo + 15) / 16 + 1);
        k_ds_out<<<(unsigned)std::min<size_t>((units + kDsThreads - 1) / kDsThreads, 8192), kDsThreads, 0, s>>>(d_st, tab, (uint32_t)C.count, e->d_dec_buf.p, C.lo,
                                                                                                              C.hi, a->dst, a->layout);
        HIPCHK(hipGetLastError());
        if (C.carry_out) {                                            // the next chunk's reference (the carried slot is as large as the largest picture: no overlap)
            const dec::ChunkPic &L = P.pics[C.first + C.count - 1];
            HIPCHK(hipMemcpyAsync(e->d_dec_buf.p, e->d_dec_buf.p + L.buf_off, (size_t)L.mbw * L.mbh * 384, hipMemcpyDeviceToDevice, s));
        }
    }
    ds_finish(s, d_st, n, h_v);
    HIPCHK(hipStreamSynchronize(s));
    ds_report(e, a->off, n, P.out_offset, P.overflow, rec, h_v);
    return M2V_OK;
}

extern "C" {

int m2v_decode_streams_device(m2v_enc *e, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams, void *d_dst, size_t cap,
                              int layout, int mode, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    if (nstreams < 1 || nstreams > 65535) { e->set_err("m2v_decode_streams_device: nstreams is 1 .. 65535, not %zu", nstreams); return M2V_E_PARAM; }
    if (!es_off || !es_bytes) { e->set_err("m2v_decode_streams_device: es_off / es_bytes is NULL"); return M2V_E_PARAM; }
    if (!layout420_ok(layout)) { e->set_err("m2v_decode_streams_device: unknown layout %d", layout); return M2V_E_PARAM; }
    if (mode != M2V_DEC_ISO && mode != M2V_DEC_MODULE) { e->set_err("m2v_decode_streams_device: unknown mode %d", mode); return M2V_E_PARAM; }
    if (!d_es) for (size_t b = 0; b < nstreams; ++b) if (es_bytes[b]) { e->set_err("m2v_decode_streams_device: d_es is NULL"); return M2V_E_PARAM; }
    if (e->decode_syntax == M2V_SYNTAX_MAIN) {                   // (the batch entry of the main syntax is a follow-up: nothing is touched)
        e->set_err("m2v_decode_streams_device: \"decode_syntax\" = main is m2v_decode_device's only; set it back to 0 for this entry");
        return M2V_E_STATE;
    }
    if (in_progress(e, "m2v_decode_streams_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    DecodeStreamsArgs a{(const uint8_t *)d_es, es_off, es_bytes, nstreams, (uint8_t *)d_dst, cap, layout, mode, (hipStream_t)hip_stream};
    return guard(e, decode_streams_impl, &a);
}

int m2v_decode_streams_report(m2v_enc *e, m2v_decode_stream_stat *out, size_t max)
{
    if (!e) return M2V_E_PARAM;
    return e->ds_q.pop31(out, max);
}

}  // extern "C"
