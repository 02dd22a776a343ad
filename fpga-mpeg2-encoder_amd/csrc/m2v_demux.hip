// m2v_demux.hip — transport and program streams in device memory back to the elementary stream (include/m2v_mi355x.h: m2v_demux_device):
// the inverse of m2v_mux.hip, so that a container - our muxer's, a batch entry, an archived .ts / .mpg - reaches m2v_decode_device without a
// trip to the host.  The bytes, the stamps and every field of the records are those of m2vc_demux_ts / m2vc_demux_ps exactly
// (m2v_container.cpp is the specification; m2v_demux_kernels.hpp holds every function that decides a byte, an offset or a verdict, and
// compiles for the host too).
//
//   k_ts_find     one block per transport stream: the length's verdict and, with stream = -1, discovery - the first PAT packet, then the
//                 first PMT packet, each a first-occurrence minimum over 256 packets at a time; one lane parses the section (its CRC is
//                 at most 184 bytes).
//   k_ts_tiles    all blocks, 1024 packets per tile, four per lane: classify() every packet - PID, payload place and length, flags,
//                 the rule it breaks - and reduce the tile's sums; a broken rule travels as a minimum (atomicMin: the verdict does not
//                 depend on scheduling).  Elementary bytes in front of the first PES start do not count: a tile keeps its sums on both
//                 sides of its own first start, so the plan needs no second pass.
//   k_ps_walk     one LANE per program stream: the chain is serial by definition (the payload may emulate any start code, so a unit is
//                 one only when the chain reaches it).  It writes the table itself.  A first version: see DESIGN.md for what a parallel
//                 one would take.
//   k_demux_plan  one block per container: a serial prefix over the tiles (a few additions per 1024 packets), the verdict; the block that
//                 finishes last places the streams one behind the other (each on a 32-byte boundary), judges them against cap, gives
//                 each its first stamp and writes the records, to the device and straight into pinned memory.
//   k_demux_table all blocks: classify() again, a block-wide exclusive scan of lengths and PES starts, one table entry per packet and the
//                 stamps (PS: the stamps of the walk's table).
//   k_demux_write grid-stride, one lane per 16 output bytes at a 16-byte boundary of the destination: binary search of the table,
//                 unaligned loads, aligned 16-byte stores; the first and last unit of a stream go byte by byte.
//
// Nothing of the encoder, the muxer or the decoder is touched, and with the entry not called nothing here is reached.
#include "m2v_host.hpp"
#include "m2v_demux_kernels.hpp"

static_assert(sizeof(m2v_demux_stat) == 64, "the record of include/m2v_mi355x.h is 64 bytes");
static_assert(sizeof(m2v_demux_stamp) == 32 && sizeof(demux::Stamp) == 32, "a stamp is 32 bytes");
static_assert(sizeof(demux::Seg) == 16 && sizeof(demux::Tile) == 56, "table entry and tile");
static_assert(M2V_MUX_TS == demux::kTs && M2V_MUX_PS == demux::kPs && M2V_DEMUX_SYNTAX == demux::kSyntax && M2V_DEMUX_OVERFLOW == demux::kOverflow &&
              M2V_DEMUX_NOSTREAM == demux::kNoStream, "m2v_demux_kernels.hpp repeats the values of include/m2v_mi355x.h");

namespace m2v {

constexpr int kDmxThreads = 256;
static_assert(demux::kTilePackets == 4 * kDmxThreads, "a tile is four packets per lane");

struct DmxHead { unsigned long long total_units; uint32_t ticket, pad; unsigned long long reserved[6]; };      // 64 bytes in front of the containers

typedef unsigned long long ull;

__device__ __forceinline__ ull wave_min(ull v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) { const ull o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the first packet of `pid` that starts a section, 256 packets at a time; every lane of the block calls it and gets the answer
__device__ ull find_psi(const uint8_t *src, ull np, uint32_t pid, ull *s_first)
{
    for (ull base = 0; base < np; base += kDmxThreads) {
        if (threadIdx.x == 0) *s_first = demux::kNone;
        __syncthreads();
        const ull k = base + threadIdx.x;
        if (k < np && demux::psi_match(src + 188 * k, pid)) atomicMin(s_first, k);
        __syncthreads();
        const ull f = *s_first;
        __syncthreads();
        if (f != demux::kNone) return f;
    }
    return demux::kNone;
}

__global__ __launch_bounds__(kDmxThreads) void k_ts_find(demux::State *st, const uint8_t *__restrict__ d_src)
{
    __shared__ ull s_first;
    __shared__ uint32_t s_pid, s_program;
    __shared__ int s_v;
    demux::State *S = st + blockIdx.x;
    const uint8_t *src = d_src + S->src_off;
    const ull n = S->src_bytes, np = n / 188;
    const int want = S->want;
    ull err = demux::ts_length_err(n);
    if (want < 0) {
        ull k = find_psi(src, np, 0, &s_first);
        if (threadIdx.x == 0) {
            uint32_t program = 0, pmt = 0;
            s_v = k == demux::kNone ? (int)demux::kNoStream : demux::pat_parse(src + 188 * k, program, pmt);
            if (s_v == demux::kSyntax && 188 * k < err) err = 188 * k;
            s_pid = pmt; s_program = program;
        }
        __syncthreads();
        if (s_v == demux::kOk) {
            k = find_psi(src, np, s_pid, &s_first);
            if (threadIdx.x == 0) {
                uint32_t video = 0;
                s_v = k == demux::kNone ? (int)demux::kNoStream : demux::pmt_parse(src + 188 * k, s_program, video);
                if (s_v == demux::kSyntax && 188 * k < err) err = 188 * k;
                s_pid = video;
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        S->found = want < 0 ? s_v : (int)demux::kOk;
        S->pid = want >= 0 ? (uint32_t)want : s_v == demux::kOk ? s_pid : demux::kNoPid;
        if (err != demux::kNone) atomicMin((ull *)&S->err, err);
    }
}

__global__ __launch_bounds__(kDmxThreads) void k_ts_tiles(demux::State *st, const uint8_t *__restrict__ d_src, demux::Tile *__restrict__ tiles)
{
    __shared__ uint8_t s_cc[demux::kTilePackets];           // 0x80 | discontinuity_indicator << 4 | counter of a packet with a payload, else 0
    __shared__ uint32_t s_sum[6], s_firstw, s_lastw;
    __shared__ ull s_fp, s_err;
    demux::State *S = st + blockIdx.y;
    const uint8_t *src = d_src + S->src_off;
    const ull np = S->src_bytes / 188;
    const uint32_t pid = S->pid, ntiles = S->ntiles, tid = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        if (tid < 6) s_sum[tid] = 0;
        if (tid == 0) { s_firstw = ~0u; s_lastw = 0; s_fp = demux::kNone; s_err = demux::kNone; }
        __syncthreads();
        demux::Pkt k[4];
        ull err = demux::kNone, fp = demux::kNone;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t idx = tid * 4 + j;
            const ull packet = (ull)t * demux::kTilePackets + idx;
            k[j] = demux::Pkt{188, 0, 0, 0};
            if (packet < np) k[j] = demux::classify(src + 188 * packet, pid);
            s_cc[idx] = k[j].flags & demux::kPayload ? (uint8_t)(0x80u | (demux::cc_word(0, k[j]) & 31u)) : (uint8_t)0;
            if ((k[j].flags & (demux::kBadSync | demux::kViol)) && err == demux::kNone) err = 188 * packet;
            if ((k[j].flags & demux::kPusi) && fp == demux::kNone) fp = packet;
        }
        err = wave_min(err); fp = wave_min(fp);
        if ((tid & 63) == 0) {
            if (err != demux::kNone) atomicMin(&s_err, err);
            if (fp != demux::kNone) atomicMin(&s_fp, fp);
        }
        __syncthreads();
        fp = s_fp;
        uint32_t v[6] = {0, 0, 0, 0, 0, 0};               // bytes, bytes_pre, video, video_pre, pes, disc
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t idx = tid * 4 + j;
            const ull packet = (ull)t * demux::kTilePackets + idx;
            if (!(k[j].flags & demux::kVideo)) continue;
            v[0] += k[j].len; ++v[2];
            if (packet < fp) { v[1] += k[j].len; ++v[3]; }
            if (k[j].flags & demux::kPusi) ++v[4];
            if (k[j].flags & demux::kPayload) {
                const uint32_t w = demux::cc_word(idx, k[j]);
                int x = (int)idx - 1;
                while (x >= 0 && !(s_cc[x] & 0x80)) --x;      // the packet with a payload in front of this one (usually the very next)
                if (x < 0) s_firstw = w;                      // (one packet of the tile has none)
                else if (demux::cc_breaks(s_cc[x] & 15u, w)) ++v[5];
                atomicMax(&s_lastw, (idx + 1) << 8 | (w & 15u));
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint32_t r = wave_sum(v[i]);
            if ((tid & 63) == 0 && r) atomicAdd(&s_sum[i], r);
        }
        __syncthreads();
        if (tid == 0) {
            demux::Tile T;
            demux::tile_clear(T);
            T.bytes = s_sum[0]; T.bytes_pre = s_sum[1]; T.video = s_sum[2]; T.video_pre = s_sum[3]; T.pes = s_sum[4]; T.disc = s_sum[5];
            T.first = s_firstw; T.last = s_lastw & 15u; T.first_pusi = s_fp;
            tiles[(size_t)S->tile_base + t] = T;
            if (s_err != demux::kNone) atomicMin((ull *)&S->err, s_err);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_ps_walk(demux::State *st, const uint8_t *__restrict__ d_src, demux::Seg *__restrict__ segs, int nstreams)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nstreams) return;
    demux::State L = st[s];
    demux::ps_walk(L, d_src + L.src_off, segs + L.seg_base);
    st[s] = L;
}

template <typename T> __device__ __forceinline__ T dmx_peek(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64) void k_demux_plan(demux::State *st, DmxHead *head, demux::Tile *tiles, demux::Seg *segs, int nstreams, ull cap, ull dst_addr,
                                                    m2v_demux_stat *h_rec)
{
    if (threadIdx.x) return;
    demux::State *S = st + blockIdx.x;
    if (S->kind == demux::kTs) {
        demux::State L = *S;
        demux::ts_plan(L, tiles + L.tile_base);
        if (L.status == demux::kOk) segs[L.seg_base + L.nseg] = demux::Seg{0, L.out_bytes};
        *S = L;
    }
    __threadfence();
    if (atomicAdd(&head->ticket, 1u) != (uint32_t)nstreams - 1u) return;
    __threadfence();
    // the last block: every container's plan is in memory
    demux::Place P;
    for (int b = 0; b < nstreams; ++b) {
        demux::State *B = st + b;
        demux::State L{};
        L.status = dmx_peek(&B->status); L.out_bytes = dmx_peek(&B->out_bytes); L.err = dmx_peek(&B->err); L.pid = dmx_peek(&B->pid);
        L.pes = dmx_peek(&B->pes); L.packets = dmx_peek(&B->packets); L.disc = dmx_peek(&B->disc); L.skipped = dmx_peek(&B->skipped);
        L.nseg = dmx_peek(&B->nseg);
        demux::place(L, P, cap, dst_addr);
        B->status = L.status; B->out_bytes = L.out_bytes; B->err = L.err; B->pid = L.pid; B->pes = L.pes; B->packets = L.packets; B->disc = L.disc;
        B->skipped = L.skipped; B->nseg = L.nseg; B->out_off = L.out_off; B->unit0 = L.unit0; B->stamp0 = L.stamp0;
        h_rec[b] = m2v_demux_stat{B->src_off, B->src_bytes, L.out_off, L.out_bytes, L.err, L.pes, L.packets, L.disc, L.skipped, L.pid, L.status};
    }
    head->total_units = P.units;
    head->ticket = 0;
}

// exclusive prefix of (a, b) over the block's lanes, in lane order; s: 2 * 4 words
__device__ __forceinline__ void block_scan2(uint32_t &a, uint32_t &b, uint32_t *s)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ua = __shfl_up(ia, d), ub = __shfl_up(ib, d);
        if (lane >= (uint32_t)d) { ia += ua; ib += ub; }
    }
    if (lane == 63) { s[wave] = ia; s[4 + wave] = ib; }
    __syncthreads();
    uint32_t ba = 0, bb = 0;
    for (uint32_t w = 0; w < wave; ++w) { ba += s[w]; bb += s[4 + w]; }
    a = ba + ia - a; b = bb + ib - b;
    __syncthreads();
}

__global__ __launch_bounds__(kDmxThreads) void k_demux_table(const demux::State *__restrict__ st, const uint8_t *__restrict__ d_src,
                                                             const demux::Tile *__restrict__ tiles, demux::Seg *__restrict__ segs,
                                                             demux::Stamp *__restrict__ stamps, ull stamp_cap)
{
    __shared__ uint32_t s_scan[8];
    const demux::State *S = st + blockIdx.y;
    if (S->status != demux::kOk) return;
    const uint8_t *src = d_src + S->src_off;
    demux::Seg *mine = segs + S->seg_base;
    const ull stamp0 = S->stamp0;
    if (S->kind == demux::kPs) {
        const ull nseg = S->nseg;
        for (ull g = (ull)blockIdx.x * kDmxThreads + threadIdx.x; g < nseg; g += (ull)gridDim.x * kDmxThreads)
            if (stamp0 + g < stamp_cap) stamps[stamp0 + g] = demux::stamp_of(mine[g], src);
        return;
    }
    const ull np = S->src_bytes / 188, first_pusi = S->first_pusi;
    const uint32_t pid = S->pid, ntiles = S->ntiles, tid = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const demux::Tile &T = tiles[(size_t)S->tile_base + t];
        demux::Pkt k[4];
        uint32_t len[4], a = 0, b = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const ull packet = (ull)t * demux::kTilePackets + tid * 4 + j;
            k[j] = demux::Pkt{188, 0, 0, 0};
            if (packet < np) k[j] = demux::classify(src + 188 * packet, pid);
            len[j] = demux::ts_len(k[j], packet, first_pusi);
            a += len[j];
            b += k[j].flags & demux::kPusi ? 1u : 0u;
        }
        block_scan2(a, b, s_scan);
        ull out = T.out0 + a;
        ull pes = stamp0 + T.pes0 + b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const ull packet = (ull)t * demux::kTilePackets + tid * 4 + j;
            if (packet >= np) break;
            const demux::Seg g = demux::ts_seg(k[j], packet, out);
            mine[packet] = g;
            if (k[j].flags & demux::kPusi) {
                if (pes < stamp_cap) stamps[pes] = demux::stamp_of(g, src);
                ++pes;
            }
            out += len[j];
        }
    }
}

typedef uint32_t dmx_store_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kDmxThreads) void k_demux_write(const demux::State *__restrict__ st, const DmxHead *__restrict__ head, const uint8_t *__restrict__ d_src,
                                                             const demux::Seg *__restrict__ segs, uint8_t *__restrict__ dst, int nstreams)
{
    const ull total = head->total_units;
    for (ull g = (ull)blockIdx.x * kDmxThreads + threadIdx.x; g < total; g += (ull)gridDim.x * kDmxThreads) {
        int lo = 0, hi = nstreams - 1;                       // the last container whose first unit is at or in front of g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (st[mid].unit0 <= g) lo = mid; else hi = mid - 1;
        }
        const demux::State &S = st[lo];
        uint8_t *out = dst + S.out_off;
        const long long q0 = (long long)((g - S.unit0) << 4) - (long long)((uintptr_t)out & 15u);
        const mux::Win w = demux::gather16(segs + S.seg_base, S.nseg, S.out_bytes, d_src + S.src_off, S.src_bytes, q0);
        if (q0 >= 0 && (ull)q0 + 16u <= S.out_bytes) {
            *(__attribute__((address_space(1))) dmx_store_t *)(out + q0) = dmx_store_t{(uint32_t)w.lo, (uint32_t)(w.lo >> 32), (uint32_t)w.hi, (uint32_t)(w.hi >> 32)};
        } else {
            for (int k = 0; k < 16; ++k) {
                const long long q = q0 + k;
                if (q >= 0 && (ull)q < S.out_bytes) out[q] = (uint8_t)((k < 8 ? w.lo : w.hi) >> (8 * (k & 7)));
            }
        }
    }
}

void dmx_release(m2v_enc *e)
{
    e->d_dmx_st.release(); e->d_dmx_tiles.release(); e->d_dmx_seg.release();
    if (e->h_dmx) (void)hipHostFree(e->h_dmx);
    e->h_dmx = nullptr; e->h_dmx_cap = 0;
}

}  // namespace m2v

struct DemuxDeviceArgs { int kind; const uint8_t *d_src; const uint64_t *off, *bytes; size_t n; int stream; uint8_t *dst; size_t cap; void *stamps; size_t stamp_cap; hipStream_t s; };

static int demux_device_impl(m2v_enc *e, void *argp)
{
    auto *a = (DemuxDeviceArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    e->dmx_q.clear();
    const size_t n = a->n;
    const size_t st_bytes = sizeof(DmxHead) + n * sizeof(demux::State), rec_bytes = n * sizeof(m2v_demux_stat);
    ensure_pinned(e->h_dmx, e->h_dmx_cap, st_bytes + rec_bytes + 64);
    memset(e->h_dmx, 0, st_bytes + rec_bytes);
    auto *h_st = (demux::State *)(e->h_dmx + sizeof(DmxHead));
    size_t tiles = 0, segs = 0, most_tiles = 1, longest = 0;
    for (size_t b = 0; b < n; ++b) {
        demux::State &S = h_st[b];
        S.src_off = a->off[b]; S.src_bytes = a->bytes[b];
        S.want = a->stream; S.kind = (uint32_t)a->kind;
        S.err = demux::kNone;
        const size_t np = a->bytes[b] / 188;
        const size_t nt = a->kind == demux::kTs ? (np + demux::kTilePackets - 1) / demux::kTilePackets : 0;
        if (tiles + nt > 0xFFFFFFFFull) { e->set_err("m2v_demux_device: the containers hold more than 2^42 packets"); return M2V_E_PARAM; }
        S.tile_base = (uint32_t)tiles; S.ntiles = (uint32_t)nt;
        S.seg_base = segs;
        S.seg_cap = a->kind == demux::kTs ? np + 1 : a->bytes[b] / 9 + 2;      // (a PES packet of the stream is at least nine bytes)
        tiles += nt; segs += S.seg_cap;
        most_tiles = std::max(most_tiles, nt);
        longest = std::max<size_t>(longest, a->bytes[b]);
    }
    e->d_dmx_st.recorded = e->d_dmx_tiles.recorded = e->d_dmx_seg.recorded = false;
    e->d_dmx_st.ensure(st_bytes);
    e->d_dmx_tiles.ensure(std::max<size_t>(tiles, 1) * sizeof(demux::Tile));
    e->d_dmx_seg.ensure(segs * sizeof(demux::Seg));
    timer_break(e);
    HIPCHK(hipMemcpyAsync(e->d_dmx_st.p, e->h_dmx, st_bytes, hipMemcpyHostToDevice, s));
    auto *d_head = (DmxHead *)e->d_dmx_st.p;
    auto *d_st = (demux::State *)(e->d_dmx_st.p + sizeof(DmxHead));
    auto *d_tiles = (demux::Tile *)e->d_dmx_tiles.p;
    auto *d_seg = (demux::Seg *)e->d_dmx_seg.p;
    auto *h_rec = (m2v_demux_stat *)(e->h_dmx + st_bytes);
    // every kernel over packets, table entries or output units strides its grid: the most workgroups of a launch is a choice (option
    // "demux_blocks"), shared out among the containers, and the result does not depend on it
    const size_t blocks = e->demux_blocks ? e->demux_blocks : 4096;
    const unsigned per = (unsigned)std::max<size_t>(1, blocks / n);
    if (a->kind == demux::kTs) {
        k_ts_find<<<(unsigned)n, kDmxThreads, 0, s>>>(d_st, a->d_src);
        HIPCHK(hipGetLastError());
        k_ts_tiles<<<dim3((unsigned)std::min<size_t>(most_tiles, per), (unsigned)n), kDmxThreads, 0, s>>>(d_st, a->d_src, d_tiles);
        HIPCHK(hipGetLastError());
    } else {
        k_ps_walk<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(d_st, a->d_src, d_seg, (int)n);
        HIPCHK(hipGetLastError());
    }
    k_demux_plan<<<(unsigned)n, 64, 0, s>>>(d_st, d_head, d_tiles, d_seg, (int)n, (ull)a->cap, (ull)(uintptr_t)a->dst, h_rec);
    HIPCHK(hipGetLastError());
    const size_t table_blocks = a->kind == demux::kTs ? most_tiles : std::max<size_t>(1, (longest / 9 + kDmxThreads) / kDmxThreads);
    k_demux_table<<<dim3((unsigned)std::min<size_t>(table_blocks, per), (unsigned)n), kDmxThreads, 0, s>>>(d_st, a->d_src, d_tiles, d_seg, (demux::Stamp *)a->stamps,
                                                                                                          (ull)(a->stamps ? a->stamp_cap : 0));
    HIPCHK(hipGetLastError());
    const unsigned gw = (unsigned)std::min<size_t>(std::max<size_t>(1, (a->cap / 16 + kDmxThreads - 1) / kDmxThreads), blocks);
    k_demux_write<<<gw, kDmxThreads, 0, s>>>(d_st, d_head, a->d_src, d_seg, a->dst, (int)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    e->dmx_q.push(h_rec, h_rec + n);
    return M2V_OK;
}

extern "C" {

size_t m2v_demux_bound(const uint64_t *src_bytes, size_t nstreams)
{
    size_t total = 0;
    for (size_t b = 0; src_bytes && b < nstreams; ++b) total += ((size_t)src_bytes[b] + 31) & ~(size_t)31;
    return total;
}

int m2v_demux_scan_tile(void) { return (int)demux::kScanTile; }

int m2v_demux_report(m2v_enc *e, m2v_demux_stat *out, size_t max)
{
    if (!e) return M2V_E_PARAM;
    return e->dmx_q.pop31(out, max);
}

int m2v_demux_device(m2v_enc *e, int kind, const void *d_src, const uint64_t *src_off, const uint64_t *src_bytes, size_t nstreams, int stream,
                     void *d_dst, size_t cap, void *d_stamps, size_t stamp_cap, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    if (kind != M2V_MUX_TS && kind != M2V_MUX_PS) { e->set_err("m2v_demux_device: unknown kind %d", kind); return M2V_E_PARAM; }
    if (!d_src || !src_off || !src_bytes || !d_dst || !nstreams) { e->set_err("m2v_demux_device: a pointer is NULL or there is no container"); return M2V_E_PARAM; }
    if (nstreams > 65535) { e->set_err("m2v_demux_device: at most 65535 containers in a call"); return M2V_E_PARAM; }
    if (stream != -1 && (kind == M2V_MUX_TS ? stream < 0 || stream > 0x1FFF : stream < 0xE0 || stream > 0xEF)) {
        e->set_err("m2v_demux_device: stream %d is neither -1 nor a %s", stream, kind == M2V_MUX_TS ? "PID 0 .. 0x1FFF" : "stream_id 0xE0 .. 0xEF");
        return M2V_E_PARAM;
    }
    if (stamp_cap && (!d_stamps || ((uintptr_t)d_stamps & 7))) { e->set_err("m2v_demux_device: d_stamps is NULL or not on an 8-byte boundary"); return M2V_E_PARAM; }
    for (size_t b = 0; b < nstreams; ++b) {
        if (src_bytes[b] >> 47) { e->set_err("m2v_demux_device: container %zu is larger than 2^47 bytes", b); return M2V_E_PARAM; }
        if (src_off[b] >> 62) { e->set_err("m2v_demux_device: the offset of container %zu is 2^62 or more", b); return M2V_E_PARAM; }
    }
    if (in_progress(e, "m2v_demux_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    DemuxDeviceArgs a{kind, (const uint8_t *)d_src, src_off, src_bytes, nstreams, stream, (uint8_t *)d_dst, cap, d_stamps, stamp_cap, (hipStream_t)hip_stream};
    return guard(e, demux_device_impl, &a);
}

}  // extern "C"
