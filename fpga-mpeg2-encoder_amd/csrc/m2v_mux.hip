// m2v_mux.hip — transport and program stream out of the encoder, muxed on the device (include/m2v_mi355x.h: m2v_set_mux_out,
// m2v_mux_device).  The container step of include/m2v_container.h rescans the whole stream on one CPU core; here it is three kernels
// behind the last chunk's assembly, and the bytes are those of m2vc_mux_ts / m2vc_mux_ps exactly (m2v_container.cpp is the
// specification; m2v_mux_kernels.hpp holds every function that decides a byte, and compiles for the host too).
//
//   k_es_scan    all blocks, 16 stream bytes per lane: start codes cannot be emulated inside MPEG-2 video, so 00 00 01 xx found at any
//                position is one.  The codes a picture table is made of (B3, B8, 00, B7 - a few per picture) are appended to the
//                stream's event list through one atomic each, in whatever order; what scan() validates travels as four maxima per
//                stream (first end code, first bad picture header, first slice, last byte that is not zero).  A lane reads the 24
//                bytes from its first position on, so a start code may straddle any lane, wavefront or tile boundary.
//   k_mux_plan   one block per stream: sorts the events (bitonic, in LDS up to kPlanLds of them), then ONE lane walks them through
//                scan()'s state machine into the picture table and walks the pictures through the plan - rate, pts0, every picture's
//                place, and for TS the PSI recurrence, whose "now" depends on the insertions before it: about one double division
//                per picture, serial by nature, microseconds for the pictures a resident call holds.  The block that finishes last
//                places the containers one behind the other (each on a 32-byte boundary), judges them against cap and writes the
//                records, to the device and straight into pinned memory.
//   k_mux_write  grid-stride, one lane per 16 output bytes at a 16-byte boundary of the destination: binary search of the plan, then
//                header, stuffing or payload bytes (gen16).  Aligned 16-byte stores, unaligned loads; the first and last unit of a
//                container that does not start or end on a boundary go byte by byte.  A stream whose status is not OK has no units.
//
// No wait is added: the kernels take the stream's length from the control word (or the batch's records) on the device.  k_mb and every
// other kernel are untouched, and with no buffer set nothing here is reached.
#include "m2v_host.hpp"
#include "m2v_mux_kernels.hpp"

static_assert(sizeof(m2v_mux_stat) == 40, "the record of include/m2v_mi355x.h is 40 bytes");
static_assert(sizeof(mux::Pic) == 32, "a picture of the plan is 32 bytes");
static_assert(M2V_MUX_TS == mux::kTs && M2V_MUX_PS == mux::kPs && M2V_MUX_SYNTAX == mux::kSyntax && M2V_MUX_OVERFLOW == mux::kOverflow,
              "m2v_mux_kernels.hpp repeats the values of include/m2v_mi355x.h");

namespace m2v {

constexpr int kMuxThreads = 256;
constexpr int kPlanLds = 2048;             // events sorted in LDS (16 KiB); more: in place, in memory
static_assert(mux::kScanTile == 4 * kMuxThreads * 16, "a tile is four passes of a block");

struct MuxHead { unsigned long long total_units; uint32_t ticket, pad; unsigned long long reserved[6]; };      // 64 bytes in front of the streams

// where a stream's place and length come from: the Stream itself (bytes == nullptr: the host wrote them), or the encoder's records
// on the device - element s * stride of off (nullptr: 0) and bytes - which are void while *overflow is set
struct MuxSrc { const unsigned long long *off, *bytes; int stride; const uint32_t *overflow; };

__device__ __forceinline__ void mux_src(const MuxSrc &src, const mux::Stream *S, int s, unsigned long long &off, unsigned long long &bytes)
{
    if (!src.bytes) { off = S->es_off; bytes = S->es_bytes; return; }
    off = src.off ? src.off[(size_t)s * src.stride] : 0ull;
    bytes = src.bytes[(size_t)s * src.stride];
}

__global__ __launch_bounds__(kMuxThreads) void k_es_scan(mux::Stream *st, MuxSrc src, const uint8_t *__restrict__ d_es, unsigned long long *__restrict__ ev)
{
    if (src.overflow && *src.overflow) return;
    mux::Stream *S = st + blockIdx.y;
    unsigned long long off, bytes;
    mux_src(src, S, blockIdx.y, off, bytes);
    const uint8_t *es = d_es + off;
    const uint32_t ev_base = S->ev_base, ev_cap = S->ev_cap;
    const unsigned long long ntiles = (bytes + mux::kScanTile - 1) / mux::kScanTile;
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        mux::ScanAcc a;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const unsigned long long p0 = t * mux::kScanTile + (unsigned long long)(it * kMuxThreads + threadIdx.x) * 16u;
            if (p0 >= bytes) break;
            uint64_t w0, w1, w2;
            mux::load24(es, p0, bytes, w0, w1, w2);
            mux::scan16(p0, bytes, w0, w1, w2, a, [&](uint64_t v) {
                const uint32_t slot = atomicAdd(&S->ev_count, 1u);
                if (slot < ev_cap) ev[(size_t)ev_base + slot] = v;
            });
        }
        // the wavefront's maxima, then one atomic per value that is set
        unsigned long long v0 = a.inv_first_end, v1 = a.inv_first_bad, v2 = a.inv_first_slice, v3 = a.last_nz;
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            v0 = mux::max64(v0, __shfl_xor(v0, d)); v1 = mux::max64(v1, __shfl_xor(v1, d));
            v2 = mux::max64(v2, __shfl_xor(v2, d)); v3 = mux::max64(v3, __shfl_xor(v3, d));
        }
        if ((threadIdx.x & 63) == 0) {
            if (v0) atomicMax((unsigned long long *)&S->inv_first_end, v0);
            if (v1) atomicMax((unsigned long long *)&S->inv_first_bad, v1);
            if (v2 && v2 > *(volatile unsigned long long *)&S->inv_first_slice) atomicMax((unsigned long long *)&S->inv_first_slice, v2);
            if (v3) atomicMax((unsigned long long *)&S->last_nz, v3);
        }
    }
}

template <typename T> __device__ __forceinline__ T mux_peek(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kMuxThreads) void k_mux_plan(mux::Stream *st, MuxHead *head, MuxSrc src, const uint8_t *__restrict__ d_es, unsigned long long *ev,
                                                          mux::Pic *pics, int nstreams, unsigned long long cap, unsigned long long dst_addr, m2v_mux_stat *h_rec)
{
    __shared__ unsigned long long s_ev[kPlanLds];
    __shared__ int s_last;
    const int s = blockIdx.x, tid = threadIdx.x;
    mux::Stream *S = st + s;
    const bool es_ov = src.overflow && *src.overflow;
    unsigned long long off = 0, bytes = 0;
    if (!es_ov) mux_src(src, S, s, off, bytes);
    const uint32_t nev = S->ev_count, ev_cap = S->ev_cap;
    unsigned long long *mine = ev + S->ev_base;
    int status = es_ov ? mux::kOverflow : nev > ev_cap ? mux::kEvents : mux::kOk;
    unsigned long long *sorted = mine;
    if (status == mux::kOk && nev > 1) {
        // bitonic sort of the events by position: padded to a power of two (ev_cap is one) with keys behind every position
        uint32_t m = 2;
        while (m < nev) m <<= 1;
        const bool lds = m <= (uint32_t)kPlanLds;
        unsigned long long *a = lds ? s_ev : mine;
        for (uint32_t i = tid; i < m; i += kMuxThreads) { if (lds) a[i] = i < nev ? mine[i] : ~0ull; else if (i >= nev) a[i] = ~0ull; }
        __syncthreads();
        for (uint32_t k = 2; k <= m; k <<= 1)
            for (uint32_t j = k >> 1; j; j >>= 1) {
                for (uint32_t i = tid; i < m; i += kMuxThreads) {
                    const uint32_t x = i ^ j;
                    if (x > i) {
                        const unsigned long long u = a[i], v = a[x];
                        if ((u > v) == ((i & k) == 0)) { a[i] = v; a[x] = u; }
                    }
                }
                __syncthreads();
            }
        sorted = a;
    }
    if (tid == 0) {
        mux::Stream L = *S;
        L.es_off = off; L.es_bytes = bytes;
        L.npics = 0; L.n = 0; L.out_bytes = 0; L.out_off = 0; L.unit0 = 0;
        if (status == mux::kOk) {
            uint64_t maxpic;
            mux::Pic *table = pics + L.pic_base;
            status = mux::plan_pictures(d_es + off, bytes, (const uint64_t *)sorted, nev, ev_cap, L, table, L.npics, L.n, maxpic);
            if (status == mux::kOk) L.out_bytes = mux::plan_layout(L, table, d_es + off, maxpic);
        }
        L.status = status;
        *S = L;
        __threadfence();
        s_last = atomicAdd(&head->ticket, 1u) == (uint32_t)nstreams - 1u;
    }
    __syncthreads();
    if (!s_last || tid) return;
    // the last block: every stream's plan is in memory.  Containers one behind the other, each on a 32-byte boundary of the buffer
    unsigned long long end = 0, units = 0;
    bool again = false;                                      // an event list was too small: the call runs again, this run writes nothing
    for (int b = 0; b < nstreams; ++b) {
        mux::Stream *B = st + b;
        int stb = mux_peek(&B->status);
        again = again || stb == mux::kEvents;
        unsigned long long ob = mux_peek(&B->out_bytes);
        const unsigned long long o = (end + 31ull) & ~31ull;
        if (stb == mux::kOk && (o > cap || ob > cap - o)) stb = mux::kOverflow;
        if (stb != mux::kOk) ob = 0;
        const unsigned long long lead = (dst_addr + o) & 15ull;
        B->status = stb; B->out_off = o; B->out_bytes = ob; B->unit0 = units;
        if (ob) { units += (ob + lead + 15ull) >> 4; end = o + ob; }
        const m2v_mux_stat r{mux_peek(&B->es_off), mux_peek(&B->es_bytes), o, ob, stb == mux::kOk ? mux_peek(&B->npics) : 0u, stb};
        h_rec[b] = r;
    }
    head->total_units = again ? 0ull : units;
    head->ticket = 0;
}

typedef uint32_t mux_store_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kMuxThreads) void k_mux_write(const mux::Stream *__restrict__ st, const MuxHead *__restrict__ head, const uint8_t *__restrict__ d_es,
                                                           const mux::Pic *__restrict__ pics, uint8_t *__restrict__ dst, int nstreams)
{
    const unsigned long long total = head->total_units;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kMuxThreads + threadIdx.x; g < total; g += (unsigned long long)gridDim.x * kMuxThreads) {
        int lo = 0, hi = nstreams - 1;                       // the last stream whose first unit is at or in front of g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (st[mid].unit0 <= g) lo = mid; else hi = mid - 1;
        }
        const mux::Stream &S = st[lo];
        uint8_t *out = dst + S.out_off;
        const long long q0 = (long long)((g - S.unit0) << 4) - (long long)((uintptr_t)out & 15u);
        const mux::Win w = mux::gen16(S, pics + S.pic_base, d_es + S.es_off, q0);
        if (q0 >= 0 && (unsigned long long)q0 + 16u <= S.out_bytes) {
            *(__attribute__((address_space(1))) mux_store_t *)(out + q0) = mux_store_t{(uint32_t)w.lo, (uint32_t)(w.lo >> 32), (uint32_t)w.hi, (uint32_t)(w.hi >> 32)};
        } else {
            for (int k = 0; k < 16; ++k) {
                const long long q = q0 + k;
                if (q >= 0 && (unsigned long long)q < S.out_bytes) out[q] = (uint8_t)((k < 8 ? w.lo : w.hi) >> (8 * (k & 7)));
            }
        }
    }
}

static uint32_t pow2_at_least(size_t v)
{
    uint32_t m = 2;
    while (m < v && m < 0x80000000u) m <<= 1;
    return m;
}

// Everything one mux enqueues on s: the streams' initial state up, the three kernels.  ev_caps: the event capacity of every stream;
// es_off / es_bytes: the host's (src.bytes == nullptr) or nullptr; longest: no stream is longer.  The records arrive in pinned memory
// (mux_records) when s has run dry.
static void mux_enqueue(m2v_enc *e, hipStream_t s, int kind, size_t nstreams, const std::vector<uint32_t> &ev_caps, const uint64_t *es_off,
                        const uint64_t *es_bytes, MuxSrc src, const uint8_t *d_es, uint8_t *dst, size_t cap, size_t longest)
{
    size_t ev_total = 0;
    for (size_t b = 0; b < nstreams; ++b) ev_total += ev_caps[b];
    const size_t st_bytes = sizeof(MuxHead) + nstreams * sizeof(mux::Stream), rec_bytes = nstreams * sizeof(m2v_mux_stat);
    e->d_mux_st.recorded = e->d_mux_pic.recorded = false;
    e->d_mux_ev.recorded = false;
    e->d_mux_st.ensure(st_bytes);
    e->d_mux_ev.ensure(ev_total);
    e->d_mux_pic.ensure((ev_total + nstreams) * sizeof(mux::Pic));
    ensure_pinned(e->h_mux, e->h_mux_cap, st_bytes + rec_bytes + 64);
    memset(e->h_mux, 0, st_bytes + rec_bytes);
    auto *h_st = (mux::Stream *)(e->h_mux + sizeof(MuxHead));
    size_t at = 0;
    for (size_t b = 0; b < nstreams; ++b) {
        mux::Stream &S = h_st[b];
        if (es_off) { S.es_off = es_off[b]; S.es_bytes = es_bytes[b]; }
        S.ev_base = (uint32_t)at; S.ev_cap = ev_caps[b]; S.pic_base = (uint32_t)(at + b); S.kind = (uint32_t)kind;
        at += ev_caps[b];
    }
    e->mux_n = nstreams;
    timer_break(e);
    HIPCHK(hipMemcpyAsync(e->d_mux_st.p, e->h_mux, st_bytes, hipMemcpyHostToDevice, s));
    auto *d_head = (MuxHead *)e->d_mux_st.p;
    auto *d_st = (mux::Stream *)(e->d_mux_st.p + sizeof(MuxHead));
    auto *d_pic = (mux::Pic *)e->d_mux_pic.p;
    auto *h_rec = (m2v_mux_stat *)(e->h_mux + st_bytes);
    const size_t tiles = std::max<size_t>(1, (longest + mux::kScanTile - 1) / mux::kScanTile);
    const unsigned gx = (unsigned)std::min<size_t>(tiles, std::max<size_t>(1, 4096 / nstreams));
    k_es_scan<<<dim3(gx, (unsigned)nstreams), kMuxThreads, 0, s>>>(d_st, src, d_es, e->d_mux_ev.p);
    HIPCHK(hipGetLastError());
    k_mux_plan<<<(unsigned)nstreams, kMuxThreads, 0, s>>>(d_st, d_head, src, d_es, e->d_mux_ev.p, d_pic, (int)nstreams, (unsigned long long)cap,
                                                        (unsigned long long)(uintptr_t)dst, h_rec);
    HIPCHK(hipGetLastError());
    const unsigned gw = (unsigned)std::min<size_t>(std::max<size_t>(1, (cap / 16 + kMuxThreads - 1) / kMuxThreads), 4096);
    k_mux_write<<<gw, kMuxThreads, 0, s>>>(d_st, d_head, d_es, d_pic, dst, (int)nstreams);
    HIPCHK(hipGetLastError());
}

static const m2v_mux_stat *mux_records(const m2v_enc *e)
{
    return (const m2v_mux_stat *)(e->h_mux + sizeof(MuxHead) + e->mux_n * sizeof(mux::Stream));
}

// behind the last chunk's assembly, in front of the control word's copy: the call's stream, or one per clip of a batch
void mux_resident(m2v_enc *e, hipStream_t s, const uint8_t *d_out, size_t cap, size_t nframes)
{
    if (!e->seq.mux.kind) return;
    const size_t nstreams = seq_batch(e) ? e->seq.lens.size() : 1;
    // (the encoder writes at most a sequence header, a GOP header and a picture header per picture, and one end code)
    std::vector<uint32_t> caps(nstreams);
    for (size_t b = 0; b < nstreams; ++b) caps[b] = pow2_at_least(3 * (size_t)(seq_batch(e) ? e->seq.lens[b] : nframes) + 2);
    MuxSrc src{nullptr, &e->d_ctl.p->total_bytes, 0, &e->d_ctl.p->overflow};
    if (seq_batch(e)) {
        static_assert(sizeof(m2v_sequence_stat) == 32 && offsetof(m2v_sequence_stat, bytes) == 8, "offset and bytes of a batch's records");
        src = MuxSrc{&e->d_seq.p->offset, &e->d_seq.p->bytes, 4, &e->d_ctl.p->overflow};
    }
    mux_enqueue(e, s, e->seq.mux.kind, nstreams, caps, nullptr, nullptr, src, d_out, e->seq.mux.p, e->seq.mux.cap, cap);
    e->mux_pending = true;
}

void mux_collect(m2v_enc *e)
{
    if (!e->mux_pending) return;
    e->mux_pending = false;
    const m2v_mux_stat *r = mux_records(e);
    e->mux_q.push(r, r + e->mux_n);               // (the queue was emptied when the call started)
    for (auto &q : e->mux_q.q) if (q.status == mux::kEvents) q.status = M2V_MUX_SYNTAX;      // (more headers than the encoder writes)
}

void mux_release(m2v_enc *e)
{
    e->d_mux_st.release(); e->d_mux_ev.release(); e->d_mux_pic.release();
    if (e->h_mux) (void)hipHostFree(e->h_mux);
    e->h_mux = nullptr; e->h_mux_cap = 0;
}

}  // namespace m2v

struct MuxDeviceArgs { int kind; const uint8_t *d_es; const uint64_t *off, *bytes; size_t n; uint8_t *dst; size_t cap; hipStream_t s; };

static int mux_device_impl(m2v_enc *e, void *argp)
{
    auto *a = (MuxDeviceArgs *)argp;
    hipStream_t s = a->s ? a->s : e->stream;
    e->mux_q.clear();
    size_t longest = 0;
    std::vector<uint32_t> caps(a->n);
    for (size_t b = 0; b < a->n; ++b) {
        longest = std::max<size_t>(longest, a->bytes[b]);
        caps[b] = pow2_at_least(std::max<size_t>(256, a->bytes[b] / 1024));       // a guess: a second run takes the count of the first
    }
    for (int run = 0; run < 2; ++run) {
        size_t total = 0;
        for (uint32_t c : caps) total += c;
        if (total > 0x7FFFFFFFu) { e->set_err("m2v_mux_device: the streams hold more than 2^31 headers"); return M2V_E_PARAM; }
        mux_enqueue(e, s, a->kind, a->n, caps, a->off, a->bytes, MuxSrc{nullptr, nullptr, 0, nullptr}, a->d_es, a->dst, a->cap, longest);
        HIPCHK(hipStreamSynchronize(s));
        const m2v_mux_stat *r = mux_records(e);
        bool again = false;
        for (size_t b = 0; b < a->n; ++b) again = again || r[b].status == mux::kEvents;
        if (!again) break;
        // some stream has more headers than guessed (nothing was written for it): their counts are in the streams' state
        std::vector<uint8_t> img(sizeof(MuxHead) + a->n * sizeof(mux::Stream));
        HIPCHK(hipMemcpy(img.data(), e->d_mux_st.p, img.size(), hipMemcpyDeviceToHost));
        const auto *st = (const mux::Stream *)(img.data() + sizeof(MuxHead));
        for (size_t b = 0; b < a->n; ++b) caps[b] = pow2_at_least(std::max<size_t>(caps[b], st[b].ev_count));
    }
    e->mux_pending = true;
    mux_collect(e);
    return M2V_OK;
}

extern "C" {

size_t m2v_mux_bound(int kind, size_t es_bytes, size_t pictures)
{
    if (kind != M2V_MUX_TS && kind != M2V_MUX_PS) return 0;
    return (size_t)mux::bound(kind, es_bytes, pictures);
}

int m2v_mux_scan_tile(void) { return (int)mux::kScanTile; }

int m2v_set_mux_out(m2v_enc *e, int kind, void *d_dst, size_t cap)
{
    if (!e) return M2V_E_PARAM;
    if (in_progress(e, "m2v_set_mux_out", "the buffer is sampled when a sequence starts")) return M2V_E_STATE;
    if (kind != M2V_MUX_NONE && kind != M2V_MUX_TS && kind != M2V_MUX_PS) { e->set_err("m2v_set_mux_out: unknown kind %d", kind); return M2V_E_PARAM; }
    if (kind != M2V_MUX_NONE && !d_dst) { e->set_err("m2v_set_mux_out: d_dst is NULL"); return M2V_E_PARAM; }
    e->seq.mux = m2v_enc::MuxDst{};
    e->set.mux = m2v_enc::MuxDst{};
    if (kind != M2V_MUX_NONE) { e->set.mux.kind = kind; e->set.mux.p = (uint8_t *)d_dst; e->set.mux.cap = cap; }
    return M2V_OK;
}

int m2v_mux_report(m2v_enc *e, m2v_mux_stat *out, size_t max)
{
    if (!e) return M2V_E_PARAM;
    return e->mux_q.pop31(out, max);
}

int m2v_mux_device(m2v_enc *e, int kind, const void *d_es, const uint64_t *es_off, const uint64_t *es_bytes, size_t nstreams, void *d_dst,
                   size_t cap, void *hip_stream)
{
    if (!e) return M2V_E_PARAM;
    if (kind != M2V_MUX_TS && kind != M2V_MUX_PS) { e->set_err("m2v_mux_device: unknown kind %d", kind); return M2V_E_PARAM; }
    if (!d_es || !es_off || !es_bytes || !d_dst || !nstreams) { e->set_err("m2v_mux_device: a pointer is NULL or there is no stream"); return M2V_E_PARAM; }
    if (nstreams > 65535) { e->set_err("m2v_mux_device: at most 65535 streams in a call"); return M2V_E_PARAM; }
    if (in_progress(e, "m2v_mux_device", "m2v_encode_resident_end first")) return M2V_E_STATE;
    MuxDeviceArgs a{kind, (const uint8_t *)d_es, es_off, es_bytes, nstreams, (uint8_t *)d_dst, cap, (hipStream_t)hip_stream};
    return guard(e, mux_device_impl, &a);
}

}  // extern "C"
