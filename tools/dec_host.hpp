// dec_host.hpp — the device decoder's arithmetic (csrc/m2v_decode_kernels.hpp) run serially on a CPU: scan every 16 positions, judge
// every event, walk every slice, reconstruct every macroblock, locate every output byte - the same functions the kernels of
// m2v_decode.hip are thin loops over, in the same order of decisions.  Plain C++ (g++ -I fpga-mpeg2-encoder_amd/csrc); used by
// tests/dec_cases.py (as a shared library) and by tools/dec_host_check.cpp (under the sanitizers).
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "m2v_decode_kernels.hpp"
#include "m2v_decode_streams.hpp"

namespace dec_host {
using namespace m2v::dec;

struct Record { uint64_t es_bytes, out_bytes, frame_bytes, err_offset; uint32_t pictures, gops, width, height, repeated_headers, chains; int32_t status; uint32_t reserved[3]; };

struct Sink {
    std::vector<MbRec> *mb_;
    std::vector<int32_t> *dc_;
    std::vector<int16_t> *lv_;
    size_t base;                                             // the slice's first macroblock
    void mb(int col, const MbRec &m, const int32_t (&dc)[6])
    {
        (*mb_)[base + col] = m;
        for (int k = 0; k < 6; ++k) (*dc_)[(base + col) * 6 + k] = dc[k];
    }
    void level(int col, int blk, uint32_t i, int32_t l) { (*lv_)[((base + col) * 6 + blk) * 64 + i] = (int16_t)l; }
};

// the residual of one block (zero where it is not coded)
inline void block_residual(const MbRec &m, const int32_t *dc, const int16_t *lv, int blk, int mode, int32_t (&res)[64])
{
    for (int i = 0; i < 64; ++i) res[i] = 0;
    if (!((m.cbp >> (5 - blk)) & 1)) return;
    int32_t sum = 0;
    for (uint32_t i = 0; i < 64; ++i) {
        res[i] = m.intra && i == 0 ? dequant_dc(dc[blk], mode) : dequant(lv[blk * 64 + i], i, m.intra != 0, 2 * m.qcode, mode);
        sum ^= res[i];
    }
    if (mode == kIso && !(sum & 1)) res[63] = mismatch(res[63]);
    for (int r = 0; r < 8; ++r) {
        int32_t a[8];
        for (int k = 0; k < 8; ++k) a[k] = res[r * 8 + k];
        idct_1d(a, true, mode);
        for (int k = 0; k < 8; ++k) res[r * 8 + k] = a[k];
    }
    for (int c = 0; c < 8; ++c) {
        int32_t a[8];
        for (int k = 0; k < 8; ++k) a[k] = res[k * 8 + c];
        idct_1d(a, false, mode);
        for (int k = 0; k < 8; ++k) res[k * 8 + c] = a[k];
    }
}

struct Pic { uint32_t ev, type, step; };

// the probe stage of one stream: the scan and the plan - the headers and the grammar of the start codes
struct Probed { Record R; Plan P; std::vector<uint64_t> ev; std::vector<Pic> pics; };

inline Probed probe(const uint8_t *es, uint64_t n)
{
    Probed Q{};
    Record &R = Q.R;
    R.es_bytes = n;
    auto refuse = [&](uint64_t at) { R.status = kSyntax; R.err_offset = at; R.out_bytes = 0; return Q; };
    // scan
    std::vector<uint64_t> &ev = Q.ev;
    uint64_t last_nz = 0;
    for (uint64_t p0 = 0; p0 < n; p0 += 16) {
        uint64_t w0, w1, w2;
        m2v::mux::load24(es, p0, n, w0, w1, w2);
        uint32_t cand = scan16(p0, n, w0, w1, w2, last_nz);
        while (cand) {
            const uint32_t j = (uint32_t)__builtin_ctz(cand);
            cand &= cand - 1u;
            ev.push_back((p0 + j) << 8 | m2v::mux::byte24(w0, w1, w2, j + 3));
        }
    }
    // plan
    const uint32_t nev = (uint32_t)ev.size();
    Plan &P = Q.P;
    uint64_t bad = plan_first(es, n, ev.data(), nev, P);
    if (bad != kNone) return refuse(bad);
    std::vector<Pic> &pics = Q.pics;
    long lastI = -1;
    for (uint32_t i = 0; i < nev; ++i) {
        const EvInfo f = plan_event(es, n, ev.data(), nev, i, P, last_nz);
        bad = min64(bad, f.bad);
        R.gops += f.gop; R.repeated_headers += f.rep;
        if (f.pic) {
            if (f.type == 1) { lastI = (long)pics.size(); ++R.chains; }
            if (lastI < 0) bad = min64(bad, ev_pos(ev[i]));            // a P picture without a reference
            pics.push_back(Pic{i, f.type, (uint32_t)((long)pics.size() - lastI)});
        }
    }
    if (bad != kNone) return refuse(bad);
    R.width = P.seq.width; R.height = P.seq.height; R.pictures = (uint32_t)pics.size();
    R.frame_bytes = frame_bytes(R.width, R.height);
    return Q;
}

// -> the record; the frames (record.out_bytes of them) in out.  cap: what the caller's buffer would hold
inline Record decode(const uint8_t *es, uint64_t n, int layout, int mode, uint64_t cap, std::vector<uint8_t> &out)
{
    out.clear();
    Probed Q = probe(es, n);
    Record R = Q.R;
    if (R.status != kOk) return R;
    auto refuse = [&](uint64_t at) { R.status = kSyntax; R.err_offset = at; R.out_bytes = 0; out.clear(); return R; };
    const std::vector<uint64_t> &ev = Q.ev;
    const std::vector<Pic> &pics = Q.pics;
    const Plan &P = Q.P;
    const uint32_t nev = (uint32_t)ev.size();
    uint64_t bad = kNone;
    const uint32_t w = P.seq.width, h = P.seq.height, W = 16 * P.mbw, H = 16 * P.mbh, mbs = P.mbw * P.mbh;
    if (R.frame_bytes * pics.size() > cap) { R.status = kOverflow; return R; }
    // slices and reconstruction, picture by picture
    std::vector<MbRec> mb(mbs);
    std::vector<int32_t> dc((size_t)mbs * 6);
    std::vector<int16_t> lv((size_t)mbs * 384);
    const size_t psz = (size_t)W * H * 3 / 2;
    std::vector<uint8_t> cur(psz), ref(psz);
    out.resize(R.frame_bytes * pics.size());
    for (size_t p = 0; p < pics.size(); ++p) {
        std::fill(lv.begin(), lv.end(), 0);
        for (uint32_t row = 0; row < P.mbh; ++row) {
            const uint32_t i = pics[p].ev + 2 + row;
            Sink sink{&mb, &dc, &lv, (size_t)row * P.mbw};
            if (!parse_slice(es, ev_pos(ev[i]), i + 1 < nev ? ev_pos(ev[i + 1]) : n, pics[p].type, (int)P.mbw, (int)P.mbh, (int)row, mode, sink))
                bad = min64(bad, ev_pos(ev[i]));
        }
        if (bad != kNone) continue;                          // (the other pictures' slices are still walked: the earliest error is reported)
        for (uint32_t k = 0; k < mbs; ++k) {
            const MbRec &m = mb[k];
            const int col = (int)(k % P.mbw), row = (int)(k / P.mbw);
            for (int blk = 0; blk < 6; ++blk) {
                int32_t res[64];
                block_residual(m, &dc[(size_t)k * 6], &lv[(size_t)k * 384], blk, mode, res);
                const bool luma = blk < 4;
                const int pw = luma ? (int)W : (int)W / 2;
                const size_t plane = luma ? 0 : (size_t)W * H + (size_t)(blk - 4) * (W / 2) * (H / 2);
                const int x0 = luma ? 16 * col + 8 * (blk & 1) : 8 * col, y0 = luma ? 16 * row + 8 * (blk >> 1) : 8 * row;
                const int mvx = luma ? m.mvx : chroma_vector(m.mvx, mode), mvy = luma ? m.mvy : chroma_vector(m.mvy, mode);
                for (int y = 0; y < 8; ++y)
                    for (int x = 0; x < 8; ++x) {
                        const int32_t pred = m.intra ? 128 : predict(ref.data() + plane, pw, x0 + x + (mvx >> 1), y0 + y + (mvy >> 1), mvx & 1, mvy & 1, mode);
                        cur[plane + (size_t)(y0 + y) * pw + x0 + x] = clip255(pred + res[y * 8 + x]);
                    }
            }
        }
        uint8_t *o = out.data() + p * R.frame_bytes;
        OutAt at{0, 0, 0, 0};
        for (uint32_t q = 0; q < (uint32_t)R.frame_bytes; ++q) {
            if (at.run > 1) out_step(at, layout); else at = out_locate(q, w, h, layout);
            o[q] = pic_sample(cur.data(), W, H, at);
        }
        cur.swap(ref);
    }
    if (bad != kNone) return refuse(bad);
    R.out_bytes = out.size();
    return R;
}

// ---- several streams per call: m2v_decode_streams.hip serially - the same plan_streams, the same tables, the same locators ----
struct Segment { const uint8_t *p; uint64_t n; };
struct StreamRecord { uint64_t es_offset, out_offset; Record rec; };      // es_offset: the caller's (a segment here is a pointer)

// the slices of a table's pictures, one after the other as the lanes of k_ds_slices take them; store: into the chunk's records
inline void walk_slices(const Segment *seg, const std::vector<Probed> &Q, const ChunkPic *tab, uint32_t ntab, uint32_t nslices, int mode,
                        const std::vector<int32_t> &status, std::vector<uint64_t> &err, bool store, std::vector<MbRec> &mb, std::vector<int32_t> &dc,
                        std::vector<int16_t> &lv)
{
    for (uint32_t g = 0; g < nslices; ++g) {
        const ChunkPic &C = tab[chunk_slice_pic(tab, ntab, g)];
        if (status[C.stream] != kOk) continue;
        const Probed &S = Q[C.stream];
        const uint32_t row = g - C.slice0, nev = (uint32_t)S.ev.size(), i = S.pics[C.pic].ev + 2 + row;
        const uint64_t start = ev_pos(S.ev[i]), end = i + 1 < nev ? ev_pos(S.ev[i + 1]) : seg[C.stream].n;
        std::vector<MbRec> mb1;
        std::vector<int32_t> dc1;
        std::vector<int16_t> lv1;
        if (!store) { mb1.resize(C.mbw); dc1.resize((size_t)C.mbw * 6); lv1.resize((size_t)C.mbw * 384); }
        Sink sink{store ? &mb : &mb1, store ? &dc : &dc1, store ? &lv : &lv1, store ? (size_t)C.mb_base + (size_t)row * C.mbw : 0};
        if (!parse_slice(seg[C.stream].p, start, end, C.type, (int)C.mbw, (int)C.mbh, (int)row, mode, sink)) err[C.stream] = min64(err[C.stream], start);
    }
}

// out: cap bytes, or NULL for a probe.  decode_batch: option "decode_batch"; level_bytes: the bound of the default chunk
inline std::vector<StreamRecord> decode_streams(const Segment *seg, size_t n, int layout, int mode, uint8_t *out, uint64_t cap, size_t decode_batch,
                                                uint64_t level_bytes = kStreamsLevelBytes)
{
    std::vector<Probed> Q(n);
    std::vector<std::vector<uint8_t>> types(n);
    std::vector<StreamInfo> info(n);
    for (size_t b = 0; b < n; ++b) {
        if (seg[b].n < 4) { Q[b].R.es_bytes = seg[b].n; Q[b].R.status = kSyntax; }      // not one start code
        else Q[b] = probe(seg[b].p, seg[b].n);
        for (const Pic &p : Q[b].pics) types[b].push_back((uint8_t)p.type);
        info[b] = StreamInfo{Q[b].R.status, Q[b].R.pictures, Q[b].R.width, Q[b].R.height, types[b].data()};
    }
    const StreamsPlan P = plan_streams(info.data(), n, cap, out == nullptr, decode_batch, level_bytes);
    std::vector<int32_t> status(n);
    std::vector<uint64_t> err(n, kNone);
    for (size_t b = 0; b < n; ++b) status[b] = Q[b].R.status;
    auto judge = [&]() { for (size_t b = 0; b < n; ++b) if (status[b] == kOk && err[b] != kNone) status[b] = kSyntax; };
    std::vector<MbRec> mb;
    std::vector<int32_t> dc;
    std::vector<int16_t> lv;
    std::vector<uint8_t> buf;
    if (out && P.pre_slices) {
        walk_slices(seg, Q, P.pre.data(), (uint32_t)P.pre.size(), P.pre_slices, mode, status, err, false, mb, dc, lv);
        judge();
    }
    for (const StreamsChunk &C : P.chunks) {
        if (!out) break;
        const ChunkPic *tab = P.pics.data() + C.first;
        mb.assign(C.mbs, MbRec{}); dc.assign(C.mbs * 6, 0); lv.assign(C.mbs * 384, 0);
        buf.resize(std::max<size_t>(buf.size(), C.buf_bytes));
        walk_slices(seg, Q, tab, (uint32_t)C.count, C.slices, mode, status, err, true, mb, dc, lv);
        judge();
        for (const StreamsChunk::Step &S : C.steps)
            for (size_t y = 0; y < S.count; ++y) {
                const ChunkPic &c = tab[P.list[S.off + y]];
                if (status[c.stream] != kOk) continue;
                const uint32_t W = 16 * c.mbw, H = 16 * c.mbh;
                uint8_t *cur = buf.data() + c.buf_off;
                const uint8_t *ref = buf.data() + c.ref_off;
                for (uint32_t k = 0; k < c.mbw * c.mbh; ++k) {
                    const size_t at = c.mb_base + k;
                    const MbRec &m = mb[at];
                    const int col = (int)(k % c.mbw), row = (int)(k / c.mbw);
                    for (int blk = 0; blk < 6; ++blk) {
                        int32_t res[64];
                        block_residual(m, &dc[at * 6], &lv[at * 384], blk, mode, res);
                        const bool luma = blk < 4;
                        const int pw = luma ? (int)W : (int)W / 2;
                        const size_t plane = luma ? 0 : (size_t)W * H + (size_t)(blk - 4) * (W / 2) * (H / 2);
                        const int x0 = luma ? 16 * col + 8 * (blk & 1) : 8 * col, y0 = luma ? 16 * row + 8 * (blk >> 1) : 8 * row;
                        const int mvx = luma ? m.mvx : chroma_vector(m.mvx, mode), mvy = luma ? m.mvy : chroma_vector(m.mvy, mode);
                        for (int yy = 0; yy < 8; ++yy)
                            for (int x = 0; x < 8; ++x) {
                                const int32_t pred = m.intra ? 128 : predict(ref + plane, pw, x0 + x + (mvx >> 1), y0 + yy + (mvy >> 1), mvx & 1, mvy & 1, mode);
                                cur[plane + (size_t)(y0 + yy) * pw + x0 + x] = clip255(pred + res[yy * 8 + x]);
                            }
                    }
                }
            }
        for (uint64_t o = C.lo; o < C.hi; ++o) {                   // every byte of the chunk's range through the locator of k_ds_out
            const OutByte B = streams_out_locate(tab, (uint32_t)C.count, o, layout);
            const ChunkPic &c = tab[B.pic];
            if (status[c.stream] == kOk) out[o] = pic_sample(buf.data() + c.buf_off, 16 * c.mbw, 16 * c.mbh, B.at);
        }
        if (C.carry_out) {
            const ChunkPic &L = tab[C.count - 1];
            memmove(buf.data(), buf.data() + L.buf_off, (size_t)L.mbw * L.mbh * 384);
        }
    }
    std::vector<StreamRecord> recs(n);
    for (size_t b = 0; b < n; ++b) {
        StreamRecord &r = recs[b];
        r.es_offset = 0; r.out_offset = P.out_offset[b]; r.rec = Q[b].R;
        if (r.rec.status != kOk) continue;
        if (P.overflow[b]) r.rec.status = kOverflow;
        else if (status[b] != kOk) { r.rec.status = status[b]; r.rec.err_offset = err[b]; }
        else r.rec.out_bytes = r.rec.frame_bytes * r.rec.pictures;
    }
    return recs;
}

}  // namespace dec_host
