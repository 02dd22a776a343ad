// dec_host.hpp — the device decoder's arithmetic (csrc/m2v_decode_kernels.hpp) run serially on a CPU: scan every 16 positions, judge
// every event, walk every slice, reconstruct every macroblock, locate every output byte - the same functions the kernels of
// m2v_decode.hip are thin loops over, in the same order of decisions.  Plain C++ (g++ -I fpga-mpeg2-encoder_amd/csrc); used by
// tests/dec_cases.py (as a shared library) and by tools/dec_host_check.cpp (under the sanitizers).
#pragma once
#include <string.h>

#include <vector>

#include "m2v_decode_kernels.hpp"

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

// -> the record; the frames (record.out_bytes of them) in out.  cap: what the caller's buffer would hold
inline Record decode(const uint8_t *es, uint64_t n, int layout, int mode, uint64_t cap, std::vector<uint8_t> &out)
{
    Record R{};
    R.es_bytes = n;
    out.clear();
    auto refuse = [&](uint64_t at) { R.status = kSyntax; R.err_offset = at; R.out_bytes = 0; out.clear(); return R; };
    // scan
    std::vector<uint64_t> ev;
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
    Plan P{};
    uint64_t bad = plan_first(es, n, ev.data(), nev, P);
    if (bad != kNone) return refuse(bad);
    struct Pic { uint32_t ev, type, step; };
    std::vector<Pic> pics;
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
    const uint32_t w = P.seq.width, h = P.seq.height, W = 16 * P.mbw, H = 16 * P.mbh, mbs = P.mbw * P.mbh;
    R.width = w; R.height = h; R.pictures = (uint32_t)pics.size();
    R.frame_bytes = frame_bytes(w, h);
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

}  // namespace dec_host
