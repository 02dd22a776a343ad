// dec_t_host.hpp — the macroblock-tools path of the device decoder (the t_ functions of csrc/m2v_decode_kernels.hpp, option
// "decode_mb_tools" on top of "decode_extended") run serially on a CPU, as tools/dec_x_host.hpp runs the extended path, in the order of
// decisions of m2v_decode_t.hip: scan, judge every event (t_event), find every picture's references - a P picture's "backward"
// picture is its forward reference, for dual prime -, display index, slices and matrices, walk every slice (t_slice), judge continuity,
// reconstruct every macroblock, place every picture at its display index.  b_pictures and interlaced are options "decode_b_pictures"
// and "decode_interlaced".  Plain C++; used by tests/mbt_cases.py (as a shared library) and tools/dec_t_host_check.cpp (under the
// sanitizers).
#pragma once
#include "dec_i_host.hpp"

namespace dec_t_host {
using namespace m2v::dec;
using dec_host::Record;
using dec_i_host::Sink;

struct Pic { uint32_t ev, type, slice0, nslices, params, display, sbase; XMats mats; long fwd, bwd; };

inline Record decode(const uint8_t *es, uint64_t n, int layout, uint64_t cap, bool b_pictures, bool interlaced, std::vector<uint8_t> &out)
{
    out.clear();
    Record R{};
    R.es_bytes = n;
    auto refuse = [&](uint64_t at) { R.status = kSyntax; R.err_offset = at; R.out_bytes = 0; out.clear(); return R; };
    if (n < 4) return refuse(0);                             // not one start code
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
    const uint32_t nev = (uint32_t)ev.size();
    MainPlan P{};
    uint64_t bad = interlaced ? il_first(es, n, ev.data(), nev, P) : main_first(es, n, ev.data(), nev, P);
    if (bad != kNone) return refuse(bad);
    std::vector<Pic> pics;
    long lastI = -1, a1 = -1, a2 = -1;                       // the last I picture; the last anchor and the one before it
    int prev = -1;
    XMats run{kNoEvent, kNoEvent};                           // the matrices in force in front of event i
    uint32_t nsl = 0;                                        // the slice events in front of event i
    for (uint32_t i = 0; i < nev; ++i) {
        const EvInfo f = t_event(es, n, ev.data(), nev, i, P, last_nz, prev, b_pictures, interlaced);
        if (main_significant(main_role(es, n, ev[i]))) prev = (int)i;
        bad = min64(bad, f.bad);
        R.gops += f.gop; R.repeated_headers += f.rep;
        if (f.pic) {
            const long p = (long)pics.size();
            if (f.type == 1) { lastI = p; ++R.chains; }
            if (lastI < 0) bad = min64(bad, ev_pos(ev[i]));            // a P picture without a reference
            if (f.type == 3 && a2 < 0) bad = min64(bad, ev_pos(ev[i]));      // a B picture without two anchors in front of it
            Pic q{i, f.type, 0, 0, 0, 0, 0, run, f.type == 2 ? a1 : f.type == 3 ? a2 : -1, f.type == 3 || f.type == 2 ? a1 : -1};
            uint32_t quant;
            q.params = t_picture_params(es, n, ev.data(), nev, i, b_pictures, interlaced, P.seq.h.progressive, q.slice0, q.nslices, quant);
            q.mats = x_mats_picture(es, n, ev.data(), nev, run, quant);
            q.sbase = nsl;
            if (f.type != 3) { a2 = a1; a1 = p; }
            pics.push_back(q);
        }
        x_mats_event(es, n, ev.data(), nev, i, run);
        nsl += main_role(es, n, ev[i]) == rSlice;
    }
    if (bad != kNone) return refuse(bad);
    {   // display indices: backwards, every anchor in front of the next one (without B pictures: the coded order)
        uint32_t next = (uint32_t)pics.size();
        for (size_t p = pics.size(); p-- > 0;) {
            if (pics[p].type == 3) pics[p].display = bp_display_b((uint32_t)p);
            else { pics[p].display = bp_display_anchor(next); next = (uint32_t)p; }
        }
    }
    const SeqHdr &h = P.seq.h;
    R.width = h.width; R.height = h.height; R.pictures = (uint32_t)pics.size();
    R.frame_bytes = frame_bytes(R.width, R.height);
    const uint32_t W = 16 * P.mbw, H = 16 * P.mbh, mbs = P.mbw * P.mbh;
    if (R.frame_bytes * pics.size() > cap) { R.status = kOverflow; return R; }
    std::vector<IMb> mb(mbs);
    std::vector<int32_t> dc((size_t)mbs * 6);
    std::vector<int16_t> lv((size_t)mbs * 384);
    const size_t psz = (size_t)W * H * 3 / 2;
    std::vector<std::vector<uint8_t>> planes(pics.size());   // every picture in coded order (the streams of the tests are small)
    std::vector<uint32_t> spans(nsl + 1u);
    out.resize(R.frame_bytes * pics.size());
    for (size_t p = 0; p < pics.size(); ++p) {
        std::fill(lv.begin(), lv.end(), 0);
        std::fill(mb.begin(), mb.end(), IMb{});
        const TPicParams pp = t_params_unpack(pics[p].params);
        std::vector<uint32_t> &span = spans;                 // slot sbase - sbase[0] + k for slice k of the picture, as in a chunk of all pictures
        const uint32_t g0 = pics[p].sbase - pics[0].sbase;
        for (uint32_t k = 0; k < pics[p].nslices; ++k) {     // the walk: one span per slice
            const uint32_t i = pics[p].slice0 + k, code = ev_code(ev[i]);
            Sink sink{&mb, &dc, &lv, (size_t)(code - 1u) * P.mbw};
            int first, last;
            const bool ok = t_slice(es, ev_pos(ev[i]), i + 1 < nev ? ev_pos(ev[i + 1]) : n, pics[p].type, pp, (int)P.mbw, (int)P.mbh, (int)code - 1, sink, first, last);
            span[g0 + k] = x_span_pack(ok, code, first, last);
            if (!ok) bad = min64(bad, ev_pos(ev[i]));
        }
        for (uint32_t g = g0; g < g0 + pics[p].nslices; ++g) {     // the judge: every slice finds its picture as a lane does
            uint32_t k;
            const uint32_t at = x_slice_pic(pics.data(), (uint32_t)pics.size(), g, k);
            if (at != p || !(span[g] >> 31)) { if (at != p) bad = min64(bad, 0); continue; }
            if (!x_continuous(span[g], k ? span[g - 1] : 0u, k, pics[at].nslices, P.mbw)) bad = min64(bad, ev_pos(ev[pics[at].slice0 + k]));
        }
        if (bad != kNone) continue;                          // (the other pictures' slices are still walked: the earliest error is reported)
        MainSeq seq = P.seq;                                 // the picture's row of the matrix table
        for (uint32_t t = 0; t < 64; ++t) {
            seq.wi[t] = (uint8_t)x_matrix_weight(es, n, ev.data(), nev, pics[p].mats.mi, 0, t, P.seq.wi);
            seq.wn[t] = (uint8_t)x_matrix_weight(es, n, ev.data(), nev, pics[p].mats.mn, 1, t, P.seq.wn);
        }
        std::vector<uint8_t> &cur = planes[p];
        cur.assign(psz, 0);
        const uint8_t *fwd = pics[p].fwd >= 0 ? planes[(size_t)pics[p].fwd].data() : cur.data();
        const uint8_t *bwd = pics[p].bwd >= 0 ? planes[(size_t)pics[p].bwd].data() : cur.data();
        for (uint32_t k = 0; k < mbs; ++k) {
            const IMb &m = mb[k];
            MainMb mm{};
            mm.intra = m.intra; mm.cbp = m.cbp; mm.qcode = m.qcode;
            const int col = (int)(k % P.mbw), row = (int)(k / P.mbw);
            int32_t res[6][64];
            for (int blk = 0; blk < 6; ++blk) dec_main_host::block_residual(mm, &dc[(size_t)k * 6], &lv[(size_t)k * 384], blk, seq, pp.i.b.p, res[blk]);
            for (uint32_t y = 0; y < 16; ++y)                // luma through the row map
                for (uint32_t x = 0; x < 16; ++x) {
                    const int px = 16 * col + (int)x, py = 16 * row + (int)y;
                    const int32_t pred = m.intra ? 128 : il_predict(fwd, bwd, (int)W, px, py, m, false);
                    cur[(size_t)py * W + px] = clip255(pred + res[il_luma_block(x, y, m.dct_type)][il_luma_row(y, m.dct_type) * 8 + (x & 7u)]);
                }
            for (int pl = 0; pl < 2; ++pl) {                 // chroma: frame blocks always
                const size_t plane = (size_t)W * H + (size_t)pl * (W / 2) * (H / 2);
                for (int y = 0; y < 8; ++y)
                    for (int x = 0; x < 8; ++x) {
                        const int px = 8 * col + x, py = 8 * row + y;
                        const int32_t pred = m.intra ? 128 : il_predict(fwd + plane, bwd + plane, (int)W / 2, px, py, m, true);
                        cur[plane + (size_t)py * (W / 2) + px] = clip255(pred + res[4 + pl][y * 8 + x]);
                    }
            }
        }
        uint8_t *o = out.data() + (size_t)pics[p].display * R.frame_bytes;
        OutAt at{0, 0, 0, 0};
        for (uint32_t q = 0; q < (uint32_t)R.frame_bytes; ++q) {
            if (at.run > 1) out_step(at, layout); else at = out_locate(q, h.width, h.height, layout);
            o[q] = pic_sample(cur.data(), W, H, at);
        }
    }
    if (bad != kNone) return refuse(bad);
    R.out_bytes = out.size();
    return R;
}

}  // namespace dec_t_host
