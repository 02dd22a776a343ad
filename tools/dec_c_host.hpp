// dec_c_host.hpp — the device decoder with damaged slices concealed (the c_ functions of csrc/m2v_decode_kernels.hpp, option
// "decode_conceal" on top of "decode_field_pictures" and what it stands on, "decode_join" 0 .. 3) run serially on a CPU, as
// tools/dec_j_host.hpp runs the plan for streams cut from a broadcast, in the order of decisions of m2v_decode_c.hip: dec_j_host's
// window and pairing; the plan over the window's events by c_event and c_place; the walk of every slice whose code names a row of its
// picture, each into the storage of that row ALONE - a heap block of exactly the row's records, DC values and levels, so that a walk
// that leaves its row is the sanitizer's to find -; the verdict per row from the picture's spans (c_row_kept) with the records of the
// concealed rows (c_record) and the counts, as k_dc_rows; and dec_f_host's reconstruction of every picture.  Plain C++; used by
// tests/conceal_cases.py (as a shared library) and tools/dec_c_host_check.cpp (under the sanitizers).
#pragma once
#include <memory>
#include "dec_j_host.hpp"

namespace dec_c_host {
using namespace m2v::dec;
using dec_host::Record;
using dec_f_host::Pic;
using dec_j_host::Join;

struct Conceal { uint64_t first_offset; uint32_t bad_slices, concealed_rows, grey_rows, damaged_pictures, reserved[2]; };

// the storage of one macroblock row, exactly: what a slice's walk may write
struct RowSink {
    IMb *mb_;
    int32_t *dc_;
    int16_t *lv_;
    void mb(int col, const IMb &m, const int32_t (&dc)[6])
    {
        mb_[col] = m;
        for (int k = 0; k < 6; ++k) dc_[col * 6 + k] = dc[k];
    }
    void level(int col, int blk, uint32_t i, int32_t l) { lv_[(col * 6 + blk) * 64 + (int)i] = (int16_t)l; }
};

inline Record decode(const uint8_t *es, uint64_t n, int layout, uint64_t cap, bool b_pictures, int join, std::vector<uint8_t> &out, Join &jr, Conceal &cr,
                     uint32_t lanes = 256)
{
    out.clear();
    Record R{};
    const uint64_t whole = n;
    R.es_bytes = whole;
    jr = Join{0, whole, 0, 0, {0, 0}};
    cr = Conceal{whole, 0, 0, 0, 0, {0, 0}};
    auto refuse = [&](uint64_t at) {
        R.status = kSyntax; R.err_offset = at; R.out_bytes = 0; out.clear();
        jr = Join{0, whole, 0, 0, {0, 0}}; cr = Conceal{whole, 0, 0, 0, 0, {0, 0}};
        return R;
    };
    if (n < 4) return refuse(0);                             // not one start code
    std::vector<uint64_t> ev0;
    uint64_t last_nz = 0;
    for (uint64_t p0 = 0; p0 < n; p0 += 16) {
        uint64_t w0, w1, w2;
        m2v::mux::load24(es, p0, n, w0, w1, w2);
        uint32_t cand = scan16(p0, n, w0, w1, w2, last_nz);
        while (cand) {
            const uint32_t j = (uint32_t)__builtin_ctz(cand);
            cand &= cand - 1u;
            ev0.push_back((p0 + j) << 8 | m2v::mux::byte24(w0, w1, w2, j + 3));
        }
    }
    const uint32_t nev0 = (uint32_t)ev0.size();
    const bool head = (join & (int)kJoinHead) != 0, tail = (join & (int)kJoinTail) != 0, drop = head && b_pictures;
    uint32_t jev = head ? nev0 : 0u;
    if (head) {                                              // J: a minimum over the lanes
        const uint32_t per0 = (nev0 + lanes - 1u) / lanes;
        for (uint32_t k = 0; k < lanes; ++k) {
            const uint32_t a0 = std::min(nev0, k * per0), b0 = std::min(nev0, a0 + per0);
            jev = std::min(jev, j_first_seq(ev0.data(), a0, b0));
        }
    }
    if (jev >= nev0 && (head || !nev0)) return refuse(0);
    const uint64_t *ev = ev0.data() + jev;                   // from here on an event's index counts from J's
    const uint32_t nw = nev0 - jev, per = (nw + lanes - 1u) / lanes;
    auto lo = [&](uint32_t k) { return std::min(nw, k * per); };
    auto hi = [&](uint32_t k) { return std::min(nw, lo(k) + per); };
    int lastsig = -1;
    for (uint32_t i = 0; i < nw; ++i) if (main_significant(main_role(es, n, ev[i]))) lastsig = (int)i;
    const bool cut = tail && !(lastsig >= 0 && main_role(es, n, ev[lastsig]) == rEnd);
    std::vector<JPair> pin(lanes, JPair{0, kNoEvent, 0});
    JScan t = j_scan_none();
    {
        std::vector<JSum> SA(lanes), SB(lanes);
        for (uint32_t k = 0; k < lanes; ++k) j_pair_range(es, n, ev, nw, lo(k), hi(k), b_pictures, SA[k], SB[k]);
        for (uint32_t k = 0; k < lanes; ++k) { pin[k] = t.in; j_pair_join(t, SA[k], SB[k]); }
    }
    const uint32_t F = cut ? t.f : kNoEvent, e2 = t.e2;
    uint32_t tw = F != kNoEvent ? F : nw;
    if (F != kNoEvent) {
        uint32_t s = 0;
        for (uint32_t k = 0; k < lanes; ++k) { const uint32_t sl = j_last_slice(ev, lo(k), std::min(hi(k), F)); if (sl != kNoEvent) s = std::max(s, sl); }
        for (uint32_t k = 0; k < lanes; ++k) tw = std::min(tw, j_first_head(ev, std::max(lo(k), s + 1u), std::min(hi(k), F + 1u)));
    }
    const uint32_t nev = tw;                                 // the window: events [0, tw), bytes [J, T)
    const uint64_t T = tw < nw ? ev_pos(ev[tw]) : n;
    if (tw < nw) last_nz = j_last_nz(es, T, ev, tw);
    n = T;                                                   // the window is read as a stream that ends at T
    MainPlan P{};
    uint64_t bad = head ? j_first(es, n, ev, nev, P) : il_first(es, n, ev, nev, P);
    if (bad != kNone) return refuse(bad);
    // every event by its own rule; the matrices in force in front of every event
    std::vector<XMats> mats(nev + 1u, XMats{kNoEvent, kNoEvent});
    int prev = -1;
    for (uint32_t i = 0; i < nev; ++i) {
        const EvInfo f = c_event(es, n, ev, nev, i, P, last_nz, prev, b_pictures);
        if (main_significant(main_role(es, n, ev[i]))) prev = (int)i;
        bad = min64(bad, f.bad);
        R.gops += f.gop; R.repeated_headers += f.rep;
        XMats run = mats[i];
        x_mats_event(es, n, ev, nev, i, run);
        mats[i + 1u] = run;
    }
    // the ranges' kept pictures, joined in order
    std::vector<JKeep> K(lanes);
    std::vector<FpRange> in(lanes);
    std::vector<uint32_t> cp0(lanes), sl0(lanes);
    for (uint32_t k = 0; k < lanes; ++k) j_keep_range(es, n, ev, nev, std::min(lo(k), tw), std::min(hi(k), tw), b_pictures, pin[k], e2, drop, K[k]);
    FpRange all = fp_range_none();
    uint32_t ncp = 0, nslices = 0, gone_frames = 0;
    for (uint32_t k = 0; k < lanes; ++k) {
        in[k] = all; cp0[k] = ncp; sl0[k] = nslices;
        fp_join(all, ncp, K[k].r, K[k].r, K[k].m);
        nslices += K[k].ns; gone_frames += K[k].dropped;
    }
    std::vector<Pic> pics(ncp);
    uint32_t lastopen = 0, lastpic = 0;
    for (uint32_t k = 0; k < lanes; ++k) {                   // every lane places its pictures behind the sums in front of its range
        const uint32_t a = std::min(lo(k), tw), b = std::min(hi(k), tw);
        FpRange s = in[k];
        JPair w = pin[k];
        bool gone = j_dropped(w, e2, drop);
        uint32_t cp = cp0[k], sl = sl0[k];
        for (uint32_t i = a; i < b; ++i) {
            const int role = main_role(es, n, ev[i]);
            if (role == rSlice) sl += !gone;
            if (w.open && (role == rSeq || role == rGop || role == rEnd)) bad = min64(bad, ev_pos(ev[i]));      // between the two fields of a frame
            uint32_t type, tref, ps;
            if (!fp_is_picture(es, n, ev, nev, i, b_pictures, type, tref, ps)) continue;
            bool wrong;
            gone = j_place(w, i, ps, type, tref, e2, drop, wrong);
            lastpic = i + 1u;
            if (w.open) lastopen = i + 1u;
            if (gone) { if (wrong) bad = min64(bad, ev_pos(ev[i])); continue; }
            const int32_t anchor_cp = s.a1cp;
            const FpPlace q = c_place(s, cp, ps, type, tref);
            if (q.bad) bad = min64(bad, ev_pos(ev[i]));
            Pic &pic = pics[cp];
            uint32_t quant;
            FPicParams pp = fp_picture_params(es, n, ev, nev, i, b_pictures, P.seq.h.progressive, pic.slice0, pic.nslices, quant);
            pp.second = q.second; pp.noref = q.second && type == 2u && q.fwd == kNoEvent;
            pic.ev = i; pic.type = type; pic.params = fp_params_pack(pp); pic.sbase = sl;
            pic.mats = x_mats_picture(es, n, ev, nev, mats[i], quant);
            pic.frame = q.frame; pic.fwd = q.fwd; pic.bwd = q.bwd; pic.display = 0;
            if (!q.second) {                                 // display order, by frames: a B frame at once, an anchor when the next one comes
                if (type == 3u) pic.display = bp_display_b(q.frame);
                else if (anchor_cp >= 0) pics[(size_t)anchor_cp].display = bp_display_anchor(q.frame);
            }
            ++cp;
        }
    }
    if (lastopen && lastopen == lastpic) bad = min64(bad, ev_pos(ev[lastopen - 1u]));      // a first field no picture follows
    if (all.a1cp >= 0) pics[(size_t)all.a1cp].display = bp_display_anchor(all.frames);
    if (bad != kNone) return refuse(bad);
    const SeqHdr &h = P.seq.h;
    const uint32_t nf = all.frames;
    R.width = h.width; R.height = h.height; R.pictures = nf; R.chains = all.ni;
    R.frame_bytes = frame_bytes(R.width, R.height);
    const uint32_t W = 16 * P.mbw, H = 16 * P.mbh, mbs = P.mbw * P.mbh, CW = W / 2, mbw = P.mbw;
    if (join) jr = Join{ev_pos(ev[0]), T, gone_frames, tw < nw ? 1u : 0u, {0, 0}};
    if (R.frame_bytes * nf > cap) { R.status = kOverflow; return R; }
    std::vector<IMb> mb(mbs);
    std::vector<int32_t> dc((size_t)mbs * 6);
    std::vector<int16_t> lv((size_t)mbs * 384);
    const size_t psz = (size_t)W * H * 3 / 2;
    std::vector<std::vector<uint8_t>> planes(nf);            // every frame (the streams of the tests are small)
    std::vector<uint32_t> spans(nslices + 1u);
    out.resize(R.frame_bytes * nf);
    for (size_t p = 0; p < pics.size(); ++p) {
        std::fill(lv.begin(), lv.end(), 0);
        std::fill(mb.begin(), mb.end(), IMb{});
        const FPicParams pp = fp_params_unpack(pics[p].params);
        const bool field = fp_is_field(pp.ps);
        const uint32_t rows = field ? P.mbh / 2u : P.mbh, par = field ? pp.ps - 1u : 0u;
        const uint32_t g0 = pics[p].sbase - pics[0].sbase;      // (kept slices alone are counted)
        for (uint32_t g = g0; g < g0 + pics[p].nslices; ++g) {  // the walk: every slice finds its picture as a lane does; one span per slice
            uint32_t k;
            const uint32_t at = x_slice_pic(pics.data(), (uint32_t)pics.size(), g, k);
            if (at != p || k != g - g0) return refuse(0);    // (the search found another picture: never, with or without slice-less pictures around)
            const uint32_t i = pics[p].slice0 + k, code = ev_code(ev[i]);
            int first = -1, last = -1;
            bool ok = !c_bad_code(code, rows);
            if (ok) {
                // the row's storage alone, exactly: its records as the walks in front left them
                std::unique_ptr<IMb[]> rmb(new IMb[mbw]);
                std::unique_ptr<int32_t[]> rdc(new int32_t[(size_t)mbw * 6]);
                std::unique_ptr<int16_t[]> rlv(new int16_t[(size_t)mbw * 384]);
                const size_t at0 = (size_t)(code - 1u) * mbw;
                std::copy(mb.begin() + at0, mb.begin() + at0 + mbw, rmb.get());
                std::copy(dc.begin() + at0 * 6, dc.begin() + (at0 + mbw) * 6, rdc.get());
                std::copy(lv.begin() + at0 * 384, lv.begin() + (at0 + mbw) * 384, rlv.get());
                RowSink sink{rmb.get(), rdc.get(), rlv.get()};
                const uint64_t end = i + 1 < nev ? ev_pos(ev[i + 1]) : n;
                ok = field ? fp_slice(es, ev_pos(ev[i]), end, pics[p].type, pp, (int)mbw, (int)rows, (int)code - 1, sink, first, last)
                           : t_slice(es, ev_pos(ev[i]), end, pics[p].type, pp.t, (int)mbw, (int)P.mbh, (int)code - 1, sink, first, last);
                std::copy(rmb.get(), rmb.get() + mbw, mb.begin() + at0);
                std::copy(rdc.get(), rdc.get() + (size_t)mbw * 6, dc.begin() + at0 * 6);
                std::copy(rlv.get(), rlv.get() + (size_t)mbw * 384, lv.begin() + at0 * 384);
            }
            spans[g] = x_span_pack(ok, code, first, last);
            cr.bad_slices += !ok;
        }
        {   // the rows: the verdict from the picture's spans, the records of a concealed row, the counts
            const bool grey = pics[p].fwd == kNoEvent;
            uint32_t hidden = 0;
            for (uint32_t r = 0; r < rows; ++r) {
                if (c_row_kept(spans.data() + g0, pics[p].nslices, r + 1u, mbw)) continue;
                for (uint32_t c = 0; c < mbw; ++c) mb[(size_t)r * mbw + c] = c_record(field, par, grey);
                ++hidden;
            }
            if (hidden) {
                cr.concealed_rows += hidden; cr.grey_rows += grey ? hidden : 0u; ++cr.damaged_pictures;
                cr.first_offset = std::min<uint64_t>(cr.first_offset, ev_pos(ev[pics[p].ev]));
            }
        }
        MainSeq seq = P.seq;                                 // the picture's row of the matrix table
        for (uint32_t t = 0; t < 64; ++t) {
            seq.wi[t] = (uint8_t)x_matrix_weight(es, n, ev, nev, pics[p].mats.mi, 0, t, P.seq.wi);
            seq.wn[t] = (uint8_t)x_matrix_weight(es, n, ev, nev, pics[p].mats.mn, 1, t, P.seq.wn);
        }
        std::vector<uint8_t> &cur = planes[pics[p].frame];
        if (!pp.second) cur.assign(psz, 0);
        const uint8_t *fwd = pics[p].fwd != kNoEvent ? planes[pics[p].fwd].data() : cur.data();
        const uint8_t *bwd = pics[p].bwd != kNoEvent ? planes[pics[p].bwd].data() : cur.data();
        // the frame that holds the field of parity q of direction d: the second field of an anchor frame finds the other parity in its own
        const bool own = field && pp.second && pics[p].type == 2u;
        const uint8_t *const ref[4] = {own && par != 0u ? cur.data() : fwd, own && par != 1u ? cur.data() : fwd,
                                       own && par != 0u ? cur.data() : bwd, own && par != 1u ? cur.data() : bwd};
        for (uint32_t k = 0; k < mbw * rows; ++k) {
            const IMb &q = mb[k];
            MainMb mm{};
            mm.intra = q.intra; mm.cbp = q.cbp; mm.qcode = q.qcode;
            const int col = (int)(k % mbw), row = (int)(k / mbw);
            int32_t res[6][64];
            for (int blk = 0; blk < 6; ++blk) dec_main_host::block_residual(mm, &dc[(size_t)k * 6], &lv[(size_t)k * 384], blk, seq, pp.t.i.b.p, res[blk]);
            for (uint32_t y = 0; y < 16; ++y)
                for (uint32_t x = 0; x < 16; ++x) {
                    const int px = 16 * col + (int)x, py = 16 * row + (int)y;
                    if (field) {                             // line py of the field is line 2 py + par of the frame
                        const int32_t pred = q.intra ? 128 : fp_predict(ref, (int)W, px, py, (int)(y >> 3), q, false);
                        cur[(size_t)(2 * py + (int)par) * W + px] = clip255(pred + res[(y >> 3) * 2u + (x >> 3)][(y & 7u) * 8 + (x & 7u)]);
                    } else {
                        const int32_t pred = q.intra ? 128 : il_predict(fwd, bwd, (int)W, px, py, q, false);
                        cur[(size_t)py * W + px] = clip255(pred + res[il_luma_block(x, y, q.dct_type)][il_luma_row(y, q.dct_type) * 8 + (x & 7u)]);
                    }
                }
            for (int pl = 0; pl < 2; ++pl) {
                const size_t plane = (size_t)W * H + (size_t)pl * CW * (H / 2);
                const uint8_t *const cref[4] = {ref[0] + plane, ref[1] + plane, ref[2] + plane, ref[3] + plane};
                for (int y = 0; y < 8; ++y)
                    for (int x = 0; x < 8; ++x) {
                        const int px = 8 * col + x, py = 8 * row + y;
                        if (field) {
                            const int32_t pred = q.intra ? 128 : fp_predict(cref, (int)CW, px, py, y >> 2, q, true);
                            cur[plane + (size_t)(2 * py + (int)par) * CW + px] = clip255(pred + res[4 + pl][y * 8 + x]);
                        } else {
                            const int32_t pred = q.intra ? 128 : il_predict(fwd + plane, bwd + plane, (int)CW, px, py, q, true);
                            cur[plane + (size_t)py * CW + px] = clip255(pred + res[4 + pl][y * 8 + x]);
                        }
                    }
            }
        }
        if (field && !pp.second) continue;                   // the frame is whole behind its second field
        size_t firstp = p;
        while (fp_params_unpack(pics[firstp].params).second) --firstp;      // (a second field's first field is the picture in front of it)
        uint8_t *o = out.data() + (size_t)pics[firstp].display * R.frame_bytes;
        OutAt at{0, 0, 0, 0};
        for (uint32_t q = 0; q < (uint32_t)R.frame_bytes; ++q) {
            if (at.run > 1) out_step(at, layout); else at = out_locate(q, h.width, h.height, layout);
            o[q] = pic_sample(cur.data(), W, H, at);
        }
    }
    R.out_bytes = out.size();
    return R;
}

}  // namespace dec_c_host
