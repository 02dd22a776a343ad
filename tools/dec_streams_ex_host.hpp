// dec_streams_ex_host.hpp — m2v_decode_streams_ex.hip run serially on a CPU: the same functions of csrc/m2v_decode_kernels.hpp, the same
// dec::plan_streams_main_ex, the same tables, slots, carried anchors, matrix table, spans and step lists, in the order of decisions of
// the device's launches - as tools/dec_streams_main_host.hpp runs m2v_decode_streams_main.hip.  flags: M2V_DECS_B_PICTURES (1) |
// M2V_DECS_INTERLACED (2) | M2V_DECS_EXTENDED (4) | M2V_DECS_MB_TOOLS (8); below 4 the call is dec_streams_main_host's, as the entry
// hands it on.  Plain C++ (g++ -I fpga-mpeg2-encoder_amd/csrc -I tools); used by tests/decstreams_ex_cases.py (as a shared library) and
// tools/dec_streams_ex_host_check.cpp (under the sanitizers).
#pragma once
#include "dec_streams_main_host.hpp"
#include "m2v_decode_streams_ex.hpp"

namespace dec_streams_ex_host {
using namespace m2v::dec;
using dec_host::Record;
using dec_host::Segment;
using dec_host::StreamRecord;

struct Pic { uint32_t type, slice0, params, nslices; XMats mats; };

// the probe stage of one stream: the scan and k_dsx_plan
struct Probed { Record R; MainPlan P; std::vector<uint64_t> ev; std::vector<Pic> pics; std::vector<uint8_t> types; std::vector<uint32_t> nslices; };

inline void probe(const uint8_t *es, uint64_t n, unsigned flags, Probed &Q)
{
    Record &R = Q.R;
    R = Record{};
    R.es_bytes = n;
    const bool b_pictures = (flags & 1u) != 0, interlaced = (flags & 2u) != 0, tools = (flags & 8u) != 0;
    auto refuse = [&](uint64_t at) { R.status = kSyntax; R.err_offset = at; R.out_bytes = 0; Q.pics.clear(); Q.types.clear(); Q.nslices.clear(); };
    if (n < 4) return refuse(0);                             // not one start code
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
    const uint32_t nev = (uint32_t)ev.size();
    MainPlan &P = Q.P;
    uint64_t bad = interlaced ? il_first(es, n, ev.data(), nev, P) : main_first(es, n, ev.data(), nev, P);
    if (bad != kNone) return refuse(bad);
    long lastI = -1;
    uint32_t anchors = 0;
    int prev = -1;
    XMats run{kNoEvent, kNoEvent};                           // the matrices in force in front of event i
    for (uint32_t i = 0; i < nev; ++i) {
        const EvInfo f = tools ? t_event(es, n, ev.data(), nev, i, P, last_nz, prev, b_pictures, interlaced)
                               : x_event(es, n, ev.data(), nev, i, P, last_nz, prev, b_pictures, interlaced);
        if (main_significant(main_role(es, n, ev[i]))) prev = (int)i;
        bad = min64(bad, f.bad);
        R.gops += f.gop; R.repeated_headers += f.rep;
        if (f.pic) {
            if (f.type == 1) { lastI = (long)Q.pics.size(); ++R.chains; }
            if (lastI < 0) bad = min64(bad, ev_pos(ev[i]));                  // a P picture without a reference
            if (f.type == 3 && anchors < 2) bad = min64(bad, ev_pos(ev[i]));  // a B picture without two anchors in front of it
            Pic q{f.type, 0, 0, 0, run};
            uint32_t quant;
            q.params = tools ? t_picture_params(es, n, ev.data(), nev, i, b_pictures, interlaced, P.seq.h.progressive, q.slice0, q.nslices, quant)
                             : x_picture_params(es, n, ev.data(), nev, i, b_pictures, interlaced, P.seq.h.progressive, q.slice0, q.nslices, quant);
            q.mats = x_mats_picture(es, n, ev.data(), nev, run, quant);
            if (f.type != 3) ++anchors;
            Q.pics.push_back(q);
            Q.types.push_back((uint8_t)f.type);
            Q.nslices.push_back(q.nslices);
        }
        x_mats_event(es, n, ev.data(), nev, i, run);
    }
    const SeqHdr &h = P.seq.h;
    R.width = h.width; R.height = h.height; R.pictures = (uint32_t)Q.pics.size();
    R.frame_bytes = frame_bytes(R.width, R.height);
    if (bad != kNone) refuse(bad);                           // (the device's record keeps the sizes of a stream its grammar refuses; they are not compared)
}

inline std::vector<ExStreamInfo> infos(const std::vector<Probed> &Q)
{
    std::vector<ExStreamInfo> info(Q.size());
    for (size_t b = 0; b < Q.size(); ++b)
        info[b] = ExStreamInfo{MainStreamInfo{Q[b].R.status, Q[b].R.pictures, Q[b].R.width, Q[b].R.height, Q[b].P.mbh, Q[b].types.data()}, Q[b].nslices.data()};
    return info;
}

// the slice events of a table's pictures, one after the other as the lanes of k_dsx_slices take them, then k_dsx_cont over their spans;
// store: into the chunk's records
inline void walk_slices(const Segment *seg, const std::vector<Probed> &Q, const MainChunkPic *tab, uint32_t ntab, uint32_t nslices, bool tools,
                        const std::vector<int32_t> &status, std::vector<uint64_t> &err, bool store, std::vector<IMb> &mb, std::vector<int32_t> &dc,
                        std::vector<int16_t> &lv)
{
    std::vector<uint32_t> spans(nslices, 0u);
    for (uint32_t g = 0; g < nslices; ++g) {
        const MainChunkPic &C = tab[main_chunk_slice_pic(tab, ntab, g)];
        if (status[C.stream] != kOk) continue;
        const Probed &S = Q[C.stream];
        const Pic &q = S.pics[C.pic];
        const uint32_t k = g - C.slice0, nev = (uint32_t)S.ev.size(), i = q.slice0 + k;
        if (k >= q.nslices || i >= nev) continue;
        const uint64_t start = ev_pos(S.ev[i]), end = i + 1 < nev ? ev_pos(S.ev[i + 1]) : seg[C.stream].n;
        const uint32_t code = ev_code(S.ev[i]);
        if (code < 1u || code > C.mbh) { err[C.stream] = min64(err[C.stream], start); continue; }
        std::vector<IMb> mb1;
        std::vector<int32_t> dc1;
        std::vector<int16_t> lv1;
        if (!store) { mb1.resize(C.mbw); dc1.resize((size_t)C.mbw * 6); lv1.resize((size_t)C.mbw * 384); }
        dec_i_host::Sink sink{store ? &mb : &mb1, store ? &dc : &dc1, store ? &lv : &lv1, store ? (size_t)C.mb_base + (size_t)(code - 1u) * C.mbw : 0};
        int c0, c1;
        const bool ok = tools ? t_slice(seg[C.stream].p, start, end, C.type, t_params_unpack(q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1)
                              : x_slice(seg[C.stream].p, start, end, C.type, il_params_unpack(q.params), (int)C.mbw, (int)C.mbh, (int)code - 1, sink, c0, c1);
        spans[g] = x_span_pack(ok, code, c0, c1);
        if (!ok) err[C.stream] = min64(err[C.stream], start);
    }
    for (uint32_t g = 0; g < nslices; ++g) {
        const MainChunkPic &C = tab[main_chunk_slice_pic(tab, ntab, g)];
        if (status[C.stream] != kOk) continue;
        const Probed &S = Q[C.stream];
        const Pic &q = S.pics[C.pic];
        const uint32_t k = g - C.slice0, cur = spans[g];
        if (!(cur >> 31) || k >= q.nslices || q.slice0 + k >= S.ev.size()) continue;
        if (!x_continuous(cur, k ? spans[g - 1] : 0u, k, q.nslices, C.mbw)) err[C.stream] = min64(err[C.stream], ev_pos(S.ev[q.slice0 + k]));
    }
}

// a picture's row of the matrix table (k_dsx_mats)
inline MainSeq matrices(const Segment &sg, const Probed &S, const Pic &q)
{
    MainSeq seq = S.P.seq;
    for (uint32_t t = 0; t < 64; ++t) {
        seq.wi[t] = (uint8_t)x_matrix_weight(sg.p, sg.n, S.ev.data(), (uint32_t)S.ev.size(), q.mats.mi, 0, t, S.P.seq.wi);
        seq.wn[t] = (uint8_t)x_matrix_weight(sg.p, sg.n, S.ev.data(), (uint32_t)S.ev.size(), q.mats.mn, 1, t, S.P.seq.wn);
    }
    return seq;
}

// one picture of a launch of k_dsx_recon
inline void recon(const MainChunkPic &c, const MainSeq &seq, uint32_t params, const std::vector<IMb> &mb, const std::vector<int32_t> &dc,
                  const std::vector<int16_t> &lv, std::vector<uint8_t> &buf)
{
    const uint32_t W = 16 * c.mbw, H = 16 * c.mbh;
    const PicParams pp = params_unpack(params);
    uint8_t *cur = buf.data() + c.buf_off;
    const uint8_t *fwd = buf.data() + c.fwd_off, *bwd = buf.data() + c.bwd_off;
    for (uint32_t k = 0; k < c.mbw * c.mbh; ++k) {
        const size_t at = c.mb_base + k;
        const IMb &m = mb[at];
        MainMb mm{};
        mm.intra = m.intra; mm.cbp = m.cbp; mm.qcode = m.qcode;
        const int col = (int)(k % c.mbw), row = (int)(k / c.mbw);
        int32_t res[6][64];
        for (int blk = 0; blk < 6; ++blk) dec_main_host::block_residual(mm, &dc[at * 6], &lv[at * 384], blk, seq, pp, res[blk]);
        for (uint32_t y = 0; y < 16; ++y)
            for (uint32_t x = 0; x < 16; ++x) {
                const int px = 16 * col + (int)x, py = 16 * row + (int)y;
                const int32_t pred = m.intra ? 128 : il_predict(fwd, bwd, (int)W, px, py, m, false);
                cur[(size_t)py * W + px] = clip255(pred + res[il_luma_block(x, y, m.dct_type)][il_luma_row(y, m.dct_type) * 8 + (x & 7u)]);
            }
        for (int pl = 0; pl < 2; ++pl) {
            const size_t plane = (size_t)W * H + (size_t)pl * (W / 2) * (H / 2);
            for (int y = 0; y < 8; ++y)
                for (int x = 0; x < 8; ++x) {
                    const int px = 8 * col + x, py = 8 * row + y;
                    const int32_t pred = m.intra ? 128 : il_predict(fwd + plane, bwd + plane, (int)W / 2, px, py, m, true);
                    cur[plane + (size_t)py * (W / 2) + px] = clip255(pred + res[4 + pl][y * 8 + x]);
                }
        }
    }
}

// out: cap bytes, or NULL for a probe.  decode_batch: option "decode_batch"; level_bytes: the bound of the default chunk
inline std::vector<StreamRecord> decode_streams(const Segment *seg, size_t n, int layout, unsigned flags, uint8_t *out, uint64_t cap, size_t decode_batch,
                                                uint64_t level_bytes = kStreamsLevelBytes)
{
    if (!(flags & 4u)) return dec_streams_main_host::decode_streams(seg, n, layout, flags, out, cap, decode_batch, level_bytes);
    const bool tools = (flags & 8u) != 0;
    std::vector<Probed> Q(n);
    for (size_t b = 0; b < n; ++b) probe(seg[b].p, seg[b].n, flags, Q[b]);
    const std::vector<ExStreamInfo> info = infos(Q);
    const MainStreamsPlan P = plan_streams_main_ex(info.data(), n, cap, out == nullptr, decode_batch, (flags & 1u) != 0, tools, level_bytes);
    std::vector<int32_t> status(n);
    std::vector<uint64_t> err(n, kNone);
    for (size_t b = 0; b < n; ++b) status[b] = Q[b].R.status;
    auto judge = [&]() { for (size_t b = 0; b < n; ++b) if (status[b] == kOk && err[b] != kNone) status[b] = kSyntax; };
    std::vector<IMb> mb;
    std::vector<int32_t> dc;
    std::vector<int16_t> lv;
    std::vector<uint8_t> buf;
    if (out && P.pre_slices) {
        walk_slices(seg, Q, P.pre.data(), (uint32_t)P.pre.size(), P.pre_slices, tools, status, err, false, mb, dc, lv);
        judge();
    }
    for (const MainStreamsChunk &C : P.chunks) {
        if (!out) break;
        const MainChunkPic *tab = P.pics.data() + C.first;
        mb.assign(C.mbs, IMb{}); dc.assign(C.mbs * 6, 0); lv.assign(C.mbs * 384, 0);
        buf.resize(std::max<size_t>(buf.size(), C.buf_bytes));
        walk_slices(seg, Q, tab, (uint32_t)C.count, C.slices, tools, status, err, true, mb, dc, lv);
        judge();
        auto launch = [&](const MainStreamsChunk::Step &S) {
            for (size_t y = 0; y < S.count; ++y) {
                const MainChunkPic &c = tab[P.list[S.off + y]];
                if (status[c.stream] != kOk) continue;
                const Pic &q = Q[c.stream].pics[c.pic];
                recon(c, matrices(seg[c.stream], Q[c.stream], q), q.params, mb, dc, lv, buf);
            }
        };
        for (const MainStreamsChunk::Step &S : C.steps) launch(S);
        launch(C.b);
        for (size_t k = 0; k < C.count; ++k) {                   // k_dsx_out: every picture at its own place
            const MainChunkPic &c = tab[k];
            if (status[c.stream] != kOk) continue;
            OutAt at{0, 0, 0, 0};
            for (uint32_t q = 0; q < (uint32_t)c.fb; ++q) {
                if (at.run > 1) out_step(at, layout); else at = out_locate(q, c.w, c.h, layout);
                out[c.out_off + q] = pic_sample(buf.data() + c.buf_off, 16 * c.mbw, 16 * c.mbh, at);
            }
        }
        if (C.carry0_from >= 0) memcpy(buf.data(), buf.data() + C.carry0_from, C.carry_bytes);
        if (C.carry1_from >= 0) memcpy(buf.data() + P.carry, buf.data() + C.carry1_from, C.carry_bytes);
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

}  // namespace dec_streams_ex_host
