// m2v_decode_streams_ex.hpp — the layout of a batch of main-syntax streams with the extended options (m2v_decode_streams_main_ex_device),
// computed on the host behind the plan's wait.  plan_streams_main_ex is plan_streams_main (m2v_decode_streams_main.hpp, whose structures
// these are) with two differences:
//   1. a picture's slices come from its stream's plan, not from its macroblock rows: with several slices in a row a picture has as many
//      slice events as its stream wrote, so a chunk's slice0 and slices, and pre_slices, are sums of the counts the device's plan left;
//   2. with mb_tools a P picture's bwd_off is its fwd_off - a dual-prime macroblock's record is a field-based one with both directions,
//      and its second prediction reads the same reference -, also where that reference is a carried slot.
// Plain C++ without HIP types: m2v_decode_streams_ex.hip and tools/dec_streams_ex_host.hpp call the same function, so the CPU build tests
// it.  Include m2v_decode_kernels.hpp in front of it (not from here: the host build may take that header from another directory).
#pragma once
#include "m2v_decode_streams_main.hpp"

namespace m2v {
namespace dec {

// MainStreamInfo and, per picture in coded order, the number of its slice events (an accepted stream's pictures have one at least)
struct ExStreamInfo { MainStreamInfo m; const uint32_t *nslices; };

// s[0 .. n): the streams in batch order.  Arguments as plan_streams_main's; mb_tools: flag M2V_DECS_MB_TOOLS
inline MainStreamsPlan plan_streams_main_ex(const ExStreamInfo *s, size_t n, uint64_t cap, bool probe, size_t decode_batch, bool b_pictures, bool mb_tools,
                                            uint64_t level_bytes = kStreamsLevelBytes)
{
    MainStreamsPlan P;
    P.out_offset.assign(n, 0); P.overflow.assign(n, 0); P.cut.assign(n, 0);
    uint64_t at = 0;
    for (size_t b = 0; b < n; ++b) {
        P.out_offset[b] = at;
        if (s[b].m.status != kOk) continue;                  // refused at the probe stage: no room
        const uint64_t room = frame_bytes(s[b].m.width, s[b].m.height) * s[b].m.pictures;
        if (!probe && (at > cap || room > cap - at)) P.overflow[b] = 1;
        at += room;
    }
    if (probe) return P;
    std::vector<uint32_t> display, nsl;                      // nsl: the slices of every picture of P.pics
    for (size_t b = 0; b < n; ++b) {
        const MainStreamInfo &m = s[b].m;
        if (m.status != kOk || P.overflow[b]) continue;
        MainChunkPic c{};
        c.fb = frame_bytes(m.width, m.height);
        c.stream = (uint32_t)b; c.w = m.width; c.h = m.height; c.mbw = (c.w + 15u) / 16u; c.mbh = m.mbh;
        if (m.pictures) P.carry = P.carry > (uint64_t)c.mbw * c.mbh * 384u ? P.carry : (uint64_t)c.mbw * c.mbh * 384u;
        main_display(m.types, m.pictures, b_pictures, display);
        for (uint32_t p = 0; p < m.pictures; ++p) {
            c.pic = p; c.type = m.types[p]; c.out_off = P.out_offset[b] + display[p] * c.fb;
            P.pics.push_back(c);
            nsl.push_back(s[b].nslices[p]);
        }
    }
    // the last two anchors of the stream that is being laid out, as places in the chunk's buffer: -1 none
    int64_t a1 = -1, a2 = -1;
    uint32_t a_stream = 0xFFFFFFFFu;
    for (size_t first = 0; first < P.pics.size();) {
        MainStreamsChunk C{};
        C.first = first;
        C.carry0_from = C.carry1_from = -1;
        uint64_t buf = 2 * P.carry;
        std::vector<int32_t> step;                           // per picture: an anchor's step, -1 for a B picture
        int32_t deepest = -1;
        int64_t prev_anchor = -1;                            // the chunk's last anchor of the stream being laid out (index in the chunk)
        // what the chunk in front left: the cut stream's anchors now lie in the carried slots (slot 1 the last one, slot 0 the one before)
        if (a1 >= 0) a1 = (int64_t)P.carry;
        if (a2 >= 0) a2 = 0;
        while (first + C.count < P.pics.size()) {
            MainChunkPic &c = P.pics[first + C.count];
            const uint64_t m = (uint64_t)c.mbw * c.mbh;
            if (C.count && (decode_batch ? C.count >= decode_batch : (C.mbs + m) * 768u > level_bytes)) break;
            if (c.stream != a_stream) { a_stream = c.stream; a1 = a2 = -1; prev_anchor = -1; }
            c.slice0 = C.slices; c.mb_base = C.mbs; c.buf_off = buf;
            c.fwd_off = c.type == 2u ? (uint64_t)(a1 < 0 ? 0 : a1) : c.type == 3u ? (uint64_t)(a2 < 0 ? 0 : a2) : 0u;
            c.bwd_off = c.type == 3u ? (uint64_t)(a1 < 0 ? 0 : a1) : c.type == 2u && mb_tools ? c.fwd_off : 0u;      // (dual prime: the forward reference again)
            if (c.type == 3u) step.push_back(-1);
            else {
                // a chain starts at its I picture, or at the stream's first anchor of the chunk: then the reference is a carried slot
                step.push_back(prev_anchor >= 0 && c.type != 1u ? step[(size_t)prev_anchor] + 1 : 0);
                deepest = deepest > step.back() ? deepest : step.back();
                prev_anchor = (int64_t)C.count;
                a2 = a1; a1 = (int64_t)buf;
            }
            const uint32_t units = (uint32_t)((c.fb + 15u) / 16u + 1u);
            C.most_units = C.most_units > units ? C.most_units : units;
            C.slices += nsl[first + C.count]; C.mbs += m; buf += m * 384u;
            ++C.count;
        }
        C.buf_bytes = buf;
        for (int32_t j = 0; j <= deepest; ++j) {
            MainStreamsChunk::Step S{P.list.size(), 0, 0};
            for (size_t k = 0; k < C.count; ++k) {
                if (step[k] != j) continue;
                const MainChunkPic &c = P.pics[first + k];
                P.list.push_back((uint32_t)k);
                S.most_mbs = S.most_mbs > c.mbw * c.mbh ? S.most_mbs : c.mbw * c.mbh;
                ++S.count;
            }
            C.steps.push_back(S);
        }
        C.b = MainStreamsChunk::Step{P.list.size(), 0, 0};
        for (size_t k = 0; k < C.count; ++k) {
            if (step[k] >= 0) continue;
            const MainChunkPic &c = P.pics[first + k];
            P.list.push_back((uint32_t)k);
            C.b.most_mbs = C.b.most_mbs > c.mbw * c.mbh ? C.b.most_mbs : c.mbw * c.mbh;
            ++C.b.count;
        }
        first += C.count;
        if (first < P.pics.size() && P.pics[first].stream == P.pics[first - 1].stream) {
            // the stream goes on: its last two anchors into slots 0 and 1 - slot 0 first (it may come from slot 1); an anchor that lies
            // where it has to stays.  Zero anchors of the stream in this chunk: nothing moves; one: slot 1 -> 0, the new one -> 1
            const MainChunkPic &L = P.pics[first - 1];
            P.cut[L.stream] = 1;
            C.carry_bytes = (uint64_t)L.mbw * L.mbh * 384u;
            if (a2 >= 0 && a2 != 0) C.carry0_from = a2;
            if (a1 >= 0 && a1 != (int64_t)P.carry) C.carry1_from = a1;
        } else {
            a_stream = 0xFFFFFFFFu; a1 = a2 = -1;            // no other stream ever reads the carried slots
        }
        P.chunks.push_back(C);
    }
    for (size_t k = 0; k < P.pics.size(); ++k) {
        if (!P.cut[P.pics[k].stream]) continue;
        MainChunkPic q = P.pics[k];
        q.slice0 = P.pre_slices;
        P.pre_slices += nsl[k];
        P.pre.push_back(q);
    }
    return P;
}

}  // namespace dec
}  // namespace m2v
