// m2v_decode_streams_main.hpp — the layout of a batch of main-syntax streams (m2v_decode_streams_main_device), computed on the host
// behind the plan's wait, as m2v_decode_streams.hpp does for the module's dialect.  New relative to plan_streams: the macroblock rows of
// a stream come from its plan (a sequence that is not progressive has 2 * ((height + 31) / 32)), a frame lies at its DISPLAY index
// inside its stream's room, a chunk's step lists hold its anchors and - one list behind them - its B pictures, and a stream cut at a
// chunk's edge carries its last TWO anchors in two slots in front of the chunk's buffer.
// Plain C++ without HIP types: m2v_decode_streams_main.hip and tools/dec_streams_main_host.hpp call the same function, so the CPU build
// tests it.  Include m2v_decode_kernels.hpp in front of it (not from here: the host build may take that header from another directory).
#pragma once
#include <stddef.h>

#include <vector>

namespace m2v {
namespace dec {

// what the probe stage found of one stream.  types: 1 = I, 2 = P, 3 = B, per picture in coded order; an accepted stream's B pictures
// have two anchors in front of them (the plan refuses the stream otherwise)
struct MainStreamInfo { int32_t status; uint32_t pictures, width, height, mbh; const uint8_t *types; };

// a chunk's picture: ChunkPic with the slots of both references.  fwd_off / bwd_off: the planar slot of the forward / backward anchor in
// the chunk's buffer - a slot of the chunk, or one of the two carried slots in front (0 and `carry`); an I picture's name slot 0 and are
// not read.  gpic: the picture's entry in the device's picture table (the stream's base + its coded index)
struct MainChunkPic {
    uint64_t out_off, fb;
    uint64_t buf_off, fwd_off, bwd_off;
    uint64_t mb_base;
    uint32_t stream, pic, gpic, slice0, type, mbw, mbh, w, h, pad;
};

template <class T>
M2V_HD inline uint32_t main_chunk_slice_pic(const T *t, uint32_t n, uint32_t g)
{
    uint32_t a = 0, b = n;
    while (b - a > 1u) { const uint32_t m = (a + b) / 2u; if (t[m].slice0 <= g) a = m; else b = m; }
    return a;
}

struct MainStreamsChunk {
    size_t first, count;                                     // its pictures in MainStreamsPlan::pics
    uint64_t mbs, buf_bytes;                                 // macroblocks; bytes of its planar pictures, the two carried slots in front
    uint32_t slices, most_units;                             // most_units: the 16-byte units of its largest frame
    struct Step { size_t off, count; uint32_t most_mbs; };   // of MainStreamsPlan::list: entries of the chunk's table
    std::vector<Step> steps;                                 // the anchors, chain step by chain step
    Step b;                                                  // every B picture of the chunk: one launch behind the anchors
    // behind the chunk, for the stream that goes on in the next: copy `bytes` from carry0_from to slot 0, then from carry1_from to slot 1
    // (offsets in the chunk's buffer; -1: that slot keeps what it holds)
    int64_t carry0_from, carry1_from;
    uint64_t carry_bytes;
};

struct MainStreamsPlan {
    std::vector<uint64_t> out_offset;
    std::vector<uint8_t> overflow, cut;
    std::vector<MainChunkPic> pics, pre;
    std::vector<uint32_t> list;
    std::vector<MainStreamsChunk> chunks;
    uint64_t carry = 0;                                      // one carried slot: the largest planar picture of the call
    uint32_t pre_slices = 0;
};

// the display index of every picture of a stream from its types: an anchor stands in front of the next anchor, a B picture one in front
// of its coded place (bp_display_anchor / bp_display_b); without B pictures the coded order.  b_pictures off: the coded order
inline void main_display(const uint8_t *types, uint32_t n, bool b_pictures, std::vector<uint32_t> &display)
{
    display.assign(n, 0);
    uint32_t next = n;
    for (uint32_t p = n; p-- > 0;) {
        if (!b_pictures) display[p] = p;
        else if (types[p] == 3u) display[p] = bp_display_b(p);
        else { display[p] = bp_display_anchor(next); next = p; }
    }
}

// s[0 .. n): the streams in batch order.  Arguments as plan_streams's; b_pictures: flag M2V_DECS_B_PICTURES
inline MainStreamsPlan plan_streams_main(const MainStreamInfo *s, size_t n, uint64_t cap, bool probe, size_t decode_batch, bool b_pictures,
                                         uint64_t level_bytes = kStreamsLevelBytes)
{
    MainStreamsPlan P;
    P.out_offset.assign(n, 0); P.overflow.assign(n, 0); P.cut.assign(n, 0);
    uint64_t at = 0;
    for (size_t b = 0; b < n; ++b) {
        P.out_offset[b] = at;
        if (s[b].status != kOk) continue;                    // refused at the probe stage: no room
        const uint64_t room = frame_bytes(s[b].width, s[b].height) * s[b].pictures;
        if (!probe && (at > cap || room > cap - at)) P.overflow[b] = 1;
        at += room;
    }
    if (probe) return P;
    std::vector<uint32_t> display;
    for (size_t b = 0; b < n; ++b) {
        if (s[b].status != kOk || P.overflow[b]) continue;
        MainChunkPic c{};
        c.fb = frame_bytes(s[b].width, s[b].height);
        c.stream = (uint32_t)b; c.w = s[b].width; c.h = s[b].height; c.mbw = (c.w + 15u) / 16u; c.mbh = s[b].mbh;
        if (s[b].pictures) P.carry = P.carry > (uint64_t)c.mbw * c.mbh * 384u ? P.carry : (uint64_t)c.mbw * c.mbh * 384u;
        main_display(s[b].types, s[b].pictures, b_pictures, display);
        for (uint32_t p = 0; p < s[b].pictures; ++p) {
            c.pic = p; c.type = s[b].types[p]; c.out_off = P.out_offset[b] + display[p] * c.fb;
            P.pics.push_back(c);
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
            c.bwd_off = c.type == 3u ? (uint64_t)(a1 < 0 ? 0 : a1) : 0u;
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
            C.slices += c.mbh; C.mbs += m; buf += m * 384u;
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
    for (const MainChunkPic &c : P.pics) {
        if (!P.cut[c.stream]) continue;
        MainChunkPic q = c;
        q.slice0 = P.pre_slices;
        P.pre_slices += q.mbh;
        P.pre.push_back(q);
    }
    return P;
}

}  // namespace dec
}  // namespace m2v
