// m2v_decode_streams.hpp — the layout of a batch of streams (m2v_decode_streams_device), computed on the host behind the plan's wait:
// where every stream's frames go, which streams do not fit, where the chunks are cut, and every chunk's picture table and step lists.
// Plain C++ without HIP types: m2v_decode_streams.hip and tools/dec_host.hpp call the same function, so the CPU build tests it.
// Include m2v_decode_kernels.hpp in front of it (not from here: the host build may take that header from another directory).
#pragma once
#include <stddef.h>

#include <vector>

namespace m2v {
namespace dec {

// what the probe stage (scan and plan: the headers and the grammar of the start codes) found of one stream
struct StreamInfo { int32_t status; uint32_t pictures, width, height; const uint8_t *types; };      // types: 1 = I, 2 = P, per picture

struct StreamsChunk {
    size_t first, count;                                     // its pictures in StreamsPlan::pics
    uint64_t mbs, buf_bytes, lo, hi;                         // macroblocks; bytes of its planar pictures, the carried slot in front; its range of the output
    uint32_t slices;
    bool carry_out;                                          // its last picture is the reference of the next chunk's first
    struct Step { size_t off, count; uint32_t most_mbs; };   // of StreamsPlan::list: entries of the chunk's table
    std::vector<Step> steps;
};

struct StreamsPlan {
    std::vector<uint64_t> out_offset;                        // per stream: the bytes of the accepted streams in front of it
    std::vector<uint8_t> overflow, cut;                      // per stream: its room does not lie inside cap; it lies in more than one chunk
    std::vector<ChunkPic> pics;                              // every picture that is decoded, in batch order: chunk after chunk
    std::vector<ChunkPic> pre;                               // the pictures of the cut streams (only slice0 and what a slice needs): walked first
    std::vector<uint32_t> list;
    std::vector<StreamsChunk> chunks;
    uint64_t carry = 0;                                      // the carried slot: the largest planar picture of the call
    uint32_t pre_slices = 0;
};

constexpr uint64_t kStreamsLevelBytes = 256ull << 20;        // the default chunk keeps its levels (768 bytes a macroblock) within this

// s[0 .. n): the streams in batch order.  probe: only the rooms (a call with d_dst == NULL).  decode_batch: pictures per chunk, 0: as
// many as keep the chunk's levels within level_bytes, counted from each picture's own macroblocks (one picture at least)
inline StreamsPlan plan_streams(const StreamInfo *s, size_t n, uint64_t cap, bool probe, size_t decode_batch, uint64_t level_bytes = kStreamsLevelBytes)
{
    StreamsPlan P;
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
    for (size_t b = 0; b < n; ++b) {
        if (s[b].status != kOk || P.overflow[b]) continue;
        ChunkPic c{};
        c.fb = frame_bytes(s[b].width, s[b].height);
        c.stream = (uint32_t)b; c.w = s[b].width; c.h = s[b].height; c.mbw = (c.w + 15u) / 16u; c.mbh = (c.h + 15u) / 16u;
        if (s[b].pictures) P.carry = P.carry > (uint64_t)c.mbw * c.mbh * 384u ? P.carry : (uint64_t)c.mbw * c.mbh * 384u;
        for (uint32_t p = 0; p < s[b].pictures; ++p) {
            c.pic = p; c.type = s[b].types[p]; c.out_off = P.out_offset[b] + p * c.fb;
            P.pics.push_back(c);
        }
    }
    for (size_t first = 0; first < P.pics.size();) {
        StreamsChunk C{};
        C.first = first;
        uint64_t buf = P.carry;
        std::vector<uint32_t> step;
        uint32_t deepest = 0;
        while (first + C.count < P.pics.size()) {
            ChunkPic &c = P.pics[first + C.count];
            const uint64_t m = (uint64_t)c.mbw * c.mbh;
            if (C.count && (decode_batch ? C.count >= decode_batch : (C.mbs + m) * 768u > level_bytes)) break;
            // a chain starts at its I picture, or at the chunk's first picture: then the reference is the carried slot
            const bool follows = C.count && P.pics[first + C.count - 1].stream == c.stream;
            c.slice0 = C.slices; c.mb_base = C.mbs; c.buf_off = buf;
            c.ref_off = follows ? P.pics[first + C.count - 1].buf_off : 0;
            step.push_back(follows && c.type != 1u ? step.back() + 1u : 0u);
            deepest = deepest > step.back() ? deepest : step.back();
            C.slices += c.mbh; C.mbs += m; buf += m * 384u;
            ++C.count;
        }
        C.buf_bytes = buf;
        C.lo = P.pics[first].out_off;
        C.hi = P.pics[first + C.count - 1].out_off + P.pics[first + C.count - 1].fb;
        for (uint32_t j = 0; j <= deepest; ++j) {
            StreamsChunk::Step S{P.list.size(), 0, 0};
            for (size_t k = 0; k < C.count; ++k) {
                if (step[k] != j) continue;
                const ChunkPic &c = P.pics[first + k];
                P.list.push_back((uint32_t)k);
                S.most_mbs = S.most_mbs > c.mbw * c.mbh ? S.most_mbs : c.mbw * c.mbh;
                ++S.count;
            }
            C.steps.push_back(S);
        }
        first += C.count;
        if (first < P.pics.size() && P.pics[first].stream == P.pics[first - 1].stream) {
            P.cut[P.pics[first].stream] = 1;
            C.carry_out = P.pics[first].type != 1u;
        }
        P.chunks.push_back(C);
    }
    // a stream that lies in several chunks would have its first pictures written before its last slices are walked: all its slices are
    // walked once in front of the chunks, for the verdict alone
    for (const ChunkPic &c : P.pics) {
        if (!P.cut[c.stream]) continue;
        ChunkPic q = c;
        q.slice0 = P.pre_slices;
        P.pre_slices += q.mbh;
        P.pre.push_back(q);
    }
    return P;
}

}  // namespace dec
}  // namespace m2v
