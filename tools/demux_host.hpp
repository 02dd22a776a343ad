// demux_host.hpp — the device demultiplexer's host build: csrc/m2v_demux_kernels.hpp behind a serial harness that does what the kernels of
// csrc/m2v_demux.hip do, step by step - find, tiles, plan, table, write - with the same functions.  tests/demux_cases.py compiles it into a
// library, tools/demux_host_check.cpp into a program of its own for the sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "m2v_demux_kernels.hpp"

namespace demux_host {

using namespace m2v::demux;

// the record of include/m2v_mi355x.h (m2v_demux_stat), field for field
struct Record { uint64_t src_offset, src_bytes, out_offset, out_bytes, err_offset; uint32_t pes_packets, packets, discontinuities, skipped, stream; int32_t status; };

// the first packet of `pid` that starts a section (k_ts_find looks 256 at a time; the answer is the first)
inline uint64_t find_psi(const uint8_t *src, uint64_t np, uint32_t pid)
{
    for (uint64_t k = 0; k < np; ++k)
        if (psi_match(src + 188 * k, pid)) return k;
    return kNone;
}

// One container as one call of m2v_demux_device sees it: the stream goes to out + 0 (out stands `lead` bytes past a 16-byte boundary;
// nullptr: the record only), at most cap bytes; stamps: at most stamp_cap.  Tiles are walked back to front: their order must not matter.
inline Record run(int kind, const uint8_t *src, uint64_t n, int stream, uint8_t *out, uint64_t cap, int lead, Stamp *stamps, uint64_t stamp_cap)
{
    State S{};
    S.src_bytes = n; S.want = stream; S.kind = (uint32_t)kind; S.err = kNone;
    const uint64_t np = n / 188;
    std::vector<Seg> segs;
    std::vector<Tile> tiles;
    if (kind == kTs) {
        S.ntiles = (uint32_t)((np + kTilePackets - 1) / kTilePackets);
        S.seg_cap = np + 1;
        segs.resize(S.seg_cap);
        tiles.resize(S.ntiles);
        // k_ts_find
        uint64_t err = ts_length_err(n);
        int v = kOk;
        uint32_t pid = stream < 0 ? kNoPid : (uint32_t)stream;
        if (stream < 0) {
            uint32_t program = 0, pmt = 0, video = 0;
            uint64_t k = find_psi(src, np, 0);
            v = k == kNone ? (int)kNoStream : pat_parse(src + 188 * k, program, pmt);
            if (v == kSyntax && 188 * k < err) err = 188 * k;
            if (v == kOk) {
                k = find_psi(src, np, pmt);
                v = k == kNone ? (int)kNoStream : pmt_parse(src + 188 * k, program, video);
                if (v == kSyntax && 188 * k < err) err = 188 * k;
                if (v == kOk) pid = video;
            }
        }
        S.found = v; S.pid = pid;
        if (err < S.err) S.err = err;
        // k_ts_tiles
        for (uint32_t t = S.ntiles; t-- > 0;) {
            Tile &T = tiles[t];
            tile_clear(T);
            uint32_t last_cc = 0;
            for (uint32_t i = 0; i < kTilePackets; ++i) {
                const uint64_t packet = (uint64_t)t * kTilePackets + i;
                if (packet >= np) break;
                const Pkt k = classify(src + 188 * packet, pid);
                if ((k.flags & (kBadSync | kViol)) && 188 * packet < S.err) S.err = 188 * packet;
                tile_add(T, k, i, packet, last_cc);
            }
        }
        // k_demux_plan
        ts_plan(S, tiles.data());
        if (S.status == kOk) segs[S.nseg] = Seg{0, S.out_bytes};
    } else {
        S.seg_cap = n / 9 + 2;
        segs.resize(S.seg_cap);
        ps_walk(S, src, segs.data());
    }
    Place P;
    place(S, P, cap, (uint64_t)lead);
    // k_demux_table
    if (S.status == kOk && kind == kPs) {
        for (uint64_t g = 0; g < S.nseg; ++g)
            if (S.stamp0 + g < stamp_cap) stamps[S.stamp0 + g] = stamp_of(segs[g], src);
    } else if (S.status == kOk) {
        for (uint32_t t = S.ntiles; t-- > 0;) {
            uint64_t o = tiles[t].out0, pes = S.stamp0 + tiles[t].pes0;
            for (uint32_t i = 0; i < kTilePackets; ++i) {
                const uint64_t packet = (uint64_t)t * kTilePackets + i;
                if (packet >= np) break;
                const Pkt k = classify(src + 188 * packet, S.pid);
                segs[packet] = ts_seg(k, packet, o);
                if (k.flags & kPusi) {
                    if (pes < stamp_cap) stamps[pes] = stamp_of(segs[packet], src);
                    ++pes;
                }
                o += ts_len(k, packet, S.first_pusi);
            }
        }
    }
    // k_demux_write
    for (uint64_t u = 0; out && u < P.units; ++u) {
        const long long q0 = (long long)(16 * u) - lead;
        const m2v::mux::Win w = gather16(segs.data(), S.nseg, S.out_bytes, src, n, q0);
        for (int k = 0; k < 16; ++k) {
            const long long q = q0 + k;
            if (q >= 0 && (uint64_t)q < S.out_bytes) out[q] = (uint8_t)((k < 8 ? w.lo : w.hi) >> (8 * (k & 7)));
        }
    }
    return Record{0, n, S.out_off, S.out_bytes, S.err, S.pes, S.packets, S.disc, S.skipped, S.pid, S.status};
}

}  // namespace demux_host
