"""tools/e2e_demux.py — what demultiplexing on the device costs a caller, in one process, one JSON line.

  * c3:     the stream of the bench clip (1920 x 1152, 90 frames, 8 P frames, Q_LEVEL 2) muxed on the device to a transport and to a
            program stream (about 17 MB each); m2v_demux_device of each, best and median of several rounds, beside a device-to-device
            copy of the same container timed the same way.  The result is held against the elementary stream, byte for byte.
  * decode: demux + decode of the container (decode_device(container=)) beside the decode of the bare stream on the same handle,
            alternating: what share of a decode the demux is.
  * batch:  64 clips x 9 frames of 320 x 240 (tools/e2e_batch.py's workload A) muxed per clip, demultiplexed as one call against one call
            per container.
ms per call; there is no threshold.

    python tools/e2e_demux.py [--rounds 5] [--out FILE]
    python tools/e2e_demux.py --once     # per kind one device-to-device copy of the container and one demux: for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, PF, GOPS = 1920, 1152, 8, 10
XL = YL = 7
VL, Q = 3, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()
    n = args.gops * (PF + 1)
    xs, ys = W // 16, H // 16
    d_clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0")
    d_es = torch.empty(n * W * H * 3 // 2, dtype=torch.uint8, device="cuda:0")
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)
    enc.set_option("batch_frames", n)
    nb = enc.encode_resident(d_clip.data_ptr(), n, d_es.data_ptr(), d_es.numel(), xs, ys, PF)
    es = d_es[:nb]
    info, _ = M.container.scan(es.cpu().numpy().tobytes())
    boxes = {}
    for kind in ("ts", "ps"):
        out, rec = enc.mux_device(es, kind, pictures=n)
        assert int(rec["status"][0]) == 0
        boxes[kind] = out[:int(rec["out_bytes"][0])].clone()
    d_out = torch.empty(M.demux_bound([max(b.numel() for b in boxes.values())]), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def demux(kind):
        _, rec = enc.demux_device(boxes[kind], kind, out=d_out)
        return rec

    for kind in ("ts", "ps"):
        rec = demux(kind)
        assert int(rec["status"][0]) == 0 and torch.equal(d_out[:int(rec["out_bytes"][0])], es[:info.bytes]), "the demultiplexed stream is not the muxed one"
    if args.once:
        for kind in ("ts", "ps"):
            d_copy = torch.empty_like(boxes[kind])
            d_copy.copy_(boxes[kind])
            demux(kind)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "e2e_demux", "once": True, "ts_bytes": boxes["ts"].numel(), "ps_bytes": boxes["ps"].numel()}))
        return

    def timed(fn, rounds):
        out = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out

    def summary(ms):
        return {"ms": [round(v, 4) for v in ms], "best_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4)}

    res = {"tool": "e2e_demux", "c3": {"frames": n, "es_bytes": int(info.bytes)}}
    for kind in ("ts", "ps"):
        d_copy = torch.empty_like(boxes[kind])
        res["c3"][kind] = {"bytes": boxes[kind].numel(), "demux": summary(timed(lambda: demux(kind), args.rounds)),
                           "copy": summary(timed(lambda: d_copy.copy_(boxes[kind]), args.rounds))}
    # the share of a decode: alternating on one handle
    fb = M.frame_bytes(W, H, "i420")
    d_dec = torch.empty(n * fb, dtype=torch.uint8, device="cuda:0")
    enc.decode_device(es, "i420", "module", out=d_dec)
    bare, boxed = [], {"ts": [], "ps": []}
    for _ in range(args.rounds):
        bare += timed(lambda: enc.decode_device(es, "i420", "module", out=d_dec), 1)
        for kind in ("ts", "ps"):
            boxed[kind] += timed(lambda: enc.decode_device(boxes[kind], "i420", "module", out=d_dec, container=kind), 1)
    res["decode"] = {"bare": summary(bare), "ts": summary(boxed["ts"]), "ps": summary(boxed["ps"])}
    # 64 small containers
    bw, bh, clips, per = 320, 240, 64, 9
    bclip = M.synth.clip_torch(bw, bh, clips * per, clip_index=3, device="cuda:0", scene_len=per).contiguous()
    benc = M.Mpeg2Encoder(XL, YL, VL, Q)
    benc.set_option("batch_frames", clips * per)
    benc.set_sequences([per] * clips)
    d_bes = torch.empty(clips * per * bw * bh * 3 // 2, dtype=torch.uint8, device="cuda:0")
    benc.encode_resident(bclip.data_ptr(), clips * per, d_bes.data_ptr(), d_bes.numel(), bw // 16, bh // 16, PF)
    seq = benc.sequence_report()
    segs = [(int(s["offset"]), int(s["bytes"])) for s in seq]
    res["batch"] = {"clips": clips, "frames_per_clip": per, "size": [bw, bh]}
    for kind in ("ts", "ps"):
        box, rec = benc.mux_device(d_bes, kind, segments=segs, pictures=clips * per)
        where = [(int(r["out_offset"]), int(r["out_bytes"])) for r in rec]
        assert all(int(r["status"]) == 0 for r in rec)
        d_bout = torch.empty(M.demux_bound([b for _, b in where]), dtype=torch.uint8, device="cuda:0")
        _, r = benc.demux_device(box, kind, segments=where, out=d_bout)
        assert all(int(v) == 0 for v in r["status"])

        def each():
            for w in where:
                benc.demux_device(box, kind, segments=[w], out=d_bout)

        res["batch"][kind] = {"bytes": sum(b for _, b in where), "one_call": summary(timed(lambda: benc.demux_device(box, kind, segments=where, out=d_bout), args.rounds)),
                              "call_per_container": summary(timed(each, args.rounds))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
