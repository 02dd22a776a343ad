"""tools/e2e_decode_streams.py — one m2v_decode_streams_device against a loop of m2v_decode_device, in one process, one JSON line.

  * batch:  64 clips x 9 frames of 320 x 240 (tools/e2e_batch.py's workload A) encoded as a batch; decoded clip by clip (64 calls of
            m2v_decode_device) and in one call, on one handle, in the same run, the frames asserted identical first.
  * ladder: one 90-frame clip at 1920 x 1080, 1280 x 720 and 640 x 360 as three streams: three calls against one.
Best and median of --rounds rounds, ms per call and the ratio loop / one call; the only condition is that the one call of the batch is
not slower than the loop.

    python tools/e2e_decode_streams.py [--rounds 5] [--out FILE] [--no-ladder]
    python tools/e2e_decode_streams.py --once    # one call on the batch and nothing else: for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PF = 8
XL = YL = 7
VL, Q = 3, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-ladder", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()

    def timed(fn, rounds):
        out = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out

    def entry(loop_ms, one_ms):
        return {"loop_ms": [round(v, 3) for v in loop_ms], "loop_best_ms": round(min(loop_ms), 3), "loop_median_ms": round(statistics.median(loop_ms), 3),
                "one_call_ms": [round(v, 3) for v in one_ms], "one_call_best_ms": round(min(one_ms), 3), "one_call_median_ms": round(statistics.median(one_ms), 3),
                "ratio_best": round(min(loop_ms) / min(one_ms), 2), "ratio_median": round(statistics.median(loop_ms) / statistics.median(one_ms), 2)}

    # the batch: 64 clips of 9 frames, 320 x 240
    bw, bh, clips, per = 320, 240, 64, 9
    bclip = M.synth.clip_torch(bw, bh, clips * per, clip_index=3, device="cuda:0", scene_len=per).contiguous()
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)
    enc.set_option("batch_frames", clips * per)
    enc.set_sequences([per] * clips)
    d_es = torch.empty(clips * per * bw * bh * 3 // 2, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    enc.encode_resident(bclip.data_ptr(), clips * per, d_es.data_ptr(), d_es.numel(), bw // 16, bh // 16, PF)
    seq = enc.sequence_report()
    enc.set_sequences(None)
    assert len(seq) == clips
    seg = [(int(s["offset"]), int(s["bytes"])) for s in seq]
    fb = M.frame_bytes(bw, bh, "i420")
    d_loop = torch.zeros(clips * per * fb, dtype=torch.uint8, device="cuda:0")
    d_one = torch.zeros(clips * per * fb, dtype=torch.uint8, device="cuda:0")

    def loop():
        for k, (a, n) in enumerate(seg):
            enc.decode_device(d_es[a:a + n], "i420", "module", out=d_loop[k * per * fb:(k + 1) * per * fb])

    def one():
        return enc.decode_streams(d_es, seg, "i420", "module", out=d_one)

    _, recs = one()
    if args.once:
        torch.cuda.synchronize()
        print(json.dumps({"tool": "e2e_decode_streams", "once": True, "streams": clips, "pictures": int(recs["rec"]["pictures"].sum())}))
        return
    loop()
    torch.cuda.synchronize()
    assert (recs["rec"]["status"] == 0).all() and list(recs["out_offset"]) == [k * per * fb for k in range(clips)]
    assert torch.equal(d_one, d_loop), "one call and the loop disagree"
    loop_ms, one_ms = [], []
    for _ in range(args.rounds):                 # alternating, so that both see the same machine
        loop_ms += timed(loop, 1)
        one_ms += timed(one, 1)
    res = {"tool": "e2e_decode_streams", "batch": dict(entry(loop_ms, one_ms), clips=clips, frames_per_clip=per, size=[bw, bh])}
    assert min(one_ms) <= min(loop_ms), "one call is slower than the loop"
    if not args.no_ladder:
        n = 90
        y, x = torch.meshgrid(torch.arange(1080, device="cuda:0"), torch.arange(1920, device="cuda:0"), indexing="ij")
        t = torch.arange(n, device="cuda:0").reshape(n, 1, 1)
        top = torch.stack([(x + 3 * t) % 256, (y + 2 * t + x // 4) % 256, ((x + y) // 2 + 5 * t) % 256], dim=3).to(torch.uint8).contiguous()
        streams = []
        for w, h in ((1920, 1080), (1280, 720), (640, 360)):
            src = top if (w, h) == (1920, 1080) else top[:, ::1080 // h, ::1920 // w][:, :h, :w].contiguous()
            streams.append(enc.encode_tensor(src, PF, header="true").clone())
        sizes = [int(s.numel()) for s in streams]
        d_les = torch.cat(streams)
        lseg = [(sum(sizes[:k]), sizes[k]) for k in range(3)]
        _, r = enc.decode_streams(d_les, lseg, "i420", "module")
        assert (r["rec"]["status"] == 0).all() and [int(v) for v in r["rec"]["pictures"]] == [n] * 3
        total = int((r["out_offset"] + r["rec"]["out_bytes"]).max())
        d_lone = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        d_lloop = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        where = [(int(q["out_offset"]), int(q["rec"]["out_bytes"])) for q in r]

        def lloop():
            for (a, nb), (o, ob) in zip(lseg, where):
                enc.decode_device(d_les[a:a + nb], "i420", "module", out=d_lloop[o:o + ob])

        def lone():
            enc.decode_streams(d_les, lseg, "i420", "module", out=d_lone)

        lloop()
        lone()
        torch.cuda.synchronize()
        assert torch.equal(d_lone, d_lloop), "one call and three calls disagree on the ladder"
        a_ms, b_ms = [], []
        for _ in range(args.rounds):
            a_ms += timed(lloop, 1)
            b_ms += timed(lone, 1)
        res["ladder"] = dict(entry(a_ms, b_ms), frames=n, sizes=[[1920, 1080], [1280, 720], [640, 360]], es_bytes=sizes)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
