"""tools/e2e_decode_streams_main.py — one m2v_decode_streams_main_device against a loop of m2v_decode_device with the options on, in one
process, one JSON line.  The streams are written by the test writers (tests/ilace_writer.py through tests/ilace_cases.py): there is no
other encoder of interlaced material with B pictures on the project's machines.

  * batch:  64 clips of nine 320 x 240 pictures, I B B P (coded I P B B P B B P B), progressive_sequence 0, frame_pred_frame_dct 0 with
            field prediction and field DCT, seeded content per clip; decoded clip by clip (64 calls of m2v_decode_device with
            "decode_syntax" = main, "decode_b_pictures" and "decode_interlaced" on) and in one call with flags 3, on one handle, in the
            same run, the frames asserted identical first.
  * ladder: one 30-picture stream at 720 x 576, 352 x 288 and 176 x 144: three calls against one.
Best and median of --rounds rounds, alternating, ms per call and the ratio loop / one call; the only condition is that the one call of
the batch is faster than the loop.

    python tools/e2e_decode_streams_main.py [--rounds 5] [--out FILE] [--no-ladder]
    python tools/e2e_decode_streams_main.py --once    # one call on the batch and nothing else: for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LETTERS = "IPBBPBBPB"


def written(w, h, letters, seed):
    import numpy as np
    import ilace_cases as I
    import ilace_writer as IW
    rng = np.random.RandomState(seed)
    return IW.stream(w, h, I.pictures(rng, letters, (w + 15) // 16, IW.mb_rows(h, 0), residual=4))[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-ladder", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def entry(loop_ms, one_ms):
        return {"loop_ms": [round(v, 3) for v in loop_ms], "loop_best_ms": round(min(loop_ms), 3), "loop_median_ms": round(statistics.median(loop_ms), 3),
                "one_call_ms": [round(v, 3) for v in one_ms], "one_call_best_ms": round(min(one_ms), 3), "one_call_median_ms": round(statistics.median(one_ms), 3),
                "ratio_best": round(min(loop_ms) / min(one_ms), 2), "ratio_median": round(statistics.median(loop_ms) / statistics.median(one_ms), 2)}

    def place(streams):
        seg, at = [], 0
        for s in streams:
            seg.append((at, len(s)))
            at += (len(s) + 31) // 32 * 32
        buf = np.zeros(at, np.uint8)
        for (a, n), s in zip(seg, streams):
            buf[a:a + n] = np.frombuffer(s, np.uint8)
        return torch.from_numpy(buf).to("cuda:0"), seg

    enc = M.Mpeg2Encoder(7, 7)

    def measure(streams):
        d_es, seg = place(streams)
        _, recs = enc.decode_streams(d_es, seg, syntax="main", b_pictures=True, interlaced=True)
        assert (recs["rec"]["status"] == 0).all(), "a written stream is refused"
        total = int((recs["out_offset"] + recs["rec"]["out_bytes"]).max())
        where = [(int(q["out_offset"]), int(q["rec"]["out_bytes"])) for q in recs]
        d_loop = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        d_one = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        for k, v in (("decode_syntax", 1), ("decode_b_pictures", 1), ("decode_interlaced", 1)):      # on the handle: the loop pays for no option change
            enc.set_option(k, v)

        def loop():
            for (a, n), (o, ob) in zip(seg, where):
                enc.decode_device(d_es[a:a + n], out=d_loop[o:o + ob], syntax="main", b_pictures=True, interlaced=True)

        def one():
            enc.decode_streams(d_es, seg, out=d_one, syntax="main", b_pictures=True, interlaced=True)

        return loop, one, d_loop, d_one, recs

    clips = 64
    streams = [written(320, 240, LETTERS, 100 + k) for k in range(clips)]
    loop, one, d_loop, d_one, recs = measure(streams)
    one()
    if args.once:
        torch.cuda.synchronize()
        print(json.dumps({"tool": "e2e_decode_streams_main", "once": True, "streams": clips, "pictures": int(recs["rec"]["pictures"].sum())}))
        return
    loop()
    torch.cuda.synchronize()
    assert torch.equal(d_one, d_loop), "one call and the loop disagree"
    loop_ms, one_ms = [], []
    for _ in range(args.rounds):                 # alternating, so that both see the same machine
        loop_ms.append(timed(loop))
        one_ms.append(timed(one))
    res = {"tool": "e2e_decode_streams_main",
           "batch": dict(entry(loop_ms, one_ms), clips=clips, pictures_per_clip=len(LETTERS), coded_order=LETTERS, size=[320, 240], es_bytes=sum(len(s) for s in streams))}
    assert min(one_ms) < min(loop_ms), "one call is not faster than the loop"
    if not args.no_ladder:
        sizes = [(720, 576), (352, 288), (176, 144)]
        letters = "IPBB" + "PBB" * 8 + "PB"
        assert len(letters) == 30
        ladder = [written(w, h, letters, 200 + k) for k, (w, h) in enumerate(sizes)]
        lloop, lone, d_lloop, d_lone, r = measure(ladder)
        assert [int(v) for v in r["rec"]["pictures"]] == [30] * 3
        lloop()
        lone()
        torch.cuda.synchronize()
        assert torch.equal(d_lone, d_lloop), "one call and three calls disagree on the ladder"
        a_ms, b_ms = [], []
        for _ in range(args.rounds):
            a_ms.append(timed(lloop))
            b_ms.append(timed(lone))
        res["ladder"] = dict(entry(a_ms, b_ms), pictures=30, sizes=[list(s) for s in sizes], es_bytes=[len(s) for s in ladder])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
