"""tools/e2e_decode_streams_ex.py — one m2v_decode_streams_main_ex_device with flags 15 against a loop of m2v_decode_device with the four
options on, and - the yardstick - one m2v_decode_streams_main_device with flags 3 against its loop on ITS workload, in one process, one
JSON line.  The streams are written by the test writers: there is no other encoder of such material on the project's machines.

  * ex:    64 clips of nine 320 x 240 pictures, I B B P (coded I P B B P B B P B), progressive_sequence 0, frame_pred_frame_dct 0,
           intra_vlc_format 1, two slices a row wherever no skipped macroblock stands at the cut, one quant_matrix_extension at the
           first P picture (tests/mbt_writer.py), seeded content per clip.
  * main:  the 64 clips of tools/e2e_decode_streams_main.py (tests/ilace_writer.py): what the old entry's ratio was measured on.
Writing the clips takes minutes of Python and no GPU, so it is a step of its own:

    python tools/e2e_decode_streams_ex.py --write DIR                          # DIR/ex.bin, DIR/main.bin (no GPU)
    python tools/e2e_decode_streams_ex.py --measure DIR [--rounds 5] [--out FILE]
    python tools/e2e_decode_streams_ex.py --main-only DIR [--rounds 5]         # the old entry's one call alone (also with an older library)
    python tools/e2e_decode_streams_ex.py --once DIR                           # one call with flags 15 and nothing else: for a kernel trace
Rounds alternate between the loop and the one call; best and median, ms per call, the ratio loop / one call, and the new ratio as a
share of the old entry's in the same run (the aim is 0.8: the new path adds a matrix launch and a continuity launch a chunk).  The
frames of the one call and of the loop are asserted identical first.
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LETTERS = "IPBBPBBPB"
CLIPS, W, H = 64, 320, 240


def write(directory):
    import numpy as np
    import ext_cases as XC
    import ext_writer as XW
    import ilace_cases as I
    import ilace_writer as IW
    import main_cases as C
    import mbt_cases as T
    import mbt_writer as TW
    import e2e_decode_streams_main as OLD
    mbw, rows = (W + 15) // 16, IW.mb_rows(H, 0)
    ex = []
    for k in range(CLIPS):
        rng = np.random.RandomState(300 + k)
        pics = XC.cycle_cuts(I.pictures(rng, LETTERS, mbw, rows, residual=4), ((mbw // 2,),))
        pics[1]["extras"] = [XW.quant_ext(intra=C.MATRIX_A, non_intra=C.MATRIX_B)]
        ex.append(TW.stream(W, H, T.with_flags(pics, ivf=1))[0])
    old = [OLD.written(W, H, LETTERS, 100 + k) for k in range(CLIPS)]
    os.makedirs(directory, exist_ok=True)
    for name, streams in (("ex.bin", ex), ("main.bin", old)):
        with open(os.path.join(directory, name), "wb") as f:
            f.write(struct.pack("<I", len(streams)))
            for s in streams:
                f.write(struct.pack("<Q", len(s)) + s)
    print(json.dumps({"tool": "e2e_decode_streams_ex", "written": directory, "ex_bytes": sum(map(len, ex)), "main_bytes": sum(map(len, old))}))


def read(path):
    data = open(path, "rb").read()
    (n,), at, out = struct.unpack_from("<I", data), 4, []
    for _ in range(n):
        (m,) = struct.unpack_from("<Q", data, at)
        out.append(data[at + 8:at + 8 + m])
        at += 8 + m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None)
    ap.add_argument("--measure", default=None)
    ap.add_argument("--main-only", default=None)
    ap.add_argument("--once", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.write:
        return write(args.write)
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()

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

    def measure(streams, **kw):
        d_es, seg = place(streams)
        _, recs = enc.decode_streams(d_es, seg, syntax="main", b_pictures=True, interlaced=True, **kw)
        assert (recs["rec"]["status"] == 0).all(), "a written stream is refused"
        total = int((recs["out_offset"] + recs["rec"]["out_bytes"]).max())
        where = [(int(q["out_offset"]), int(q["rec"]["out_bytes"])) for q in recs]
        d_loop = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        d_one = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        options = [("decode_syntax", 1), ("decode_b_pictures", 1), ("decode_interlaced", 1)] + [("decode_" + k, 1) for k in kw]

        def loop():
            for (a, n), (o, ob) in zip(seg, where):
                enc.decode_device(d_es[a:a + n], out=d_loop[o:o + ob], syntax="main", b_pictures=True, interlaced=True, **kw)

        def timed_loop():                            # the options on the handle while the loop runs: it pays for no option change
            for k, v in options:
                enc.set_option(k, v)
            try:
                return timed(loop)
            finally:
                for k, v in options:
                    enc.set_option(k, 0)

        def one():
            enc.decode_streams(d_es, seg, out=d_one, syntax="main", b_pictures=True, interlaced=True, **kw)

        return timed_loop, one, d_loop, d_one, recs

    if args.main_only:
        streams = read(os.path.join(args.main_only, "main.bin"))
        loop, one, d_loop, d_one, recs = measure(streams)
        one()
        ms = [timed(one) for _ in range(args.rounds)]
        print(json.dumps({"tool": "e2e_decode_streams_ex", "main_only": True, "one_call_ms": [round(v, 3) for v in ms], "one_call_median_ms": round(statistics.median(ms), 3)}))
        return
    directory = args.measure or args.once
    ex = read(os.path.join(directory, "ex.bin"))
    loop, one, d_loop, d_one, recs = measure(ex, extended=True, mb_tools=True)
    one()
    if args.once:
        torch.cuda.synchronize()
        print(json.dumps({"tool": "e2e_decode_streams_ex", "once": True, "streams": len(ex), "pictures": int(recs["rec"]["pictures"].sum())}))
        return
    loop()
    torch.cuda.synchronize()
    assert torch.equal(d_one, d_loop), "one call and the loop disagree"
    old = read(os.path.join(directory, "main.bin"))
    oloop, oone, d_oloop, d_oone, orecs = measure(old)
    oone()
    oloop()
    torch.cuda.synchronize()
    assert torch.equal(d_oone, d_oloop), "one call and the loop disagree on the old entry's workload"
    a_ms, b_ms, c_ms, d_ms = [], [], [], []
    for _ in range(args.rounds):                     # alternating, so that all four see the same machine
        a_ms.append(loop())
        b_ms.append(timed(one))
        c_ms.append(oloop())
        d_ms.append(timed(oone))
    res = {"tool": "e2e_decode_streams_ex",
           "ex": dict(entry(a_ms, b_ms), clips=len(ex), pictures_per_clip=len(LETTERS), coded_order=LETTERS, size=[W, H], es_bytes=sum(len(s) for s in ex), flags=15),
           "main": dict(entry(c_ms, d_ms), clips=len(old), es_bytes=sum(len(s) for s in old), flags=3)}
    res["share_of_old_ratio_best"] = round(res["ex"]["ratio_best"] / res["main"]["ratio_best"], 3)
    res["share_of_old_ratio_median"] = round(res["ex"]["ratio_median"] / res["main"]["ratio_median"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
