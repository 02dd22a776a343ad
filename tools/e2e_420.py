"""tools/e2e_420.py — what 4:2:0 input buys on the port path and costs on the resident path, in one process, one JSON line.

Config c3's clip (1920x1152, 90 frames, 8 P frames), its content put through the module's own down-conversion (M.to420) so that the
4:4:4 route (the clip with its chroma repeated 2 x 2) and the 4:2:0 routes encode the same pictures.  Legs, A B C A B C in turn on
one handle, one GOP per call, the stream drained into the caller's buffer as it goes (as bench_e2e.py drives them):
  * m2v_push_frames_pull (4:4:4, 3 B/px) against m2v_push_frames420_pull with I420 and NV12 (1.5 B/px), page-locked source;
  * the same three from a pageable numpy array;
  * the box's plain pinned host-to-device rate, measured the way bench_e2e.py does, and every leg as a fraction of it at its own
    bytes per pixel;
  * resident: m2v_encode_resident420_begin / _end against m2v_encode_resident_begin / _end, two handles taking turns as bench.py
    times them, the two forms alternating on the same pair of handles.

    python tools/e2e_420.py [--rounds 5] [--steps 20] [--out FILE]
    python tools/e2e_420.py --once      # one short pass with k_expand420 and k_unpack444 launches of a GOP each: for a kernel trace
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, PF, GOPS = 1920, 1152, 8, 10
XL = YL = 7
VL, Q = 3, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every port leg (best of, >= 4 for a figure)")
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed resident pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true", help="one pass of the I420, NV12 and packed YUV24 legs, nothing timed")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()
    gop = PF + 1
    n = args.gops * gop
    xs, ys = W // 16, H // 16
    px = n * W * H
    src420 = {"i420": M.to420(M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0").cpu().numpy(), "i420")}     # the bench clip
    clip = M.to444(src420["i420"], W, H, "i420")
    src420["nv12"] = M.to420(clip, "nv12")
    outbuf = np.empty(px * 3 // 2 + 4096, np.uint8)

    def new_enc():
        enc = M.Mpeg2Encoder(XL, YL, VL, Q)
        enc.set_option("batch_frames", gop)
        return enc

    def run(enc, push):
        """one sequence, a GOP per call; push(k, pos) -> bytes pulled meanwhile.  -> seconds, stream"""
        t0 = time.perf_counter()
        pos = 0
        for k in range(0, n, gop):
            pos += push(k, pos)
        enc.sequence_stop()
        last = False
        while not last:
            m, last = enc.pull_into(outbuf, pos)
            pos += m
        return time.perf_counter() - t0, outbuf[:pos].tobytes()

    def leg444(enc, frames):
        return lambda: run(enc, lambda k, pos: enc.push_frames_pull(xs, ys, PF, frames[k:k + gop], outbuf, pos)[0])

    def leg420(enc, frames, layout):
        return lambda: run(enc, lambda k, pos: enc.push_frames420_pull(xs, ys, PF, frames[k:k + gop], outbuf, pos, layout)[0])

    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()          # noqa: E731
    pinned = {"444": pin(clip), "i420": pin(src420["i420"]), "nv12": pin(src420["nv12"])}

    if args.once:
        # the kernels side by side for a trace: k_expand420 (both forms) and k_unpack444, one launch per GOP of 9 frames each
        packed = pin(np.ascontiguousarray(clip.transpose(0, 2, 3, 1)).reshape(n, -1)).numpy()
        enc = new_enc()
        try:
            _, a = leg420(enc, pinned["i420"].numpy(), "i420")()
            _, b = leg420(enc, pinned["nv12"].numpy(), "nv12")()

            def push_packed(k, pos):
                enc.push_packed(xs, ys, PF, packed[k:k + gop], "yuv24")
                return enc.pull_into(outbuf, pos)[0]
            _, c = run(enc, push_packed)
        finally:
            enc.close()
        print(json.dumps({"once": True, "frames": n, "identical": a == b == c, "stream_bytes": len(a)}))
        return 0 if a == b == c else 1

    def alternate(legs, rounds):
        """legs: name -> callable; every leg once per round, in turn -> name -> (times, stream)"""
        res = {k: ([], None) for k in legs}
        for k, fn in legs.items():
            fn()                                                                    # warm-up: buffers, clocks
        for _ in range(rounds):
            for k, fn in legs.items():
                t, data = fn()
                res[k][0].append(t)
                res[k] = (res[k][0], data)
        return res

    # ONE handle for every leg, sequence after sequence: which hardware queues a handle's streams land on is the runtime's choice and
    # differs from handle to handle (three handles side by side gave the third one's legs 20 % less, whichever layout it was given)
    enc = new_enc()
    try:
        pinned_res = alternate({"444": leg444(enc, pinned["444"].numpy()), "i420": leg420(enc, pinned["i420"].numpy(), "i420"),
                                "nv12": leg420(enc, pinned["nv12"].numpy(), "nv12")}, args.rounds)
        page_res = alternate({"444": leg444(enc, clip), "i420": leg420(enc, src420["i420"], "i420"),
                              "nv12": leg420(enc, src420["nv12"], "nv12")}, args.rounds)
    finally:
        enc.close()

    # what the link gives a plain copy of page-locked bytes on this box (bench_e2e.py's measurement)
    dev_t = torch.empty_like(pinned["444"], device="cuda")
    dev_t.copy_(pinned["444"], non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        dev_t.copy_(pinned["444"], non_blocking=True)
    torch.cuda.synchronize()
    h2d = 4 * pinned["444"].numel() / (time.perf_counter() - t0)
    del dev_t

    bpp = {"444": 3.0, "i420": 1.5, "nv12": 1.5}

    def report(res):
        out = {}
        for k, (times, _) in res.items():
            best, worst = min(times), max(times)
            out[k] = {"GPixel_per_s": round(px / best * 1e-9, 2), "GPixel_per_s_slowest": round(px / worst * 1e-9, 2),
                      "spread": round((worst - best) / best, 4), "seconds": [round(t, 5) for t in times], "bytes_per_pixel": bpp[k],
                      "input_GBps": round(px * bpp[k] / best * 1e-9, 2), "fraction_of_measured_h2d": round(px * bpp[k] / best / h2d, 3)}
        for k in ("i420", "nv12"):
            out[k]["speedup_over_444"] = round(min(res["444"][0]) / min(res[k][0]), 3)
            # every repetition of the 4:2:0 leg beats every repetition of the 4:4:4 leg: faster by more than the run's spread
            out[k]["faster_than_444_beyond_spread"] = max(res[k][0]) < min(res["444"][0])
        return out

    streams = [r[k][1] for r in (pinned_res, page_res) for k in r]

    # ---- resident: two handles taking turns, 4:4:4 against I420 / NV12, alternating ----
    d_clip = torch.from_numpy(clip).to("cuda:0")
    d_420 = {k: torch.from_numpy(v).to("cuda:0") for k, v in src420.items()}
    cap = px * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
        h.set_option("split_streams", 1)
    torch.cuda.synchronize()

    def run_steps(steps, layout):
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
            if layout is None:
                pair[h].encode_resident_begin(d_clip.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF, 0)
            else:
                pair[h].encode_resident420_begin(d_420[layout].data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF, layout, 0)
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
        return nb

    res_t = {"444": [], "i420": [], "nv12": []}
    res_stream = {}
    try:
        for layout in (None, "i420", "nv12"):
            run_steps(6, layout)
        for _ in range(max(4, args.rounds)):
            for name, layout in (("444", None), ("i420", "i420"), ("nv12", "nv12")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nb = run_steps(args.steps, layout)
                torch.cuda.synchronize()
                res_t[name].append((time.perf_counter() - t0) / args.steps)
                res_stream[name] = d_outs[(args.steps - 1) & 1][:nb].cpu().numpy().tobytes()
    finally:
        for h in pair:
            h.close()
    streams += list(res_stream.values())
    resident = {k: {"GPixel_per_s": round(px / min(t) * 1e-9, 1), "ms_per_sequence": round(min(t) * 1e3, 4),
                    "spread": round((max(t) - min(t)) / min(t), 4)} for k, t in res_t.items()}
    for k in ("i420", "nv12"):
        resident[k]["time_ratio_to_444"] = round(min(res_t[k]) / min(res_t["444"]), 4)

    line = {"tool": "tools/e2e_420.py", "workload": "c3: %dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; chroma 2 x 2 constant" % (W, H, n, PF, VL, Q),
            "rounds": args.rounds, "pinned_h2d_GBps": round(h2d * 1e-9, 2),
            "all_streams_identical": all(s == streams[0] for s in streams), "stream_bytes": len(streams[0]),
            "page_locked_source": report(pinned_res), "pageable_source": report(page_res),
            "resident_two_handles": resident}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["all_streams_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
