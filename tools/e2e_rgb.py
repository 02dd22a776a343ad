"""tools/e2e_rgb.py — what RGB input costs on the port path and on the resident path, in one process, one JSON line.

Config c3's geometry (1920x1152, 90 frames, 8 P frames); the clip's three planes taken as R, G, B.  The 4:4:4 route encodes
M.rgb_to444 of it (BT.601), so every route encodes the same pictures.  Legs, A B C A B C in turn on one handle, one GOP per call, the
stream drained into the caller's buffer as it goes (as tools/e2e_420.py drives them):
  * m2v_push_frames_pull (4:4:4, 3 B/px) against m2v_push_rgb_pull with RGB24 (3 B/px) and BGRX32 (4 B/px), page-locked source;
  * the same three from a pageable numpy array;
  * the box's plain pinned host-to-device rate, and every leg as a fraction of it at its own bytes per pixel;
  * resident: m2v_encode_resident_rgb_begin / _end with RGB24, BGRX32 and RGBP against m2v_encode_resident_begin / _end, two handles
    taking turns as bench.py times them, the forms alternating on the same pair of handles.

    python tools/e2e_rgb.py [--rounds 5] [--steps 20] [--out FILE] [--oracle]
    python tools/e2e_rgb.py --once [--gops 1]   # one short pass: k_rgb2yuv for RGB24, BGRX32, RGBP and its yardsticks k_unpack444<3>, <4>
                                                # on the same frames, a launch per GOP each: for a kernel trace
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
MATRIX = "bt601"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of every port leg (best of, >= 4 for a figure)")
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed resident pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true", help="one pass of the RGB24, BGRX32, RGBP and packed YUV24 / YUVX32 legs, nothing timed")
    ap.add_argument("--oracle", action="store_true", help="also hold the stream against the oracle's (minutes of CPU at the full length)")
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
    planes = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0").cpu().numpy()          # the bench clip, [n, 3, H, W], as R, G, B
    src = {"rgbp": planes.reshape(n, -1), "rgb24": np.ascontiguousarray(planes.transpose(0, 2, 3, 1)).reshape(n, -1)}
    bgrx = np.full((n, H, W, 4), 255, np.uint8)
    for c in range(3):
        bgrx[..., 2 - c] = planes[:, c]
    src["bgrx"] = bgrx.reshape(n, -1)
    del bgrx
    clip = M.rgb_to444(src["rgbp"], W, H, "rgbp", MATRIX)
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

    def leg_rgb(enc, frames, layout):
        return lambda: run(enc, lambda k, pos: enc.push_rgb_pull(xs, ys, PF, frames[k:k + gop], outbuf, pos, layout, MATRIX)[0])

    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()          # noqa: E731

    if args.once:
        # the kernels side by side for a trace: k_rgb2yuv (24-bit, 32-bit, planar) and k_unpack444 (24-bit, 32-bit) on the same frames
        yuv24 = np.ascontiguousarray(clip.transpose(0, 2, 3, 1))
        yuvx = np.zeros((n, H, W, 4), np.uint8)
        yuvx[..., :3] = yuv24
        enc = new_enc()
        try:
            got = [leg_rgb(enc, pin(src[l]).numpy(), l)()[1] for l in ("rgb24", "bgrx", "rgbp")]
            for packed, name in ((pin(yuv24.reshape(n, -1)).numpy(), "yuv24"), (pin(yuvx.reshape(n, -1)).numpy(), "yuvx32")):
                def push_packed(k, pos):
                    enc.push_packed(xs, ys, PF, packed[k:k + gop], name)
                    return enc.pull_into(outbuf, pos)[0]
                got.append(run(enc, push_packed)[1])
        finally:
            enc.close()
        same = all(g == got[0] for g in got)
        print(json.dumps({"once": True, "frames": n, "identical": same, "stream_bytes": len(got[0])}))
        return 0 if same else 1

    pinned = {"444": pin(clip), "rgb24": pin(src["rgb24"]), "bgrx": pin(src["bgrx"])}

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

    # ONE handle for every leg, sequence after sequence (tools/e2e_420.py says why)
    enc = new_enc()
    try:
        pinned_res = alternate({"444": leg444(enc, pinned["444"].numpy()), "rgb24": leg_rgb(enc, pinned["rgb24"].numpy(), "rgb24"),
                                "bgrx": leg_rgb(enc, pinned["bgrx"].numpy(), "bgrx")}, args.rounds)
        page_res = alternate({"444": leg444(enc, clip), "rgb24": leg_rgb(enc, src["rgb24"], "rgb24"),
                              "bgrx": leg_rgb(enc, src["bgrx"], "bgrx")}, args.rounds)
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

    bpp = {"444": 3.0, "rgb24": 3.0, "bgrx": 4.0}

    def report(res):
        out = {}
        for k, (times, _) in res.items():
            best, worst = min(times), max(times)
            out[k] = {"GPixel_per_s": round(px / best * 1e-9, 2), "GPixel_per_s_slowest": round(px / worst * 1e-9, 2),
                      "spread": round((worst - best) / best, 4), "seconds": [round(t, 5) for t in times], "bytes_per_pixel": bpp[k],
                      "input_GBps": round(px * bpp[k] / best * 1e-9, 2), "fraction_of_measured_h2d": round(px * bpp[k] / best / h2d, 3)}
        for k in ("rgb24", "bgrx"):
            out[k]["rate_ratio_to_444"] = round(min(res["444"][0]) / min(res[k][0]), 4)
        return out

    streams = [r[k][1] for r in (pinned_res, page_res) for k in r]
    del pinned

    # ---- resident: two handles taking turns, 4:4:4 against RGB24 / BGRX32 / RGBP, alternating ----
    d_clip = torch.from_numpy(clip).to("cuda:0")
    d_rgb = {k: torch.from_numpy(v).to("cuda:0") for k, v in src.items()}
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
                pair[h].encode_resident_rgb_begin(d_rgb[layout].data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF, layout, MATRIX, 0)
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
        return nb

    forms = (("444", None), ("rgb24", "rgb24"), ("bgrx", "bgrx"), ("rgbp", "rgbp"))
    res_t = {name: [] for name, _ in forms}
    res_stream = {}
    try:
        for _, layout in forms:
            run_steps(6, layout)
        for _ in range(max(4, args.rounds)):
            for name, layout in forms:
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
    for k in ("rgb24", "bgrx", "rgbp"):
        resident[k]["time_ratio_to_444"] = round(min(res_t[k]) / min(res_t["444"]), 4)

    line = {"tool": "tools/e2e_rgb.py", "workload": "c3's geometry: %dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; matrix %s" % (W, H, n, PF, VL, Q, MATRIX),
            "rounds": args.rounds, "pinned_h2d_GBps": round(h2d * 1e-9, 2),
            "all_streams_identical": all(s == streams[0] for s in streams), "stream_bytes": len(streams[0]),
            "page_locked_source": report(pinned_res), "pageable_source": report(page_res),
            "resident_two_handles": resident}
    if args.oracle:
        from oracle import m2v_oracle_ctypes as orc
        line["identical_to_oracle"] = streams[0] == orc.encode(clip, xs, ys, PF, XL, YL, VL, Q)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if line["all_streams_identical"] and line.get("identical_to_oracle", True) else 1


if __name__ == "__main__":
    sys.exit(main())
