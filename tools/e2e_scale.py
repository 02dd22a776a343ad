"""tools/e2e_scale.py — what resampling on the device (m2v_set_source_size, k_scale) costs on the resident path, one JSON line.

A 1920x1080 I420 clip (the bench clip's recipe, 90 frames, 8 P frames) coded at 1280x720 two ways on the same pair of handles taking
turns (as bench.py and tools/e2e_fit.py time the resident entry), in rotating order:
  * scaled:      the 1080-line frames with the source size set - k_scale resamples every chunk in front of its conversion;
  * prescaled:   the same clip resampled beforehand by the same definition (M.scale_frames: a second copy of the frames, at
                 1280x720) and passed with nothing set.
The two streams must be identical.  The ratio is the price of not keeping that second copy.

    python tools/e2e_scale.py [--rounds 4] [--steps 20] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/e2e_scale.py --once
                                    # one GOP of nine frames, twice: I420 and RGB24 scaled with either filter, and the same sources in
                                    # a fit-only sequence (1920x1080 padded to 1920x1088): k_scale beside k_fit
    python tools/e2e_scale.py --trace DIR --out FILE    # adds the kernel times of that trace (the second pass) to FILE's JSON line
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SW, SH, W, H, PF, GOPS = 1920, 1080, 1280, 720, 8, 10
XL = YL = 7
VL, Q = 3, 2
FILTERS = ("triangle", "area")


def frame_bytes(w, h, kind):
    return w * h * 3 if kind == "rgb24" else w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def from_trace(d):
    """the k_scale and k_fit dispatches of a --once run, in time order -> microseconds per GOP and nanoseconds per KB moved (source in,
    padded frame out), second pass"""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for k in ("k_scale", "k_fit"):
                    if k in r["Kernel_Name"]:
                        rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    rows.sort()
    sc = [us for _, k, us in rows if k == "k_scale"]
    fit = [us for _, k, us in rows if k == "k_fit"]
    out = {"dispatches": {"k_scale": len(sc), "k_fit": len(fit)}}
    gop = PF + 1
    if len(sc) == 8 and len(fit) == 8:      # per pass: k_scale I420 x 2 filters, RGB24 x 2 filters; k_fit 3 planes (I420), 1 plane (RGB24)
        sc, fit = sc[4:], fit[4:]
        moved = {"scale": {k: gop * (frame_bytes(SW, SH, k) + frame_bytes(W, H, k)) for k in ("i420", "rgb24")},
                 "fit": {k: gop * (frame_bytes(SW, SH, k) + frame_bytes(SW, 1088, k)) for k in ("i420", "rgb24")}}
        us = {"k_scale": {"i420": dict(zip(FILTERS, sc[0:2])), "rgb24": dict(zip(FILTERS, sc[2:4]))},
              "k_fit": {"i420": sum(fit[0:3]), "rgb24": fit[3]}}
        out["us_per_gop"] = {"k_scale": {k: {f: round(v, 2) for f, v in us["k_scale"][k].items()} for k in us["k_scale"]},
                             "k_fit": {k: round(v, 2) for k, v in us["k_fit"].items()}}
        out["bytes_moved_per_gop"] = moved
        per = {"k_fit": {k: us["k_fit"][k] * 1e3 / (moved["fit"][k] / 1024) for k in moved["fit"]},
               "k_scale": {k: {f: v * 1e3 / (moved["scale"][k] / 1024) for f, v in us["k_scale"][k].items()} for k in moved["scale"]}}
        out["ns_per_KB_moved"] = {"k_fit": {k: round(v, 3) for k, v in per["k_fit"].items()},
                                  "k_scale": {k: {f: round(v, 3) for f, v in per["k_scale"][k].items()} for k in per["k_scale"]}}
        out["k_scale_over_k_fit_per_byte"] = {k: {f: round(v / per["k_fit"][k], 2) for f, v in per["k_scale"][k].items()} for k in per["k_scale"]}
        out["allowed"] = 3.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true", help="two passes of one GOP per format and filter, nothing timed: for a kernel trace")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --once: merge its kernel times into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace:
        line = json.loads(open(args.out).read()) if args.out and os.path.exists(args.out) else {"tool": "tools/e2e_scale.py"}
        line["kernel_trace"] = from_trace(args.trace)
        text = json.dumps(line)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return 0
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    gop = PF + 1
    n = (1 if args.once else args.gops) * gop
    xs, ys = M.fit_size(W, H)
    assert (16 * xs, 16 * ys) == (W, H)
    full = M.synth.clip_torch(SW, 1088, n, clip_index=0, device="cuda:0")[:, :, :SH, :SW].contiguous()       # [n, 3, 1080, 1920]
    y, c = full[:, 0], full[:, 1:, ::2, ::2]
    src = {"i420": torch.cat([y.reshape(n, -1), c.reshape(n, -1)], dim=1).contiguous(),
           "rgb24": full.permute(0, 2, 3, 1).contiguous().reshape(n, -1)}
    for k in src:
        assert src[k].shape[1] == M.frame_bytes(SW, SH, k)
    cap = n * SW * 1088 * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
        h.set_option("split_streams", 1)
    torch.cuda.synchronize()

    def begin(h, kind, t, xs, ys):
        a = (t.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF)
        if kind == "i420":
            pair[h].encode_resident420_begin(*a, "i420")
        else:
            pair[h].encode_resident_rgb_begin(*a, "rgb24", "bt601")

    def run_steps(steps, kind, t, source=None, fit=None, size=(W, H)):
        """`steps` sequences of the frames t, the two handles taking turns; source = (sw, sh, filter) and fit = (w, h) are set first"""
        for h in pair:
            h.set_frame_size(*(fit or (0, 0)))
            h.set_source_size(*(source or (0, 0)))
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
            begin(h, kind, t, *M.fit_size(*size))
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
        return d_outs[(steps - 1) & 1][:nb].cpu().numpy().tobytes()

    try:
        if args.once:
            for _ in range(2):
                for kind in ("i420", "rgb24"):
                    for f in FILTERS:
                        run_steps(1, kind, src[kind], source=(SW, SH, f))
                for kind in ("i420", "rgb24"):
                    run_steps(1, kind, src[kind], fit=(SW, SH), size=(SW, SH))
            print(json.dumps({"once": True, "frames": n}))
            return 0
        # the second copy: the clip at 1280 x 720 by the numpy statement of the definition, a GOP at a time
        pre = torch.from_numpy(np.concatenate([M.scale_frames(src["i420"][k:k + gop].cpu().numpy(), SW, SH, W, H, "i420")
                                               for k in range(0, n, gop)])).to("cuda:0")
        same = run_steps(4, "i420", src["i420"], source=(SW, SH, "triangle")) == run_steps(4, "i420", pre)
        legs = (("prescaled", pre, None), ("scaled", src["i420"], (SW, SH, "triangle")))
        times = {name: [] for name, _, _ in legs}
        rounds = max(4, args.rounds)
        for r in range(rounds):
            for name, t, source in legs[r % 2:] + legs[:r % 2]:           # rotating order
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, "i420", t, source=source)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
    finally:
        for h in pair:
            h.close()
    a, b = min(times["scaled"]), min(times["prescaled"])
    px = n * W * H
    line = {"tool": "tools/e2e_scale.py",
            "workload": "%dx%d I420 coded at %dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d, triangle; two handles taking turns"
            % (SW, SH, W, H, n, PF, VL, Q), "rounds": rounds, "steps": args.steps,
            "resident": {"scaled_ms_per_sequence": round(a * 1e3, 4), "prescaled_ms_per_sequence": round(b * 1e3, 4), "time_ratio": round(a / b, 4),
                         "time_ratio_slowest_over_fastest": round(max(times["scaled"]) / b, 4),
                         "time_ratio_fastest_over_slowest": round(a / max(times["prescaled"]), 4),
                         "scaled_GPixel_per_s_of_picture": round(px / a * 1e-9, 1), "prescaled_GPixel_per_s_of_picture": round(px / b * 1e-9, 1),
                         "spread_scaled": round((max(times["scaled"]) - a) / a, 4), "spread_prescaled": round((max(times["prescaled"]) - b) / b, 4),
                         "ms_scaled": [round(t * 1e3, 4) for t in times["scaled"]], "ms_prescaled": [round(t * 1e3, 4) for t in times["prescaled"]],
                         "streams_identical": bool(same)}}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
