"""tools/e2e_fit.py — what padding on the device (m2v_set_frame_size, k_fit) costs on the resident path, one JSON line.

A 1920x1080 clip (the bench clip's recipe, 90 frames, 8 P frames) as planar 4:4:4, I420 and RGB24, each encoded two ways on the same
pair of handles taking turns (as bench.py and tools/e2e_420.py time the resident entry), alternating:
  * fit:        the 1080-line frames with the size set - k_fit pads every chunk in front of its conversion;
  * prepadded:  the same clip padded to 1920x1088 beforehand (M.pad_frames' rule), no size set - today's way.
The two streams of a format must be identical.

    python tools/e2e_fit.py [--rounds 4] [--steps 20] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/e2e_fit.py --once
                                    # two passes of one GOP per format, 4:4:4 then I420 then RGB24: k_fit beside the conversions
    python tools/e2e_fit.py --trace DIR --out FILE    # adds the kernel times of that trace (the second pass) to FILE's JSON line
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

W0, H0, PF, GOPS = 1920, 1080, 8, 10
XL = YL = 7
VL, Q = 3, 2
KINDS = ("444", "i420", "rgb24")


def from_trace(d):
    """the k_fit / k_expand420 / k_rgb2yuv dispatches of a --once run, in time order -> microseconds per GOP and format (second pass)"""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                for k in ("k_fit", "k_expand420", "k_rgb2yuv"):
                    if k in name:
                        rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    rows.sort()
    fit = [us for _, k, us in rows if k == "k_fit"]
    out = {"dispatches": {k: sum(1 for r in rows if r[1] == k) for k in ("k_fit", "k_expand420", "k_rgb2yuv")}}
    if len(fit) == 14:             # per pass: 3 planes (4:4:4), 3 planes (I420), 1 plane (RGB24)
        f2 = fit[7:]
        out["k_fit_us_per_gop"] = {"444": round(sum(f2[0:3]), 2), "i420": round(sum(f2[3:6]), 2), "rgb24": round(f2[6], 2)}
        out["k_fit_us_per_launch"] = [round(v, 2) for v in f2]
    for k in ("k_expand420", "k_rgb2yuv"):
        v = [us for _, kk, us in rows if kk == k]
        if v:
            out[k + "_us_per_gop"] = round(v[-1], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true", help="two passes of one GOP per format, nothing timed: for a kernel trace")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --once: merge its kernel times into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace:
        line = json.loads(open(args.out).read()) if args.out and os.path.exists(args.out) else {"tool": "tools/e2e_fit.py"}
        line["kernel_trace"] = from_trace(args.trace)
        text = json.dumps(line)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return 0
    import torch
    import m2v_load
    M = m2v_load.load()
    gop = PF + 1
    n = (1 if args.once else args.gops) * gop
    xs, ys = M.fit_size(W0, H0)
    W, H = 16 * xs, 16 * ys
    px = n * W0 * H0
    full = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0")[:, :, :H0, :W0].contiguous()       # [n, 3, 1080, 1920]

    def pad_rows(t, rows):            # pad_frames' rule on the device, for planes whose width is whole already
        return torch.cat([t, t[..., -1:, :].expand(*t.shape[:-2], rows - t.shape[-2], t.shape[-1])], dim=-2).contiguous()

    src, pre = {}, {}
    src["444"], pre["444"] = full.reshape(n, -1), pad_rows(full, H).reshape(n, -1)
    y, c = full[:, 0], full[:, 1:, ::2, ::2]
    src["i420"] = torch.cat([y.reshape(n, -1), c.reshape(n, -1)], dim=1).contiguous()
    pre["i420"] = torch.cat([pad_rows(y, H).reshape(n, -1), pad_rows(c, H // 2).reshape(n, -1)], dim=1).contiguous()
    hwc = full.permute(0, 2, 3, 1).contiguous()
    src["rgb24"] = hwc.reshape(n, -1)
    pre["rgb24"] = torch.cat([hwc, hwc[:, -1:].expand(n, H - H0, W0, 3)], dim=1).contiguous().reshape(n, -1)
    for k in KINDS:
        assert src[k].shape[1] == M.frame_bytes(W0, H0, k) and pre[k].shape[1] == M.frame_bytes(W, H, k)
    cap = n * W * H * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
        h.set_option("split_streams", 1)
    torch.cuda.synchronize()

    def begin(h, kind, t):
        a = (t.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF)
        if kind == "444":
            pair[h].encode_resident_begin(*a)
        elif kind == "i420":
            pair[h].encode_resident420_begin(*a, "i420")
        else:
            pair[h].encode_resident_rgb_begin(*a, "rgb24", "bt601")

    def run_steps(steps, kind, fit):
        for h in pair:
            h.set_frame_size(W0 if fit else 0, H0 if fit else 0)
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
            begin(h, kind, (src if fit else pre)[kind])
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
        return d_outs[(steps - 1) & 1][:nb].cpu().numpy().tobytes()

    try:
        if args.once:
            same = True
            for _ in range(2):
                for kind in KINDS:
                    same &= run_steps(1, kind, True) == run_steps(1, kind, False)
            print(json.dumps({"once": True, "frames": n, "identical": bool(same)}))
            return 0 if same else 1
        times = {k: {"fit": [], "prepadded": []} for k in KINDS}
        same = {}
        for kind in KINDS:
            same[kind] = run_steps(4, kind, True) == run_steps(4, kind, False)
        for _ in range(max(4, args.rounds)):
            for kind in KINDS:
                for name, fit in (("prepadded", False), ("fit", True)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run_steps(args.steps, kind, fit)
                    torch.cuda.synchronize()
                    times[kind][name].append((time.perf_counter() - t0) / args.steps)
    finally:
        for h in pair:
            h.close()
    res = {}
    for kind in KINDS:
        a, b = min(times[kind]["fit"]), min(times[kind]["prepadded"])
        res[kind] = {"fit_ms_per_sequence": round(a * 1e3, 4), "prepadded_ms_per_sequence": round(b * 1e3, 4), "time_ratio": round(a / b, 4),
                     "fit_GPixel_per_s_of_source": round(px / a * 1e-9, 1), "prepadded_GPixel_per_s_of_source": round(px / b * 1e-9, 1),
                     "spread_fit": round((max(times[kind]["fit"]) - a) / a, 4), "spread_prepadded": round((max(times[kind]["prepadded"]) - b) / b, 4),
                     "streams_identical": bool(same[kind])}
    line = {"tool": "tools/e2e_fit.py", "workload": "%dx%d coded as %dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; two handles taking turns"
            % (W0, H0, W, H, n, PF, VL, Q), "rounds": max(4, args.rounds), "steps": args.steps, "resident": res}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
