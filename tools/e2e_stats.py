"""tools/e2e_stats.py — what the per-picture statistics (option "stats", m2v_picture_stats) cost on the resident path, one JSON line.

The bench clip's recipe at 1920x1152, 10 GOPs of 1 I + 8 P frames, encoded on one pair of handles taking turns (as bench.py and
tools/e2e_fit.py time the resident entry) with the option off and on, alternating, in one process.  The two streams must be identical.
The cost has two parts: every GOP's last picture is reconstructed too (one ninth more pictures with a reconstruction), and k_picstat
reads source and reconstruction once, 4.5 bytes per pixel.

    python tools/e2e_stats.py [--rounds 4] [--steps 20] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/e2e_stats.py --once
                                    # two sequences with the option on: k_picstat per GOP step, k_picstat_mb per chunk
    python tools/e2e_stats.py --trace DIR --out FILE    # adds the kernel times of that trace (the second sequence) to FILE's JSON line
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

W, H, PF, GOPS = 1920, 1152, 8, 10
XL = YL = 7
VL, Q = 3, 2


def from_trace(d):
    """the k_picstat / k_picstat_mb / k_mb dispatches of a --once run in time order -> microseconds (second sequence)"""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                kind = "k_picstat_mb" if "k_picstat_mb" in name else "k_picstat" if "k_picstat" in name else "k_mb" if "k_mb<" in name else None
                if kind:
                    rows.append((int(r["Start_Timestamp"]), kind, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    rows.sort()
    out = {"dispatches": {k: sum(1 for r in rows if r[1] == k) for k in ("k_picstat", "k_picstat_mb", "k_mb")}}
    for k in ("k_picstat", "k_picstat_mb", "k_mb"):
        v = [us for _, kk, us in rows if kk == k]
        v = v[len(v) // 2:]                       # the second sequence
        if v:
            out[k + "_us_per_launch_mean"] = round(sum(v) / len(v), 2)
            out[k + "_us_per_sequence"] = round(sum(v), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true", help="two sequences with the option on, nothing timed: for a kernel trace")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --once: merge its kernel times into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace:
        line = json.loads(open(args.out).read()) if args.out and os.path.exists(args.out) else {"tool": "tools/e2e_stats.py"}
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
    n = args.gops * (PF + 1)
    xs, ys = W // 16, H // 16
    px = n * W * H
    clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0").contiguous()
    cap = n * W * H * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
    torch.cuda.synchronize()

    def run_steps(steps, stats):
        for h in pair:
            h.set_option("stats", int(stats))
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
                pair[h].picture_stats()
            pair[h].encode_resident_begin(clip.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF)
            busy[h] = True
        rec = None
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
                rec = pair[h].picture_stats()
        return d_outs[(steps - 1) & 1][:nb].cpu().numpy().tobytes(), rec

    try:
        if args.once:
            a, rec = run_steps(1, True)
            b, rec = run_steps(1, True)
            print(json.dumps({"once": True, "frames": n, "identical": a == b, "records": len(rec)}))
            return 0 if a == b and len(rec) == n else 1
        off, none = run_steps(4, False)
        on, rec = run_steps(4, True)
        same = off == on and len(none) == 0 and len(rec) == n
        times = {"off": [], "on": []}
        for _ in range(max(4, args.rounds)):
            for name, stats in (("off", False), ("on", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, stats)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
    finally:
        for h in pair:
            h.close()
    a, b = min(times["on"]), min(times["off"])
    y = M.psnr_from_sse(rec["sse"][:, 0], W * H)
    line = {"tool": "tools/e2e_stats.py",
            "workload": "%dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; two handles taking turns" % (W, H, n, PF, VL, Q),
            "rounds": max(4, args.rounds), "steps": args.steps,
            "stats_on_ms_per_sequence": round(a * 1e3, 4), "stats_off_ms_per_sequence": round(b * 1e3, 4), "time_ratio": round(a / b, 4),
            "stats_on_GPixel_per_s": round(px / a * 1e-9, 1), "stats_off_GPixel_per_s": round(px / b * 1e-9, 1),
            "spread_on": round((max(times["on"]) - a) / a, 4), "spread_off": round((max(times["off"]) - b) / b, 4),
            "streams_identical": bool(same), "luma_psnr_mean_dB": round(float(y.mean()), 3), "luma_psnr_min_dB": round(float(y.min()), 3)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
