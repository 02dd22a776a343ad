"""tools/e2e_recon.py — what the reconstructed pictures out (m2v_set_recon_out) cost on the resident path, one JSON line.

The bench clip's recipe at 1920x1152, 10 GOPs of 1 I + 8 P frames, encoded on one pair of handles taking turns (as bench.py and
tools/e2e_stats.py time the resident entry) with no buffer set, with I420 out and with NV12 out, alternating, in one process.  The
three streams must be identical, and the two buffers must hold the same samples.  The cost has two parts: every GOP's last picture is
reconstructed too (one ninth more pictures with a reconstruction), and k_recon_out moves 3 bytes per pixel.

    python tools/e2e_recon.py [--rounds 4] [--steps 20] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/e2e_recon.py --once
                                    # two sequences from I420 frames with I420 out: k_expand420 in front, k_recon_out per GOP step;
                                    # --split-streams 1: every kernel on one stream, a launch holds a step's ten pictures
    python tools/e2e_recon.py --trace DIR --out FILE    # adds the kernel times of that trace (the second sequence) to FILE's JSON line
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
KINDS = ("k_recon_out", "k_expand420", "k_mb")
BYTES_PER_PIXEL = {"k_recon_out": 3.0, "k_expand420": 4.5}      # read + written


def from_trace(d, frames):
    """the k_recon_out / k_expand420 / k_mb dispatches of a --once run in time order -> microseconds (second sequence), and the two
    copies' time per byte moved"""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                kind = next((k for k in KINDS if k + "<" in name or k + "(" in name or name.endswith(k)), None)
                if kind:
                    rows.append((int(r["Start_Timestamp"]), kind, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    rows.sort()
    out = {"dispatches": {k: sum(1 for r in rows if r[1] == k) for k in KINDS}, "frames_per_sequence": frames}
    for k in KINDS:
        v = [us for _, kk, us in rows if kk == k]
        v = v[len(v) // 2:]                       # the second sequence
        if v:
            out[k + "_us_per_launch_mean"] = round(sum(v) / len(v), 2)
            out[k + "_us_per_sequence"] = round(sum(v), 2)
            if k in BYTES_PER_PIXEL:
                out[k + "_ps_per_byte"] = round(sum(v) * 1e6 / (frames * W * H * BYTES_PER_PIXEL[k]), 4)
    if "k_recon_out_us_per_sequence" in out:
        out["k_recon_out_us_per_gop_step"] = round(out["k_recon_out_us_per_sequence"] / (PF + 1), 2)
    if "k_recon_out_ps_per_byte" in out and "k_expand420_ps_per_byte" in out:
        out["per_byte_ratio_to_k_expand420"] = round(out["k_recon_out_ps_per_byte"] / out["k_expand420_ps_per_byte"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true", help="two sequences from I420 frames with I420 out, nothing timed: for a kernel trace")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --once: merge its kernel times into --out")
    ap.add_argument("--split-streams", type=int, default=None, help="option \"split_streams\" of both handles (1: every kernel of a sequence on one stream)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.gops * (PF + 1)
    if args.trace:
        line = json.loads(open(args.out).read()) if args.out and os.path.exists(args.out) else {"tool": "tools/e2e_recon.py"}
        line["kernel_trace"] = from_trace(args.trace, n)
        text = json.dumps(line)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return 0
    import torch
    import m2v_load
    M = m2v_load.load()
    xs, ys = W // 16, H // 16
    px = n * W * H
    fb = M.frame_bytes(W, H, "i420")
    clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0").contiguous()
    cap = n * W * H * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    d_recs = [torch.zeros(n * fb, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
        if args.split_streams is not None:
            h.set_option("split_streams", args.split_streams)
    torch.cuda.synchronize()

    def run_steps(steps, layout, src=None):
        """`steps` sequences on the two handles taking turns; layout None: no buffer set; src: I420 frames instead of the 4:4:4 clip"""
        for k, h in enumerate(pair):
            h.set_recon_out(d_recs[k].data_ptr() if layout else None, d_recs[k].numel(), layout or "i420")
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
            if src is None:
                pair[h].encode_resident_begin(clip.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF)
            else:
                pair[h].encode_resident420_begin(src.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF, "i420")
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
        last = (steps - 1) & 1
        return d_outs[last][:nb].cpu().numpy().tobytes(), d_recs[last]

    try:
        if args.once:
            src = torch.cat([clip[:, 0].reshape(n, -1), clip[:, 1, ::2, ::2].reshape(n, -1), clip[:, 2, ::2, ::2].reshape(n, -1)], dim=1).contiguous()
            torch.cuda.synchronize()
            a, _ = run_steps(1, "i420", src)
            b, rec = run_steps(1, "i420", src)
            print(json.dumps({"once": True, "frames": n, "identical": a == b, "written": bool(rec.any().item())}))
            return 0 if a == b else 1
        off, _ = run_steps(4, None)
        on_i, rec = run_steps(4, "i420")
        planes_i = [p.clone() for p in M.planes_of_recon(rec, W, H, "i420")]
        torch.cuda.synchronize()                  # (the copies run on torch's stream, the next sequences overwrite the buffer on the handles')
        on_n, rec = run_steps(4, "nv12")
        planes_n = M.planes_of_recon(rec, W, H, "nv12")
        same = off == on_i == on_n
        same_planes = all(bool(torch.equal(a, b)) for a, b in zip(planes_i, planes_n)) and bool(planes_i[0].any().item())
        names = (("off", None), ("i420", "i420"), ("nv12", "nv12"))
        times = {name: [] for name, _ in names}
        for _ in range(max(4, args.rounds)):
            for name, layout in names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, layout)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
    finally:
        for h in pair:
            h.close()
    best = {k: min(v) for k, v in times.items()}
    line = {"tool": "tools/e2e_recon.py",
            "workload": "%dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; two handles taking turns" % (W, H, n, PF, VL, Q),
            "rounds": max(4, args.rounds), "steps": args.steps,
            "off_ms_per_sequence": round(best["off"] * 1e3, 4), "i420_ms_per_sequence": round(best["i420"] * 1e3, 4),
            "nv12_ms_per_sequence": round(best["nv12"] * 1e3, 4),
            "time_ratio_i420": round(best["i420"] / best["off"], 4), "time_ratio_nv12": round(best["nv12"] / best["off"], 4),
            "off_GPixel_per_s": round(px / best["off"] * 1e-9, 1), "i420_GPixel_per_s": round(px / best["i420"] * 1e-9, 1),
            "spread": {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()},
            "streams_identical": bool(same), "i420_and_nv12_hold_the_same_samples": bool(same_planes)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and same_planes else 1


if __name__ == "__main__":
    sys.exit(main())
