"""tools/e2e_gopcap.py — what the byte cap per GOP (option "gop_bytes_max", m2v_gop_report) costs on the resident path, one JSON line.

The bench clip's recipe at 1920x1152, 10 GOPs of 1 I + 8 P frames, encoded on one pair of handles taking turns (as bench.py and
tools/e2e_stats.py time the resident entry), alternating in one process:
  off      no cap: the parent's launches
  loose    a cap no GOP exceeds: k_gop_judge and one host wait per chunk, nothing encoded again
  median   a cap at the median GOP size of level 2: about half the GOPs are encoded once more, at level 3
The "off" and "loose" streams must be identical; the "median" stream must hold every GOP the report says, at the size it says.

    python tools/e2e_gopcap.py [--rounds 4] [--steps 20] [--out FILE]
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
LOOSE = 1 << 40


def gop_bytes(stream):
    """bytes of every GOP of a stream: from its group_start_code to the next one or to the sequence_end_code"""
    at, k = [], stream.find(b"\x00\x00\x01\xb8")
    while k >= 0:
        at.append(k)
        k = stream.find(b"\x00\x00\x01\xb8", k + 4)
    at.append(stream.rfind(b"\x00\x00\x01\xb7"))
    return [b - a for a, b in zip(at, at[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
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

    def run_steps(steps, B):
        for h in pair:
            h.set_option("gop_bytes_max", B)
        busy, nb, rec = [False, False], 0, None
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
                pair[h].gop_report()
            pair[h].encode_resident_begin(clip.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF)
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
                rec = pair[h].gop_report()
        return d_outs[(steps - 1) & 1][:nb].cpu().numpy().tobytes(), rec

    try:
        off, none = run_steps(4, 0)
        loose, rec2 = run_steps(4, LOOSE)
        B = int(np.sort(rec2["bytes"])[len(rec2) // 2])           # the median GOP size of level 2
        med, rec = run_steps(4, B)
        ok = (off == loose and len(none) == 0 and len(rec2) == args.gops and (rec2["tries"] == 1).all() and (rec2["level"] == Q).all()
              and gop_bytes(off) == list(rec2["bytes"]) and gop_bytes(med) == list(rec["bytes"])
              and all((r["bytes"] <= B) != bool(r["over"]) for r in rec))
        legs = (("off", 0), ("loose", LOOSE), ("median", B))
        times = {name: [] for name, _ in legs}
        for _ in range(max(4, args.rounds)):
            for name, b in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, b)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
    finally:
        for h in pair:
            h.close()
    best = {k: min(v) for k, v in times.items()}
    line = {"tool": "tools/e2e_gopcap.py",
            "workload": "%dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; two handles taking turns" % (W, H, n, PF, VL, Q),
            "rounds": max(4, args.rounds), "steps": args.steps, "median_cap_bytes": B,
            "gops_encoded_again": int((rec["tries"] > 1).sum()), "levels_under_median_cap": [int(v) for v in rec["level"]],
            "checks_ok": bool(ok)}
    for k in times:
        line[k + "_ms_per_sequence"] = round(best[k] * 1e3, 4)
        line[k + "_GPixel_per_s"] = round(px / best[k] * 1e-9, 1)
        line[k + "_spread"] = round((max(times[k]) - best[k]) / best[k], 4)
    line["loose_time_ratio"] = round(best["loose"] / best["off"], 4)
    line["median_time_ratio"] = round(best["median"] / best["off"], 4)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
