"""tools/e2e_scenecut.py — what the cut detector (option "scene_cut", m2v_scene_report) costs on the resident path, and what a cut is
worth, one JSON line.

Cost: the bench clip's recipe at 1920x1152, 90 frames, 8 P frames per GOP, resident, alternating in one process:
  off      the option off: the parent's launches
  never    T = 65280, which no picture can exceed: k_mbsum, k_scene_judge and one host wait per chunk, and not one cut
on ONE handle (the wait is exposed) and on a pair of handles taking turns (the other handle's kernels cover it).  The "off" and
"never" streams must be identical, so the ratio is the detector plus its wait alone.

Worth: the same clip - the recipe has a scene change every 23 frames -, T = 3000 against the option off: stream bytes, luma PSNR from the
encoder's own records (option "stats"), and the time ratio.  Description, not a pass mark.

    python tools/e2e_scenecut.py [--rounds 4] [--steps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, PF, N = 1920, 1152, 8, 90
XL = YL = 7
VL, Q = 3, 2
NEVER, T_CUT, SCENE_LEN = 65280, 3000, 23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="sequences per timed pass")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    xs, ys = W // 16, H // 16
    px = N * W * H
    clip = M.synth.clip_torch(W, H, N, clip_index=0, device="cuda:0", scene_len=SCENE_LEN).contiguous()
    scenes = clip                       # (the recipe's own scene changes: one every 23 frames)
    cap = N * W * H * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", N)
    torch.cuda.synchronize()

    def run_steps(steps, T, src, handles=2):
        """`steps` sequences of src on `handles` handles taking turns -> (the last stream, its scene records)"""
        for h in pair:
            h.set_option("scene_cut", T)
        busy, nb, rec = [False, False], 0, None
        for i in range(steps):
            h = i % handles
            if busy[h]:
                nb = pair[h].encode_resident_end()
                pair[h].scene_report()
            pair[h].encode_resident_begin(src.data_ptr(), N, d_outs[h].data_ptr(), cap, xs, ys, PF)
            busy[h] = True
        for h in range(handles):
            if busy[h]:
                nb = pair[h].encode_resident_end()
                rec = pair[h].scene_report()
        return d_outs[(steps - 1) % handles][:nb].cpu().numpy().tobytes(), rec

    def psnr_y(T):
        h = pair[0]
        h.set_option("stats", 1)
        h.set_option("scene_cut", T)
        try:
            nb = h.encode_resident(scenes.data_ptr(), N, d_outs[0].data_ptr(), cap, xs, ys, PF)
            rec = h.picture_stats()
        finally:
            h.set_option("stats", 0)
        return nb, float(np.mean(M.psnr_from_sse(rec["sse"][:, 0], W * H))), float(np.min(M.psnr_from_sse(rec["sse"][:, 0], W * H)))

    try:
        off, none = run_steps(2, 0, clip)
        never, rec = run_steps(2, NEVER, clip)
        ok = off == never and len(none) == 0 and len(rec) == N and not (rec["flags"] & M.GOP_CUT).any() and int(rec["diff"][0]) == 0
        s_off, _ = run_steps(2, 0, scenes)
        s_cut, rec_cut = run_steps(2, T_CUT, scenes)
        cut_at = [int(r["frame"]) for r in rec_cut if r["flags"] & M.GOP_CUT]
        ok = ok and cut_at == [n for n in range(1, N) if n % SCENE_LEN == 0]
        q_off, q_cut = psnr_y(0), psnr_y(T_CUT)
        legs = (("off_pair", 0, clip, 2), ("never_pair", NEVER, clip, 2), ("off_single", 0, clip, 1), ("never_single", NEVER, clip, 1),
                ("scenes_off_pair", 0, scenes, 2), ("scenes_cut_pair", T_CUT, scenes, 2))
        times = {name: [] for name, _, _, _ in legs}
        for _ in range(max(3, args.rounds)):
            for name, T, src, nh in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, T, src, nh)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
    finally:
        for h in pair:
            h.close()
    best = {k: min(v) for k, v in times.items()}
    line = {"tool": "tools/e2e_scenecut.py",
            "workload": "%dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d, resident, one chunk" % (W, H, N, PF, VL, Q),
            "rounds": max(3, args.rounds), "steps": args.steps, "checks_ok": bool(ok)}
    for k in times:
        line[k + "_ms_per_sequence"] = round(best[k] * 1e3, 4)
        line[k + "_spread"] = round((max(times[k]) - best[k]) / best[k], 4)
    line["never_time_ratio_pair"] = round(best["never_pair"] / best["off_pair"], 4)
    line["never_time_ratio_single"] = round(best["never_single"] / best["off_single"], 4)
    line["off_GPixel_per_s_pair"] = round(px / best["off_pair"] * 1e-9, 1)
    line["scenes"] = {"scene_len": SCENE_LEN, "T": T_CUT, "cuts_at": cut_at, "bytes_off": len(s_off), "bytes_cut": len(s_cut),
                      "bytes_ratio": round(len(s_cut) / len(s_off), 4),
                      "psnr_y_mean_off": round(q_off[1], 3), "psnr_y_mean_cut": round(q_cut[1], 3),
                      "psnr_y_min_off": round(q_off[2], 3), "psnr_y_min_cut": round(q_cut[2], 3),
                      "time_ratio_pair": round(best["scenes_cut_pair"] / best["scenes_off_pair"], 4)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
