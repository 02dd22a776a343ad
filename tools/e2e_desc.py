"""tools/e2e_desc.py — what a stream description (m2v_set_stream_desc) costs on the resident path, one JSON line.

The bench clip's recipe at 1920x1152, 10 GOPs of 1 I + 8 P frames, encoded on one pair of handles taking turns (as bench.py and
tools/e2e_recon.py time the resident entry) with nothing set, with a description that changes every field but repeats nothing, and
with repeat_headers on, alternating in rotating order, in one process; then k_assemble and the scans of one blocking sequence by the
library's own device events (option "profile"), without and with repeat_headers.  The streams must differ in the header bytes alone: the described stream is
checked against the plain one with the 34 bytes and the time codes rewritten on the host (the library's own m2v_time_code; the byte
comparison against the oracle is tests/test_gpu_stream_desc.py's).  Expected inside the noise: 34 bytes per GOP, written by one thread.

    python tools/e2e_desc.py [--rounds 9] [--steps 20] [--out FILE]
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
GOP_CODE, END_CODE = b"\x00\x00\x01\xb8", b"\x00\x00\x01\xb7"


def rewritten(M, plain, head, code, repeat):
    """the plain stream with its sequence headers replaced by `head`, every GOP's time code counted at `code` and, with repeat, `head`
    again in front of every GOP after the first"""
    at, k = [], plain.find(GOP_CODE)
    while k >= 0:
        at.append(k)
        k = plain.find(GOP_CODE, k + 4)
    end = plain.rfind(END_CODE)
    body = head
    for g, (a, b) in enumerate(zip(at, at[1:] + [end])):
        body += (head if repeat and g else b"") + GOP_CODE + M.time_code(g * (PF + 1), code) + plain[a + 8:b]
    body += END_CODE
    return body + bytes((len(body) // 32 + 1) * 32 - len(body))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.gops * (PF + 1)
    import torch
    import m2v_load
    M = m2v_load.load()
    xs, ys = W // 16, H // 16
    px = n * W * H
    clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0").contiguous()
    cap = n * W * H * 3 // 2
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
    torch.cuda.synchronize()
    fields = dict(fps=(30000, 1001), aspect="16:9", bit_rate=8_000_000, vbv_bits=1835008, video_format=0, colour="bt709")
    descs = {"off": None, "described": M.stream_desc(**fields), "repeat": M.stream_desc(repeat_headers=True, **fields)}

    def run_steps(steps, desc):
        """`steps` sequences on the two handles taking turns"""
        for h in pair:
            h.set_stream_desc(desc)
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
            pair[h].encode_resident_begin(clip.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF)
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
        return d_outs[(steps - 1) & 1][:nb].cpu().numpy().tobytes()

    try:
        got = {name: run_steps(4, d) for name, d in descs.items()}
        head = got["described"][:34]
        ok = (head != got["off"][:34] and got["described"] == rewritten(M, got["off"], head, 4, False)
              and got["repeat"] == rewritten(M, got["off"], head, 4, True) and got["repeat"].count(head) == args.gops)
        times = {name: [] for name in descs}
        order = list(descs.items())
        for _ in range(max(4, args.rounds)):
            for name, d in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, d)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps)
            order = order[1:] + order[:1]          # (whatever else the GPU is doing, no setting always meets the same part of it)
        # the two kernels the feature touches, by the library's own device events (option "profile"): one blocking sequence each
        kernels = {}
        pair[0].set_option("profile", 1)
        for name in ("off", "repeat", "off", "repeat"):
            pair[0].set_stream_desc(descs[name])
            pair[0].encode_resident(clip.data_ptr(), n, d_outs[0].data_ptr(), cap, xs, ys, PF)
            kernels[name] = {"k_assemble_us": round(pair[0].kernel_stats(3)[1] * 1e3, 2), "scans_us": round(pair[0].kernel_stats(4)[1] * 1e3, 2)}
    finally:
        for h in pair:
            h.close()
    best = {k: min(v) for k, v in times.items()}
    median = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    line = {"tool": "tools/e2e_desc.py",
            "workload": "%dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d; two handles taking turns" % (W, H, n, PF, VL, Q),
            "rounds": max(4, args.rounds), "steps": args.steps,
            "off_ms_per_sequence": round(best["off"] * 1e3, 4), "described_ms_per_sequence": round(best["described"] * 1e3, 4),
            "repeat_ms_per_sequence": round(best["repeat"] * 1e3, 4),
            "time_ratio_described": round(best["described"] / best["off"], 4), "time_ratio_repeat": round(best["repeat"] / best["off"], 4),
            "off_GPixel_per_s": round(px / best["off"] * 1e-9, 1), "repeat_GPixel_per_s": round(px / best["repeat"] * 1e-9, 1),
            "median_ms_per_sequence": {k: round(v * 1e3, 4) for k, v in median.items()},
            "kernels_by_device_events": kernels,
            "spread": {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()},
            "stream_bytes": {k: len(v) for k, v in got.items()},
            "streams_differ_in_the_header_bytes_alone": bool(ok)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
