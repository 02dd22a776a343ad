"""tools/e2e_mux.py — what a container costs a resident caller, in one process, one JSON line.

Config c3's geometry (1920x1152, 90 frames, 8 P frames), two handles taking turns as bench.py times them, the forms alternating on the
same pair of handles, best of several rounds:
  * none:   m2v_encode_resident_begin / _end, the elementary stream stays in device memory;
  * ts, ps: the same with m2v_set_mux_out - the container muxed on the device behind the last chunk's assembly;
  * cpu_ts: the way without the device muxer - the elementary stream copied to pinned host memory, then m2vc_mux_ts on one host thread.
The device containers are held against m2vc_mux_ts / m2vc_mux_ps of the stream, byte for byte.

    python tools/e2e_mux.py [--rounds 5] [--steps 10] [--out FILE]
    python tools/e2e_mux.py --once     # one pass, nothing timed: k_es_scan, k_mux_plan, k_mux_write for TS and PS over the bench clip's stream
                                       # and a device-to-device copy of the same bytes beside them: for a kernel trace
"""
import argparse
import ctypes
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="sequences per timed pass")
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import importlib
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()
    C = importlib.import_module(M.__name__ + ".container")
    n = args.gops * (PF + 1)
    xs, ys = W // 16, H // 16
    px = n * W * H
    d_clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0")
    cap = px * 3 // 2
    room = M.mux_bound("ts", cap, n)
    d_outs = [torch.empty(cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    d_mux = [torch.empty(room, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    h_es = torch.empty(cap, dtype=torch.uint8).pin_memory()
    h_ts = np.empty(room, np.uint8)
    pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
    for h in pair:
        h.set_option("batch_frames", n)
        h.set_option("split_streams", 1)
    torch.cuda.synchronize()
    L = C.lib()

    def cpu_ts(h, nb):
        """the stream of handle h's buffer to pinned memory, then the CPU muxer -> container bytes"""
        h_es[:nb].copy_(d_outs[h][:nb], non_blocking=True)
        torch.cuda.synchronize()
        got = ctypes.c_size_t()
        r = L.m2vc_mux_ts(ctypes.cast(h_es.data_ptr(), ctypes.c_char_p), nb, h_ts.ctypes.data, h_ts.size, ctypes.byref(got))
        assert r == 0, r
        return got.value

    def run_steps(steps, form):
        for h in range(2):
            pair[h].set_mux_out(form if form in ("ts", "ps") else None, d_mux[h].data_ptr(), room)
        busy, nb = [False, False], 0
        for i in range(steps):
            h = i & 1
            if busy[h]:
                nb = pair[h].encode_resident_end()
                if form == "cpu_ts":
                    cpu_ts(h, nb)
            pair[h].encode_resident_begin(d_clip.data_ptr(), n, d_outs[h].data_ptr(), cap, xs, ys, PF, 0)
            busy[h] = True
        for h in range(2):
            if busy[h]:
                nb = pair[h].encode_resident_end()
                if form == "cpu_ts":
                    cpu_ts(h, nb)
        return nb

    try:
        if args.once:
            out = {"once": True, "frames": n}
            for form in ("ts", "ps"):
                nb = run_steps(1, form)
                rec = pair[0].mux_report()
                es = d_outs[0][:nb].cpu().numpy().tobytes()
                want = C.mux_ts(es) if form == "ts" else C.mux_ps(es)
                out[form + "_identical"] = int(rec["status"][0]) == 0 and d_mux[0][:int(rec["out_bytes"][0])].cpu().numpy().tobytes() == want
                out["stream_bytes"] = nb
            d_mux[1][:nb].copy_(d_outs[0][:nb])              # the yardstick: a device-to-device copy of the stream's bytes
            torch.cuda.synchronize()
            print(json.dumps(out))
            return 0 if out["ts_identical"] and out["ps_identical"] else 1

        forms = ("none", "ts", "ps", "cpu_ts")
        res_t = {f: [] for f in forms}
        same = {}
        for f in forms:
            run_steps(4, f)
        for _ in range(max(4, args.rounds)):
            for f in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nb = run_steps(args.steps, f)
                torch.cuda.synchronize()
                res_t[f].append((time.perf_counter() - t0) / args.steps)
                last = (args.steps - 1) & 1
                if f in ("ts", "ps"):
                    rec = pair[last].mux_report()
                    es = d_outs[last][:nb].cpu().numpy().tobytes()
                    want = C.mux_ts(es) if f == "ts" else C.mux_ps(es)
                    same[f] = int(rec["status"][0]) == 0 and d_mux[last][:int(rec["out_bytes"][0])].cpu().numpy().tobytes() == want
    finally:
        for h in pair:
            h.close()
    t = {f: min(v) for f, v in res_t.items()}
    line = {"tool": "tools/e2e_mux.py", "workload": "c3's geometry: %dx%d, %d frames, %d P frames per GOP, VL=%d Q=%d" % (W, H, n, PF, VL, Q),
            "rounds": max(4, args.rounds), "steps": args.steps, "stream_bytes": nb, "containers_identical_to_cpu_mux": same,
            "ms_per_sequence": {f: round(v * 1e3, 4) for f, v in t.items()},
            "spread": {f: round((max(v) - min(v)) / min(v), 4) for f, v in res_t.items()},
            "ratio_to_none": {f: round(t[f] / t["none"], 4) for f in forms},
            "added_ms": {f: round((t[f] - t["none"]) * 1e3, 4) for f in forms}}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
