"""tools/e2e_deint.py — what deinterlacing on the device costs, per byte moved, beside a device-to-device copy.

The clips are 30 woven I420 frames of 720 x 576 and of 1920 x 1080 (random bytes: the clamp of "adaptive" is open almost everywhere and
no dword takes its short cut for still content; "adaptive" is also run on a still clip, where every dword takes it).  Every legal mode
and rate runs as one m2v_deinterlace_device call.  Bytes moved = what the mode must read plus what it writes, with B = frames x
frame_bytes: line / frame B/2 + B, line / field B + 2B, adaptive / frame 5B/2 + B (five fields' rows per output frame), adaptive / field
3B + 2B, blend B + B; the copy B + B.

    python tools/e2e_deint.py [--rounds 20] [--out FILE]       # ms per call by HIP events, best and median
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python tools/e2e_deint.py --once
                                    # two passes per clip: every call once, a copy kernel (torch: x + 0 on 32-bit words) and a
                                    # hipMemcpy device to device of the clip
    python tools/e2e_deint.py --trace DIR --out FILE    # adds the kernel times of that trace (the second pass) to FILE's JSON line
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLIPS = (("576i", 720, 576), ("1080i", 1920, 1080))
FRAMES = 30
CALLS = (("line", "frame"), ("line", "field"), ("adaptive", "frame"), ("adaptive", "field"), ("blend", "frame"), ("adaptive_still", "frame"), ("adaptive_still", "field"))
TARGET = 3.0


def frame_bytes(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def moved(mode, rate, B):
    """bytes the call must read plus bytes it writes"""
    mode = mode.split("_")[0]
    read = {("line", "frame"): B // 2, ("line", "field"): B, ("adaptive", "frame"): 5 * B // 2, ("adaptive", "field"): 3 * B, ("blend", "frame"): B}[(mode, rate)]
    return read + B * (2 if rate == "field" else 1)


def from_trace(d):
    """the k_deint dispatches of a --once run in time order, the kernel that follows each pass (the copy kernel) and the device-to-device
    copies -> microseconds per call, GB/s over the bytes moved, and the copy's rate over the call's; the second pass of each clip"""
    ker, mc = [], []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                ker.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, r["Kernel_Name"]))
    for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "DEVICE_TO_DEVICE" in (r.get("Direction") or "").upper():
                    mc.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    ker.sort()
    mc.sort()
    at = [i for i, k in enumerate(ker) if "k_deint" in k[2]]
    per, checks = len(CALLS), 5                  # per clip: five calls held against the definition, then two passes of every call
    each = checks + 2 * per
    out = {"dispatches": {"k_deint": len(at), "memcpy_d2d": len(mc)}}
    if len(at) != each * len(CLIPS):
        return out
    for k, (name, w, h) in enumerate(CLIPS):
        B = FRAMES * frame_bytes(w, h)
        res = {"bytes": B}
        second = at[each * k + checks + per:each * (k + 1)]
        copies = {}
        if second[-1] + 1 < len(ker) and "k_deint" not in ker[second[-1] + 1][2]:
            copies["copy_kernel"] = ker[second[-1] + 1][1]
            res["copy_kernel_name"] = ker[second[-1] + 1][2][:120]
        t0 = ker[second[-1]][0]
        t1 = ker[at[each * (k + 1)]][0] if k + 1 < len(CLIPS) else None
        mine = [us for t, us in mc if t > t0 and (t1 is None or t < t1)]
        if mine:
            copies["memcpy_d2d"] = mine[0]
        for c, us in copies.items():
            res[c] = {"us": round(us, 2), "GB_per_s": round(2 * B / us * 1e-3, 1)}
        best_copy = max((res[c]["GB_per_s"] for c in copies), default=None)
        for j, (mode, rate) in enumerate(CALLS):
            us = ker[second[j]][1]
            rate_gb = moved(mode, rate, B) / us * 1e-3
            res["%s/%s" % (mode, rate)] = {"us": round(us, 2), "bytes_moved": moved(mode, rate, B), "GB_per_s": round(rate_gb, 1),
                                          "copy_over_call_per_byte": round(best_copy / rate_gb, 2) if best_copy else None}
        out[name] = res
    out["aim"] = "within x%.1f of the copy per byte moved; reported, not gated" % TARGET
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="two passes per clip, nothing timed: for a kernel trace")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 run of --once: merge its kernel times into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace:
        line = json.loads(open(args.out).read()) if args.out and os.path.exists(args.out) else {"tool": "tools/e2e_deint.py"}
        line["kernel_trace"] = from_trace(args.trace)
        text = json.dumps(line)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()
    enc = M.Mpeg2Encoder(6, 6, 3, 2)
    res = {"tool": "tools/e2e_deint.py", "frames": FRAMES, "layout": "i420", "rounds": args.rounds, "events": {}}
    s = torch.cuda.Stream()
    for name, w, h in CLIPS:
        fb = frame_bytes(w, h)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(w)
        noise = torch.randint(0, 256, (FRAMES, fb), dtype=torch.uint8, device="cuda:0", generator=g)
        still = noise[:1].repeat(FRAMES, 1).contiguous()
        out = torch.empty(2 * FRAMES * fb, dtype=torch.uint8, device="cuda:0")
        dup = torch.empty_like(noise)
        # the call is the definition's, on the first three frames
        for mode, rate in CALLS[:5]:
            got = enc.deinterlace_device(noise[:3].contiguous(), w, h, "i420", mode, rate, "tff")
            assert np.array_equal(got.cpu().numpy(), M.deinterlace_frames(noise[:3].cpu().numpy(), w, h, "i420", mode, rate, "tff")), (name, mode, rate)
        torch.cuda.synchronize()

        def call(mode, rate):
            enc.deinterlace_device(still if mode.endswith("_still") else noise, w, h, "i420", mode.split("_")[0], rate, "tff", out=out, stream=s)

        def copies():
            with torch.cuda.stream(s):
                torch.add(noise.view(torch.int32), 0, out=dup.view(torch.int32))
                dup.copy_(noise)
        if args.once:
            for _ in range(2):
                for mode, rate in CALLS:
                    call(mode, rate)
                copies()
            torch.cuda.synchronize()
            continue
        ev = {}
        for mode, rate in CALLS:
            ms = []
            call(mode, rate)
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                call(mode, rate)
                b.record(s)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            B = FRAMES * fb
            ev["%s/%s" % (mode, rate)] = {"best_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "bytes_moved": moved(mode, rate, B),
                                          "GB_per_s_best": round(moved(mode, rate, B) / min(ms) * 1e-6, 1)}
        res["events"][name] = ev
    line = json.dumps(res if not args.once else {"tool": "tools/e2e_deint.py", "once": True})
    print(line)
    if args.out and not args.once:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    enc.close()


if __name__ == "__main__":
    main()
