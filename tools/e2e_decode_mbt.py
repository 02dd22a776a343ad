"""tools/e2e_decode_mbt.py — what option "decode_mb_tools" costs, in one process, one JSON line per mode (after tools/e2e_decode_ext.py,
whose --unchanged mode measures the paths neither option touches).

  --onoff       option on against off ("decode_extended" on in both) on streams both accept, one handle, alternating, three rounds of 7
                decodes (medians), the frames asserted equal: the conformant stream of the bench clip (1920 x 1152, 90 frames) in the
                main syntax, and --stream FILE (b_pictures and interlaced on) where given.
  --twins       B14 B15: the same macroblocks written with intra_vlc_format 0 and 1 (tests/mbt_writer.py), the option on for both:
                the decode time of each, three rounds of 7 alternating, and the frames asserted equal.
  --once        one decode of --twins' two files with the option on, and one of the first with it off: for a kernel trace.
ms per call; there is no threshold.

    python tools/e2e_decode_mbt.py --onoff [--stream FILE] | --twins B14 B15 | --once B14 B15   [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, PF, GOPS = 1920, 1152, 8, 10
XL = YL = 7
VL, Q = 3, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--onoff", action="store_true")
    ap.add_argument("--twins", nargs=2, default=None)
    ap.add_argument("--once", nargs=2, default=None)
    ap.add_argument("--stream", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    n = GOPS * (PF + 1)
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)

    def conformant_stream():
        d_clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0")
        d_es = torch.empty(n * W * H * 3 // 2, dtype=torch.uint8, device="cuda:0")
        enc.set_option("batch_frames", n)
        enc.set_option("conformant", 1)
        nb = enc.encode_resident(d_clip.data_ptr(), n, d_es.data_ptr(), d_es.numel(), W // 16, H // 16, PF)
        enc.set_option("conformant", 0)
        return d_es[:nb].clone()

    def load(path):
        return torch.from_numpy(np.fromfile(path, np.uint8)).to("cuda:0")

    def timed(fn, rounds=7):
        out = []
        fn()
        for _ in range(rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(round((time.perf_counter() - t) * 1e3, 3))
        return out

    res = {"tool": "e2e_decode_mbt"}
    both = dict(syntax="main", b_pictures=True, interlaced=True, extended=True)
    if args.onoff:
        streams = [("c3_conformant_main_syntax", conformant_stream(), dict(syntax="main", extended=True))]
        if args.stream:
            streams.append((os.path.basename(args.stream), load(args.stream), both))
        for name, es, kw in streams:
            off, r = enc.decode_device(es, "i420", "iso", **kw)
            on, _ = enc.decode_device(es, "i420", "iso", mb_tools=True, **kw)
            assert torch.equal(off, on), name
            enc.set_option("decode_syntax", 1)                  # on the handle: the loop pays for no change of these options
            enc.set_option("decode_extended", 1)
            rounds = []
            for _ in range(3):
                a = timed(lambda: enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw))
                b = timed(lambda: enc.decode_device(es, "i420", "iso", out=on.reshape(-1), mb_tools=True, **kw))
                rounds.append({"off": statistics.median(a), "on": statistics.median(b)})
            assert torch.equal(off, on), name
            o, x = statistics.median(v["off"] for v in rounds), statistics.median(v["on"] for v in rounds)
            res[name] = {"pictures": int(r["pictures"]), "es_bytes": int(es.numel()), "rounds_median_ms": rounds, "off_ms": o, "on_ms": x, "ratio": round(x / o, 4)}
    for paths in (args.twins, args.once):
        if not paths:
            continue
        es = [load(p) for p in paths]
        frames = [enc.decode_device(e, "i420", "iso", mb_tools=True, **both) for e in es]
        assert torch.equal(frames[0][0], frames[1][0]), "the twins decode to the same frames"
        off, _ = enc.decode_device(es[0], "i420", "iso", **both)
        assert torch.equal(off, frames[0][0])
        if paths is args.once:
            res["once"] = {os.path.basename(p): {"pictures": int(f[1]["pictures"]), "es_bytes": int(e.numel())} for p, e, f in zip(paths, es, frames)}
            continue
        enc.set_option("decode_syntax", 1)
        enc.set_option("decode_extended", 1)
        enc.set_option("decode_mb_tools", 1)
        rounds = []
        for _ in range(3):
            rounds.append([statistics.median(timed(lambda: enc.decode_device(e, "i420", "iso", out=f[0].reshape(-1), mb_tools=True, **both))) for e, f in zip(es, frames)])
        med = [statistics.median(r[k] for r in rounds) for k in (0, 1)]
        res["twins"] = {"files": [os.path.basename(p) for p in paths], "es_bytes": [int(e.numel()) for e in es], "pictures": int(frames[0][1]["pictures"]),
                        "rounds_median_ms": rounds, "b14_ms": med[0], "b15_ms": med[1], "ratio_b15_to_b14": round(med[1] / med[0], 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
