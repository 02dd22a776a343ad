"""tools/e2e_decode_ext.py — what option "decode_extended" costs, in one process, one JSON line per mode.

  --unchanged   the paths the option does not touch, for an A/B of two libraries (M2V_LIB names the other one): the conformant stream of
                the bench clip (1920 x 1152, 90 frames) through m2v_decode_device with M2V_DEC_ISO in the module and in the main syntax,
                median of 7 decodes each.  Sets no option the parent lacks.
  --onoff       option on against off on streams both accept, one handle, alternating, three rounds of 7 decodes (medians), the frames
                asserted equal: the conformant stream above, and --stream FILE (b_pictures and interlaced on) where given.
  --slices      FILES...: streams of the same macroblocks cut into more and more slices a row (tests/ext_writer.py), the option on:
                the decode time of each, median of 7, and the frames asserted equal among them.
  --once        one decode with the option off and one with it on of the conformant stream and of --stream FILE: for a kernel trace.
ms per call; there is no threshold.

    python tools/e2e_decode_ext.py --unchanged | --onoff [--stream FILE] | --slices FILE... | --once [--stream FILE]   [--out FILE]
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
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--onoff", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--slices", nargs="*", default=None)
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

    res = {"tool": "e2e_decode_ext", "lib": os.environ.get("M2V_LIB") or "tree"}
    if args.unchanged:
        es = conformant_stream()
        out = torch.empty(n * M.frame_bytes(W, H, "i420"), dtype=torch.uint8, device="cuda:0")
        for name, syntax in (("module_syntax_iso_ms", "module"), ("main_syntax_iso_ms", "main")):
            ms = timed(lambda: enc.decode_device(es, "i420", "iso", out=out, syntax=syntax))
            res[name] = {"all": ms, "median": statistics.median(ms)}
    streams = []
    if args.onoff or args.once:
        streams.append(("c3_conformant_main_syntax", conformant_stream(), dict(syntax="main")))
        if args.stream:
            streams.append((os.path.basename(args.stream), load(args.stream), dict(syntax="main", b_pictures=True, interlaced=True)))
    for name, es, kw in streams:
        off, r = enc.decode_device(es, "i420", "iso", **kw)
        on, _ = enc.decode_device(es, "i420", "iso", extended=True, **kw)
        assert torch.equal(off, on), name
        if args.once:
            res[name] = {"pictures": int(r["pictures"]), "es_bytes": int(es.numel())}
            continue
        enc.set_option("decode_syntax", 1)                      # on the handle: the loop pays for no change of this option
        rounds = []
        for _ in range(3):
            a = timed(lambda: enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw))
            b = timed(lambda: enc.decode_device(es, "i420", "iso", out=on.reshape(-1), extended=True, **kw))
            rounds.append({"off": statistics.median(a), "on": statistics.median(b)})
        assert torch.equal(off, on), name
        o, x = statistics.median(v["off"] for v in rounds), statistics.median(v["on"] for v in rounds)
        res[name] = {"pictures": int(r["pictures"]), "es_bytes": int(es.numel()), "rounds_median_ms": rounds, "off_ms": o, "on_ms": x, "ratio": round(x / o, 4)}
    if args.slices:
        first = None
        res["slices"] = {}
        for path in args.slices:
            es = load(path)
            frames, r = enc.decode_device(es, "i420", "iso", syntax="main", b_pictures=True, extended=True)
            first = frames if first is None else first
            assert torch.equal(first, frames), path
            ms = timed(lambda: enc.decode_device(es, "i420", "iso", out=frames.reshape(-1), syntax="main", b_pictures=True, extended=True))
            res["slices"][os.path.basename(path)] = {"pictures": int(r["pictures"]), "es_bytes": int(es.numel()), "all": ms, "median": statistics.median(ms)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
