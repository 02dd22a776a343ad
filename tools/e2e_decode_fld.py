"""tools/e2e_decode_fld.py — what option "decode_field_pictures" costs, in one process, one JSON line per run (after
tools/e2e_decode_mbt.py).

  --write DIR    (CPU) writes the measurement's streams with tests/fld_writer.py: DIR/fields.m2v, 720 x 576, 30 field pairs I P B B
                 of field-based macroblocks; DIR/frames.m2v, its frame-picture twin - the same macroblocks, a pair's two fields one
                 above the other in one frame picture; DIR/interlaced.m2v, 720 x 576, 30 interlaced frame pictures (field prediction,
                 field DCT).
  --off          the conformant stream of the bench clip (1920 x 1152, 90 frames) through m2v_decode_device in the main syntax with
                 the four older options on and this one off: three rounds of 7 decodes.  Run it with this tree's library and with
                 the parent's (M2V_LIB) in turn.
  --onoff FILE   option on against off on a stream both accept (DIR/interlaced.m2v), one handle, alternating, three rounds of 7, the
                 frames asserted equal.
  --twins FIELDS FRAMES   the field pairs with the option on against the twin with it off, three rounds of 7 alternating.
ms per call; there is no threshold.

    python tools/e2e_decode_fld.py --write DIR | --off | --onoff FILE | --twins FIELDS FRAMES   [--out FILE]
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


def write(out_dir):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import fld_cases as F
    import ilace_cases as IC
    import mbt_writer as TW
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.RandomState(91)
    mbw, rows = 45, 18
    pairs = []
    for n in range(30):
        pairs.append(F.pair(rng, ("II", "PP", "BB", "BB")[n % 4] if n else "II", 1, mbw, rows, same_parity=True))
    fields, _ = F.FW.stream(720, 576, [p for pr in pairs for p in pr])
    frames = [dict(type=a["type"], slices=[dict(sl, mbs=[F._as_frame_mb(m) for m in sl["mbs"]]) for sl in a["slices"] + c["slices"]]) for a, c in pairs]
    twin, _ = TW.stream(720, 576, frames, seq=dict(progressive=0))
    interlaced, _ = TW.stream(720, 576, IC.pictures(rng, ("IPBB" * 8)[:30], mbw, 2 * rows, most=5))
    for name, data in (("fields.m2v", fields), ("frames.m2v", twin), ("interlaced.m2v", interlaced)):
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(data)
    print(json.dumps({"tool": "e2e_decode_fld", "written": {"fields.m2v": len(fields), "frames.m2v": len(twin), "interlaced.m2v": len(interlaced)}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None)
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--onoff", default=None)
    ap.add_argument("--twins", nargs=2, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.write:
        return write(args.write)
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

    res = {"tool": "e2e_decode_fld", "library": os.environ.get("M2V_LIB", "this tree's")}
    older = dict(syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True)
    for name in ("decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools"):
        enc.set_option(name, 1)                                 # on the handle: the loops pay for no change of these options
    enc.set_option("decode_syntax", 1)
    if args.off:
        es = conformant_stream()
        frames, r = enc.decode_device(es, "i420", "iso", **older)
        rounds = [timed(lambda: enc.decode_device(es, "i420", "iso", out=frames.reshape(-1), **older)) for _ in range(3)]
        res["c3_older_options_on"] = {"pictures": int(r["pictures"]), "es_bytes": int(es.numel()), "rounds_ms": rounds,
                                      "median_ms": statistics.median(statistics.median(v) for v in rounds), "min_ms": min(min(v) for v in rounds),
                                      "max_ms": max(max(v) for v in rounds)}
    if args.onoff:
        es = load(args.onoff)
        off, r = enc.decode_device(es, "i420", "iso", **older)
        on, _ = enc.decode_device(es, "i420", "iso", field_pictures=True, **older)
        assert torch.equal(off, on)
        rounds = []
        for _ in range(3):
            a = timed(lambda: enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **older))
            b = timed(lambda: enc.decode_device(es, "i420", "iso", out=on.reshape(-1), field_pictures=True, **older))
            rounds.append({"off": statistics.median(a), "on": statistics.median(b)})
        assert torch.equal(off, on)
        o, x = statistics.median(v["off"] for v in rounds), statistics.median(v["on"] for v in rounds)
        res["onoff"] = {"file": os.path.basename(args.onoff), "pictures": int(r["pictures"]), "es_bytes": int(es.numel()), "rounds_median_ms": rounds, "off_ms": o, "on_ms": x,
                        "ratio": round(x / o, 4)}
    if args.twins:
        fields, frames = (load(p) for p in args.twins)
        f_on, rf = enc.decode_device(fields, "i420", "iso", field_pictures=True, **older)
        t_off, rt = enc.decode_device(frames, "i420", "iso", **older)
        assert rf["pictures"] == rt["pictures"] and f_on.shape == t_off.shape
        rounds = []
        for _ in range(3):
            a = timed(lambda: enc.decode_device(frames, "i420", "iso", out=t_off.reshape(-1), **older))
            b = timed(lambda: enc.decode_device(fields, "i420", "iso", out=f_on.reshape(-1), field_pictures=True, **older))
            rounds.append({"frame_twin_off": statistics.median(a), "field_pairs_on": statistics.median(b)})
        o, x = statistics.median(v["frame_twin_off"] for v in rounds), statistics.median(v["field_pairs_on"] for v in rounds)
        res["twins"] = {"files": [os.path.basename(p) for p in args.twins], "es_bytes": [int(fields.numel()), int(frames.numel())], "frames": int(rf["pictures"]),
                        "rounds_median_ms": rounds, "frame_twin_off_ms": o, "field_pairs_on_ms": x, "ratio": round(x / o, 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
