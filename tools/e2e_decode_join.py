"""tools/e2e_decode_join.py — what option "decode_join" costs, in one process, one JSON line per run (tools/e2e_decode_fld.py extended;
its --write and --off serve here too: the streams, and the c3 stream with the older options on for this tree's library and the
parent's).

  --join FIELDS  DIR/fields.m2v of e2e_decode_fld.py --write (720 x 576, 30 field pairs I P B B, sequence_end_code) with
                 "decode_field_pictures" on: option 3 against 0 on one handle, alternating, three rounds of 7, the frames asserted
                 equal; then the same stream with 1 MB of junk in front of it (start codes of slices, no sequence header) under
                 option 3: what the unjudged head costs - it is scanned, not planned.
  --trace FIELDS four decodes with the option 0 and four with 3, for a kernel trace around the process (k_df_plan beside k_dj_plan).
ms per call; there is no threshold.

    python tools/e2e_decode_join.py --join FIELDS | --trace FIELDS   [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
XL = YL = 7
VL, Q = 3, 2
JUNK_BYTES = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--join", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import m2v_load
    M = m2v_load.load()
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)

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

    res = {"tool": "e2e_decode_join", "library": os.environ.get("M2V_LIB", "this tree's")}
    kw = dict(syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True)
    for name in ("decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures"):
        enc.set_option(name, 1)                                 # on the handle: the loops pay for no change of these options
    enc.set_option("decode_syntax", 1)
    path = args.join or args.trace
    data = np.fromfile(path, np.uint8)
    es = torch.from_numpy(data).to("cuda:0")
    # 1 MB of junk: a slice start code every 64 bytes, the bytes between them not zero
    junk = np.full(JUNK_BYTES, 0x5A, np.uint8).reshape(-1, 64)
    junk[:, 0:3] = (0, 0, 1)
    junk[:, 3] = 1 + np.arange(len(junk)) % 0xAF
    es_junk = torch.from_numpy(np.concatenate([junk.reshape(-1), data])).to("cuda:0")
    off, r = enc.decode_device(es, "i420", "iso", **kw)
    on, _ = enc.decode_device(es, "i420", "iso", join=3, **kw)
    far, _ = enc.decode_device(es_junk, "i420", "iso", join=3, **kw)
    assert torch.equal(off, on) and torch.equal(off, far) and int(enc.decode_join_report()["join_offset"]) == JUNK_BYTES
    if args.trace:
        for _ in range(4):
            enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw)
            enc.decode_device(es, "i420", "iso", out=on.reshape(-1), join=3, **kw)
        torch.cuda.synchronize()
        res["trace"] = {"decodes": 4}
    else:
        rounds = []
        for _ in range(3):
            a = timed(lambda: enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw))
            b = timed(lambda: enc.decode_device(es, "i420", "iso", out=on.reshape(-1), join=3, **kw))
            c = timed(lambda: enc.decode_device(es_junk, "i420", "iso", out=far.reshape(-1), join=3, **kw))
            rounds.append({"join_0": statistics.median(a), "join_3": statistics.median(b), "join_3_behind_1MB": statistics.median(c)})
        assert torch.equal(off, on) and torch.equal(off, far)
        o, x, j = (statistics.median(v[k] for v in rounds) for k in ("join_0", "join_3", "join_3_behind_1MB"))
        res["join"] = {"file": os.path.basename(path), "frames": int(r["pictures"]), "es_bytes": int(es.numel()), "junk_bytes": JUNK_BYTES, "rounds_median_ms": rounds,
                       "join_0_ms": o, "join_3_ms": x, "join_3_behind_1MB_ms": j, "ratio_3_to_0": round(x / o, 4), "junk_ms": round(j - x, 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
