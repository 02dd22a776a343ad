"""tools/e2e_decode_conceal.py — what option "decode_conceal" costs, in one process, one JSON line per run (tools/e2e_decode_join.py's
frame; the streams are those of tools/e2e_decode_fld.py --write).

  --conceal FIELDS  DIR/fields.m2v (720 x 576, 30 field pairs I P B B) with "decode_field_pictures" on: option 1 against 0 on one
                    handle, alternating, three rounds of 7, the frames asserted equal and the report asserted zero; then the same
                    stream with the payload of one slice in ten overwritten (it cannot be read) under option 1: the report, the time.
  --c3              the conformant stream of the bench clip (tools/e2e_decode_fld.py's: 1920 x 1152, 90 frames, I and P) with the five
                    older options on: option 1 against 0, three rounds of 7.
  --trace FIELDS    four decodes with the option 0, four with 1 and four of the damaged stream, for a kernel trace around the process
                    (k_df_cont beside k_dc_rows, k_df_plan beside k_dc_plan).
ms per call; there is no threshold.

    python tools/e2e_decode_conceal.py --conceal FIELDS | --c3 | --trace FIELDS   [--out FILE]
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


def damaged(data, every=10):
    """the stream with the payload of every `every`-th slice overwritten with ones; -> (bytes, slices overwritten)"""
    import numpy as np
    d = np.array(data, np.uint8)
    at = np.nonzero((d[:-3] == 0) & (d[1:-2] == 0) & (d[2:-1] == 1))[0]
    codes = d[at + 3]
    ends = np.append(at[1:], len(d))
    n = 0
    for k in np.nonzero((codes >= 1) & (codes <= 0xAF))[0][every // 2::every]:
        d[at[k] + 4:ends[k]] = 0xFF
        n += 1
    return d, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conceal", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--c3", action="store_true")
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

    res = {"tool": "e2e_decode_conceal", "library": os.environ.get("M2V_LIB", "this tree's")}
    kw = dict(syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True)
    for name in ("decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures"):
        enc.set_option(name, 1)                                 # on the handle: the loops pay for no change of these options
    enc.set_option("decode_syntax", 1)
    if args.c3:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import e2e_decode_fld as E
        n = E.GOPS * (E.PF + 1)
        d_clip = M.synth.clip_torch(E.W, E.H, n, clip_index=0, device="cuda:0")
        es = torch.empty(n * E.W * E.H * 3 // 2, dtype=torch.uint8, device="cuda:0")
        enc.set_option("batch_frames", n)
        enc.set_option("conformant", 1)
        nb = enc.encode_resident(d_clip.data_ptr(), n, es.data_ptr(), es.numel(), E.W // 16, E.H // 16, E.PF)
        enc.set_option("conformant", 0)
        es = es[:nb].clone()
        off, r = enc.decode_device(es, "i420", "iso", **kw)
        on, _ = enc.decode_device(es, "i420", "iso", conceal=True, **kw)
        assert torch.equal(off, on) and int(enc.decode_conceal_report()["concealed_rows"]) == 0
        rounds = []
        for _ in range(3):
            a = timed(lambda: enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw))
            b = timed(lambda: enc.decode_device(es, "i420", "iso", out=on.reshape(-1), conceal=True, **kw))
            rounds.append({"conceal_0": statistics.median(a), "conceal_1": statistics.median(b)})
        o, x = (statistics.median(v[k] for v in rounds) for k in ("conceal_0", "conceal_1"))
        res["c3"] = {"frames": int(r["pictures"]), "es_bytes": int(es.numel()), "rounds_median_ms": rounds, "conceal_0_ms": o, "conceal_1_ms": x, "ratio_1_to_0": round(x / o, 4)}
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    path = args.conceal or args.trace
    data = np.fromfile(path, np.uint8)
    es = torch.from_numpy(data).to("cuda:0")
    bad, nbad = damaged(data)
    es_bad = torch.from_numpy(bad).to("cuda:0")
    off, r = enc.decode_device(es, "i420", "iso", **kw)
    on, _ = enc.decode_device(es, "i420", "iso", conceal=True, **kw)
    rep = enc.decode_conceal_report()
    assert torch.equal(off, on) and int(rep["bad_slices"]) == 0 and int(rep["concealed_rows"]) == 0 and int(rep["first_offset"]) == len(data)
    hurt, _ = enc.decode_device(es_bad, "i420", "iso", conceal=True, **kw)
    rep = enc.decode_conceal_report()
    assert int(rep["bad_slices"]) == nbad and hurt.shape == off.shape
    report = {k: int(rep[k]) for k in ("first_offset", "bad_slices", "concealed_rows", "grey_rows", "damaged_pictures")}
    if args.trace:
        for _ in range(4):
            enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw)
            enc.decode_device(es, "i420", "iso", out=on.reshape(-1), conceal=True, **kw)
            enc.decode_device(es_bad, "i420", "iso", out=hurt.reshape(-1), conceal=True, **kw)
        torch.cuda.synchronize()
        res["trace"] = {"decodes": 4}
    else:
        rounds = []
        for _ in range(3):
            a = timed(lambda: enc.decode_device(es, "i420", "iso", out=off.reshape(-1), **kw))
            b = timed(lambda: enc.decode_device(es, "i420", "iso", out=on.reshape(-1), conceal=True, **kw))
            c = timed(lambda: enc.decode_device(es_bad, "i420", "iso", out=hurt.reshape(-1), conceal=True, **kw))
            rounds.append({"conceal_0": statistics.median(a), "conceal_1": statistics.median(b), "conceal_1_damaged": statistics.median(c)})
        assert torch.equal(off, on)
        o, x, h = (statistics.median(v[k] for v in rounds) for k in ("conceal_0", "conceal_1", "conceal_1_damaged"))
        res["conceal"] = {"file": os.path.basename(path), "frames": int(r["pictures"]), "es_bytes": int(es.numel()), "rounds_median_ms": rounds, "conceal_0_ms": o,
                          "conceal_1_ms": x, "conceal_1_damaged_ms": h, "ratio_1_to_0": round(x / o, 4), "slices_overwritten": nbad, "report_damaged": report}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
