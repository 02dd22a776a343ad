"""tools/e2e_decode.py — what decoding on the device costs a caller, in one process, one JSON line.

  * c3:     the stream of the bench clip (1920 x 1152, 90 frames, 8 P frames, Q_LEVEL 2), resident, decoded to I420 on one handle
            (m2v_decode_device, M2V_DEC_MODULE), best and median of several rounds; beside it in the same run the resident encode of
            that clip on one handle, and the decode again with "decode_batch" = 90 (the whole stream as one chunk).  The decoded
            frames are held against m2v_set_recon_out's of the encode, byte for byte.
  * batch:  64 clips x 9 frames of 320 x 240 (tools/e2e_batch.py's workload A) encoded as a batch, then decoded clip by clip.
  * python: for scale only, decoder.py on the first picture of the 1920 x 1152 stream (one I picture, cut out and closed with an end
            code).
ms per sequence and frames per second; there is no threshold.

    python tools/e2e_decode.py [--rounds 5] [--out FILE] [--no-python]
    python tools/e2e_decode.py --once    # one decode of the c3 stream, one k_recon_out pass over the same pictures (an encode with
                                         # m2v_set_recon_out) and a device-to-device copy of the stream's bytes: for a kernel trace
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gops", type=int, default=GOPS)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--no-python", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import m2v_load
    M = m2v_load.load()
    M.build()
    n = args.gops * (PF + 1)
    xs, ys = W // 16, H // 16
    fb = M.frame_bytes(W, H, "i420")
    d_clip = M.synth.clip_torch(W, H, n, clip_index=0, device="cuda:0")
    d_es = torch.empty(n * W * H * 3 // 2, dtype=torch.uint8, device="cuda:0")
    d_rec = torch.empty(n * fb, dtype=torch.uint8, device="cuda:0")
    d_dec = torch.empty(n * fb, dtype=torch.uint8, device="cuda:0")
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)
    enc.set_option("batch_frames", n)
    torch.cuda.synchronize()

    def encode(recon):
        enc.set_recon_out(d_rec.data_ptr() if recon else None, d_rec.numel() if recon else 0, "i420")
        return enc.encode_resident(d_clip.data_ptr(), n, d_es.data_ptr(), d_es.numel(), xs, ys, PF)

    nb = encode(True)
    es = d_es[:nb]
    enc.set_recon_out(None, 0)
    frames, rec = enc.decode_device(es, "i420", "module", out=d_dec)
    torch.cuda.synchronize()
    assert int(rec["pictures"]) == n and torch.equal(frames.reshape(-1), d_rec), "the decoded frames are not the encoder's reconstruction"
    if args.once:
        d_copy = torch.empty_like(es)
        d_copy.copy_(es)
        encode(True)
        enc.set_recon_out(None, 0)
        enc.decode_device(es, "i420", "module", out=d_dec)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "e2e_decode", "once": True, "pictures": n, "es_bytes": int(nb)}))
        return

    def timed(fn, rounds):
        out = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out

    dec_ms = timed(lambda: enc.decode_device(es, "i420", "module", out=d_dec), args.rounds)
    enc.set_option("decode_batch", n)                  # the whole stream as one chunk: every slice of the clip walked at once
    one_ms = timed(lambda: enc.decode_device(es, "i420", "module", out=d_dec), args.rounds + 1)[1:]
    enc.set_option("decode_batch", 0)
    assert torch.equal(d_dec, d_rec)
    enc_ms = timed(lambda: encode(False), args.rounds)
    res = {"tool": "e2e_decode", "c3": {"frames": n, "es_bytes": int(nb), "decode_ms": [round(v, 3) for v in dec_ms], "decode_best_ms": round(min(dec_ms), 3),
                                        "decode_median_ms": round(statistics.median(dec_ms), 3), "decode_fps_best": round(n / min(dec_ms) * 1e3, 1),
                                        "decode_one_chunk_ms": [round(v, 3) for v in one_ms], "decode_one_chunk_best_ms": round(min(one_ms), 3),
                                        "encode_ms": [round(v, 3) for v in enc_ms], "encode_best_ms": round(min(enc_ms), 3),
                                        "encode_fps_best": round(n / min(enc_ms) * 1e3, 1)}}
    # the batch: 64 clips of 9 frames, 320 x 240
    bw, bh, clips, per = 320, 240, 64, 9
    bclip = M.synth.clip_torch(bw, bh, clips * per, clip_index=3, device="cuda:0", scene_len=per).contiguous()
    benc = M.Mpeg2Encoder(XL, YL, VL, Q)
    benc.set_option("batch_frames", clips * per)
    benc.set_sequences([per] * clips)
    d_bes = torch.empty(clips * per * bw * bh * 3 // 2, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    benc.encode_resident(bclip.data_ptr(), clips * per, d_bes.data_ptr(), d_bes.numel(), bw // 16, bh // 16, PF)
    seq = benc.sequence_report()
    assert len(seq) == clips
    bfb = M.frame_bytes(bw, bh, "i420")
    d_bdec = torch.empty(clips * per * bfb, dtype=torch.uint8, device="cuda:0")

    def decode_batch():
        for k, s in enumerate(seq):
            benc.decode_device(d_bes[int(s["offset"]):int(s["offset"]) + int(s["bytes"])], "i420", "module", out=d_bdec[k * per * bfb:(k + 1) * per * bfb])

    decode_batch()
    b_ms = timed(decode_batch, args.rounds)
    res["batch"] = {"clips": clips, "frames_per_clip": per, "size": [bw, bh], "decode_ms": [round(v, 3) for v in b_ms], "decode_best_ms": round(min(b_ms), 3),
                    "ms_per_clip_best": round(min(b_ms) / clips, 4), "decode_fps_best": round(clips * per / min(b_ms) * 1e3, 1)}
    if not args.no_python:
        host = es.cpu().numpy().tobytes()
        second = host.find(b"\x00\x00\x01\x00", host.find(b"\x00\x00\x01\x00") + 4)
        one = host[:second] + b"\x00\x00\x01\xb7"
        one += bytes(-len(one) % 32)
        t = time.perf_counter()
        d = M.decoder.decode(one, quirks=True)
        res["python"] = {"pictures": len(d.frames), "size": [W, H], "seconds": round(time.perf_counter() - t, 2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
