#!/usr/bin/env python3
"""Size / type statistics of an .m2v elementary stream in the style of the reference's README:735-768 (bytes per clip,
PSNR), optional PSNR against the source through the repo's decoder, optional PS / TS multiplexing.

    python tools/m2v_stats.py out.m2v [--yuv src.yuv [--i420 | --yv12 | --nv12 | --nv21]] [--ps out.mpg] [--ts out.ts]
    python tools/m2v_stats.py out.m2v --yuv src.yuv --device [--VL 3] [--Q 2] [--pframes N] [--conformant]
    python tools/m2v_stats.py out.m2v --yuv src.rgb [--rgb24 | --bgr24 | --rgbx | --bgrx | --xrgb | --xbgr | --rgbp] [--matrix bt601]
    python tools/m2v_stats.py out.m2v --levels
    python tools/m2v_stats.py out.m2v --gops

--levels: the level every GOP was coded at (m2v_set_gop_levels, option "gop_bytes_max"), read from the quantiser_scale_code of its slice
headers by the repo's decoder (Decoded.slice_qcodes; the Python decoder walks the whole stream: slow at full size).

--gops: start frame and length of every GOP (m2v_set_gop_starts, option "scene_cut"), read from the stream's start codes on the CPU
(the container scan: fast at any size).

--device: the PSNR comes from the encoder itself (option "stats", m2v_picture_stats) instead of the Python decoder, which takes minutes
per second of full-size video: the source is encoded again on the GPU with the given parameters, must give the file's stream byte for
byte, and the records' exact squared errors make the PSNR of all three planes.  That PSNR is the module's reconstruction against the
4:2:0 picture it codes (chroma: the module's two-stage mean of the 4:4:4 planes), over the source's size.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import m2v_load


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("m2v")
    ap.add_argument("--yuv", help="planar yuv444p source (SIM/tb_mpeg2encoder.v:210-218 layout) for PSNR")
    for l in ("i420", "yv12", "nv12", "nv21"):
        ap.add_argument("--" + l, dest="layout", action="store_const", const=l, help="--yuv holds 4:2:0 frames in this layout (W*H*3/2 bytes each)")
    for l in ("rgb24", "bgr24", "rgbx", "bgrx", "xrgb", "xbgr", "rgbp"):
        ap.add_argument("--" + l, dest="layout", action="store_const", const=l, help="--yuv holds RGB frames in this layout (W*H*3 or W*H*4 bytes each)")
    ap.add_argument("--matrix", default="bt601", choices=("bt601", "bt709", "bt601f", "bt709f"), help="the matrix the RGB frames were encoded with")
    ap.add_argument("--ps", help="write an MPEG-2 program stream")
    ap.add_argument("--ts", help="write an MPEG-2 transport stream")
    ap.add_argument("--pictures", action="store_true", help="one line per picture")
    ap.add_argument("--levels", action="store_true", help="one line per GOP: the level in its slice headers, its pictures, its bytes")
    ap.add_argument("--gops", action="store_true", help="one line per GOP: its start frame, its length, its bytes")
    ap.add_argument("--device", action="store_true", help="PSNR from the encoder's own statistics: --yuv is encoded again on the GPU and must give this stream")
    ap.add_argument("--VL", type=int, default=3, help="--device: VECTOR_LEVEL the stream was made with")
    ap.add_argument("--Q", type=int, default=2, help="--device: Q_LEVEL the stream was made with")
    ap.add_argument("--pframes", type=int, default=None, help="--device: i_pframes_count (default: what the stream's first GOP shows)")
    ap.add_argument("--conformant", action="store_true", help="--device: the stream was made with option conformant")
    args = ap.parse_args()
    M = m2v_load.load()
    C = M.container
    es = open(args.m2v, "rb").read()
    info, pics = C.scan(es)
    num, den = C.frame_rate(info.frame_rate_code)
    secs = info.pictures * den / num
    px = info.width * info.height * info.pictures
    print("%s: %dx%d, %d pictures (%d I, %d P, %d GOPs), %.3f s at %d/%d fps" % (
        args.m2v, info.width, info.height, info.pictures, info.i_pictures, info.p_pictures, info.gops, secs, num, den))
    print("  %d bytes (+%d padding) = %.4f bit/pixel, %.1f kbit/s; I pictures %.1f %% of the bytes" % (
        info.bytes, info.padding_bytes, info.bytes * 8 / px, info.bytes * 8 / secs / 1e3,
        100.0 * sum(p.bytes for p in pics if p.coding_type == 1) / max(info.bytes, 1)))
    # what the stream says about itself (m2v_set_stream_desc), and whether its sequence headers come again in front of later GOPs
    # (start codes cannot occur inside the coded data, so counting them is exact)
    seq = M.decoder.sequence_headers(es)[2]
    repeats = es[:info.bytes].count(b"\x00\x00\x01\xb3") - 1
    colour = (seq["colour_primaries"], seq["transfer_characteristics"], seq["matrix_coefficients"])
    print("  description: aspect code %d, bit rate %d bit/s, vbv %d bits, video_format %d, colour %s, display %dx%d" % (
        seq["aspect"], seq["bit_rate"] * 400, seq["vbv"] * 16384, seq["video_format"],
        {v: k for k, v in M.COLOURS.items()}.get(colour, "%s/%s/%s" % colour), seq["display_size"][0], seq["display_size"][1]))
    print("  sequence headers: %s" % ("repeated in front of %d of %d later GOPs" % (repeats, info.gops - 1) if repeats else "once, at byte 0"))
    sizes = np.array([p.bytes for p in pics], dtype=np.float64)
    for name, t in (("I", 1), ("P", 2)):
        s = sizes[[p.coding_type == t for p in pics]]
        if s.size:
            print("  %s pictures: mean %.0f  min %.0f  max %.0f bytes" % (name, s.mean(), s.min(), s.max()))
    if args.pictures:
        for k, p in enumerate(pics):
            print("  %5d  %s  tref %3d  %8d bytes  %d slices%s" % (k, "IP"[p.coding_type - 1], p.temporal_reference, p.bytes,
                                                                p.slices, "  GOP" if p.gop_start else ""))
    if args.levels:
        qc = M.decoder.decode(es, quirks=True).slice_qcodes
        starts = [k for k, p in enumerate(pics) if p.gop_start] + [len(pics)]
        for g, (a, b) in enumerate(zip(starts, starts[1:])):
            codes = sorted({c for row in qc[a:b] for c in row})
            names = ["%d" % (c.bit_length() - 1) if c & (c - 1) == 0 and 2 <= c <= 16 else "code %d" % c for c in codes]
            print("  GOP %4d  level %s  pictures %d..%d  %8d bytes" % (g, " + ".join(names), a, b - 1, sum(p.bytes for p in pics[a:b])))
    if args.gops:
        starts = [k for k, p in enumerate(pics) if p.gop_start] + [len(pics)]
        for g, (a, b) in enumerate(zip(starts, starts[1:])):
            print("  GOP %4d  start %6d  length %4d  %8d bytes" % (g, a, b - a, sum(p.bytes for p in pics[a:b])))
    if args.yuv and args.device:
        W, H = info.width, info.height
        xs, ys = M.fit_size(W, H)
        fb = M.frame_bytes(W, H, args.layout or "444")
        src = np.fromfile(args.yuv, np.uint8)
        n = min(src.size // fb, len(pics))
        starts = [k for k, p in enumerate(pics) if p.gop_start]
        pf = args.pframes if args.pframes is not None else (starts[1] - starts[0] if len(starts) > 1 else max(len(pics), 1)) - 1
        level = lambda s16: max(4, (s16 - 1).bit_length())           # the smallest XL / YL that holds the size
        enc = M.Mpeg2Encoder(level(xs), level(ys), args.VL, args.Q)
        try:
            enc.set_option("stats", 1)
            enc.set_option("conformant", int(args.conformant))
            if W % 16 or H % 16:
                enc.set_frame_size(W, H, "true")
            d = M.StreamDesc(seq["frame_rate_code"], seq["aspect"], seq["bit_rate"], seq["vbv"], seq["video_format"], *colour,
                             *seq["display_size"], 1 if repeats else 0, 0)
            if seq["display_size"] == (W, H):
                d.display_width = d.display_height = 0
            enc.set_stream_desc(d)
            got = enc.encode(src[:n * fb], xs, ys, pf, layout=args.layout, matrix=args.matrix)
            rec = enc.picture_stats()
        finally:
            enc.close()
        if got != es:
            sys.exit("  --device: encoding %s again with VL=%d Q=%d pframes=%d%s gives another stream (%d bytes): not this stream's source or parameters"
                     % (args.yuv, args.VL, args.Q, pf, " conformant" if args.conformant else "", len(got)))
        ny, nc = W * H, ((W + 1) // 2) * ((H + 1) // 2)
        db = np.stack([M.psnr_from_sse(rec["sse"][:, 0], ny), M.psnr_from_sse(rec["sse"][:, 1], nc), M.psnr_from_sse(rec["sse"][:, 2], nc)], axis=1)
        if args.pictures:
            for r, d in zip(rec, db):
                print("  %5d  %s  PSNR Y %6.2f U %6.2f V %6.2f  intra %5d inter %5d  mb bits %d" % (
                    r["frame"], "IP"[r["coding_type"] - 1], d[0], d[1], d[2], r["intra_mbs"], r["inter_mbs"], r["mb_bits"]))
        print("  luma PSNR over %d frames: mean %.2f dB  min %.2f dB   (from the encoder: U mean %.2f min %.2f, V mean %.2f min %.2f)" % (
            n, db[:, 0].mean(), db[:, 0].min(), db[:, 1].mean(), db[:, 1].min(), db[:, 2].mean(), db[:, 2].min()))
    elif args.yuv:
        m2v_decode = M.decoder
        dec = m2v_decode.decode(es, quirks=True)           # the encoder's own reconstruction (see fpga-mpeg2-encoder_amd/decoder.py)
        # (a true-size stream, M2V_HEADER_TRUE: the header's size is the source's own, the decoder hands out pictures of that size, and
        # the planes the encoder was given are those of the source padded to whole macroblocks - compared where the source is)
        W, H = info.width, info.height
        PW, PH = (16 * s16 for s16 in M.fit_size(W, H))
        src = np.fromfile(args.yuv, np.uint8)
        rgb = args.layout in M.LAYOUTS_RGB
        fb = M.frame_bytes(W, H, args.layout or "444")
        n = min(src.size // fb, len(dec.frames))
        src = M.pad_frames(src[:n * fb], W, H, args.layout or "444")
        if rgb:
            src = M.rgb_to444(src, PW, PH, args.layout, args.matrix)       # PSNR against the planes the encoder was given, by definition
        else:
            src = M.to444(src, PW, PH, args.layout) if args.layout else src.reshape(n, 3, PH, PW)
        src = src[:, :, :H, :W]
        ps = [m2v_decode.psnr(src[k, 0], dec.frames[k][0]) for k in range(n)]
        print("  luma PSNR over %d frames: mean %.2f dB  min %.2f dB" % (n, float(np.mean(ps)), float(np.min(ps))))
    if args.ps:
        d = C.mux_ps(es)
        open(args.ps, "wb").write(d)
        print("  program stream  : %s, %d bytes (+%.2f %%)" % (args.ps, len(d), 100.0 * (len(d) - info.bytes) / info.bytes))
    if args.ts:
        d = C.mux_ts(es)
        open(args.ts, "wb").write(d)
        print("  transport stream: %s, %d bytes (+%.2f %%)" % (args.ts, len(d), 100.0 * (len(d) - info.bytes) / info.bytes))


if __name__ == "__main__":
    main()
