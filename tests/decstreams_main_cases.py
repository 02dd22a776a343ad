"""A batch of main-syntax streams per call (m2v_decode_streams_main_device): the batches it is tried on and what it must answer - shared
by tests/test_decstreams_main_cases.py (CPU, the host build tools/dec_streams_main_host.hpp) and tests/test_gpu_decode_streams_main.py.

The model composes, stream by stream, what the definition says of that stream ALONE under the call's flags -
decoder.decode(stream, quirks=False, syntax="main", b_pictures=bool(flags & 1), interlaced=bool(flags & 2)) - into the records, the
packed output and a written-mask.  The stage of a refusal is "probe" iff decoder._main_plan raises (the headers and the grammar of the
start codes); the sizes of a stream refused inside a slice are _main_plan's.  Nothing here looks at what the code under test computes.

The streams come from the existing writers (main_writer, bpic_writer, ilace_writer; the oracle's stream through decstreams_cases) and are small: decoder.py costs about
0.65 ms a macroblock."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import bpic_cases as B
import bpic_writer as BW
import dec_cases as D
import decstreams_cases as S
import ilace_cases as I
import ilace_writer as IW
import main_cases as C
import main_writer as MW

M = D.M
decoder = M.decoder
Refused = decoder.Refused
GUARD, FILL = D.GUARD, D.FILL
B_PICTURES, INTERLACED = 1, 2
ALL_FLAGS = (0, 1, 2, 3)
StreamStat, records_of, check, place = S.StreamStat, S.records_of, S.check, S.place
DECODE_BATCHES = (1, 2, 3, 5, 0)


# ---- the model ----
@functools.lru_cache(maxsize=None)
def alone(stream, flags):
    """what the definition says of one stream alone -> dict(stage, err_offset, the sizes, the counts, decoded)"""
    b, i = bool(flags & B_PICTURES), bool(flags & INTERLACED)
    try:
        hdr, pictures = decoder._main_plan(stream, b, i)[:2]
    except Refused as e:
        return dict(stage="probe", err_offset=e.offset)
    r = dict(stage=None, err_offset=0, pictures=len(pictures), width=hdr["width"], height=hdr["height"],
             frame_bytes=M.frame_bytes(hdr["width"], hdr["height"], "i420"))
    try:
        d = decoder.decode(stream, quirks=False, syntax="main", b_pictures=b, interlaced=i)
    except Refused as e:
        r.update(stage="slice", err_offset=e.offset)
        return r
    assert (len(d.pictures), d.width, d.height) == (r["pictures"], r["width"], r["height"])
    r.update(gops=len(d.gops), repeated_headers=d.repeated_headers, chains=sum(q["type"] == 1 for q in d.pictures), decoded=d)
    return r


def expected(batch, flags=3, layout="i420", cap=None, probe=False):
    """-> dict(records = [dict per stream: the fields of the record that are defined for it, out_offset, stage], out = the packed
    output (FILL where nothing may be written), written = bool per byte, total = the bytes of all rooms).  stage: None (OK),
    "probe", "slice" or "cap".  cap None: everything fits.  probe: what a call without a destination reports"""
    recs, at, parts = [], 0, []
    for s in batch:
        s = bytes(s)
        a = alone(s, flags)
        r = dict(es_bytes=len(s), out_offset=at, out_bytes=0, err_offset=0, status=D.OK, stage=None)
        if a["stage"] == "probe":
            r.update(status=D.SYNTAX, err_offset=a["err_offset"], stage="probe")
            recs.append(r)
            continue
        r.update({k: a[k] for k in S.SIZED})
        if a["stage"] is None:
            r.update({k: a[k] for k in S.COUNTS})
        room = r["pictures"] * r["frame_bytes"]
        if probe:
            r["out_bytes"] = room
        elif cap is not None and at + room > cap:
            r.update(status=D.OVERFLOW, stage="cap")
        elif a["stage"] == "slice":
            r.update(status=D.SYNTAX, err_offset=a["err_offset"], stage="slice")
        else:
            r["out_bytes"] = room
            parts.append((at, D.frames_of(a["decoded"], layout).reshape(-1)))
        at += room
        recs.append(r)
    out, mask = np.full(at, FILL, np.uint8), np.zeros(at, bool)
    for a, f in parts if not probe else []:
        out[a:a + f.size] = f
        mask[a:a + f.size] = True
    return dict(records=recs, out=out, written=mask, total=at)


def stages(batch, flags=3, **kw):
    return [w["stage"] for w in expected(batch, flags, **kw)["records"]]


# ---- the streams ----
def _ip(rng, mbw, mbh, **kw):
    return [C.intra_picture(rng, mbw, mbh, **kw), C.random_p(rng, mbw, mbh, **kw)]


@functools.lru_cache(maxsize=None)
def good(seed=1, w=32, h=32):
    """a main-syntax I / P stream of w x h"""
    rng = np.random.RandomState(9000 + seed)
    return MW.stream(w, h, _ip(rng, (w + 15) // 16, (h + 15) // 16))[0]


@functools.lru_cache(maxsize=None)
def ipbbpbb():
    """(stream, log): 32 x 32, I P B B P B B in coded order"""
    rng = np.random.RandomState(9100)
    return BW.stream(32, 32, B.order_pictures(rng, "IPBBPBB", 2, 2))


@functools.lru_cache(maxsize=None)
def field48():
    """(stream, log): 48 x 48, progressive_sequence 0 (four macroblock rows, not three), an I picture of field-DCT macroblocks and a P
    picture whose every macroblock is field-predicted and coded with field DCT"""
    rng = np.random.RandomState(9200)
    i = I.random_il(rng, 1, 3, 4)
    for sl in i["slices"]:
        for m in sl["mbs"]:
            m["dct"] = 1

    def mb(row, col):
        m = I.fmb(int(rng.randint(2)), I.legal_field(rng, col, row, 3, 4, 5), int(rng.randint(2)), I.legal_field(rng, col, row, 3, 4, 5))
        I.coded(rng, m, int(rng.randint(1, 64)))
        m["dct"] = 1
        return m
    return IW.stream(48, 48, [i, I.pred_picture(2, 3, 4, mb, q=4)])


@functools.lru_cache(maxsize=None)
def params_streams():
    """name -> (stream, log): 32 x 32 (48 x 32 for the f_code) I / P streams, each with one thing that differs from lane to lane of the walk"""
    out = {}
    rng = np.random.RandomState(9300)
    out["matrix_a"] = MW.stream(32, 32, _ip(rng, 2, 2), seq=dict(intra_matrix=C.MATRIX_A, non_intra_matrix=C.MATRIX_B))
    out["matrix_b"] = MW.stream(32, 32, _ip(rng, 2, 2), seq=dict(intra_matrix=C.MATRIX_B, non_intra_matrix=C.MATRIX_A))
    out["alternate_scan"] = MW.stream(32, 32, _ip(rng, 2, 2, alt=1))
    out["q_scale_type"] = MW.stream(32, 32, _ip(rng, 2, 2, qst=1))
    out["precisions"] = MW.stream(32, 32, [C.intra_picture(rng, 2, 2, prec=0), C.random_p(rng, 2, 2, prec=3)])
    out["f_code_3"] = MW.stream(48, 32, [C.intra_picture(rng, 3, 2), C.random_p(rng, 3, 2, f_code=(3, 3)), C.random_p(rng, 3, 2, f_code=(3, 3))])
    out["repeated_header"] = MW.stream(32, 32, _ip(rng, 2, 2) + [C.intra_picture(rng, 2, 2, seq=True, gop=True)], seq=dict(intra_matrix=C.MATRIX_A))
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    P = params_streams()
    return tuple([tiny(), good(4, 17, 33), ipbbpbb()[0], field48()[0], I.cases()["ipb_16"][0], S.oracle64(), P["matrix_a"][0], P["matrix_b"][0]] +
                 [P[k][0] for k in ("alternate_scan", "q_scale_type", "precisions", "f_code_3", "repeated_header")])


MIXED_B, MIXED_FIELD = (2, 4), (3, 4)          # the streams of mixed() with B pictures / with frame_pred_frame_dct 0


def _first(items, flags, stage):
    for name, s in items:
        if alone(bytes(s), flags)["stage"] == stage:
            return name, bytes(s)
    raise AssertionError("no stream of the list is refused at stage %s" % stage)


@functools.lru_cache(maxsize=None)
def verdicts():
    """[(what, stream)]: each case between good streams"""
    g = good(1)
    main_ref = sorted((n, v[0]) for n, v in C.refusals().items())
    cases = [("ok", good(2)),
             ("grammar", _first(main_ref, 3, "probe")[1]),
             ("leading_b", B.refusals()["b_first"][0]),
             ("slice_anchor", _first(main_ref, 3, "slice")[1]),
             ("slice_b", B.refusals()["backward_vector_outside"][0]),
             ("slice_field", I.refusals()["field_vector_left_0"][0]),
             ("empty", b""),
             ("three_bytes", b"\x00\x00\x01"),
             ("truncated", g[:len(g) * 2 // 3])]
    out = [("good", g)]
    for what, s in cases:
        out += [(what, bytes(s)), ("good", g)]
    return tuple(out)


VERDICT_STAGES = dict(ok=None, grammar="probe", leading_b="probe", slice_anchor="slice", slice_b="slice", slice_field="slice", empty="probe",
                      three_bytes="probe", good=None)          # (truncated: whatever the definition says of the cut)


@functools.lru_cache(maxsize=None)
def altered(seed):
    """64 seeded alterations of ilace_cases.altered_base() (32 x 32, I P B B of field pictures) - bit flips anywhere, cuts, insertions"""
    s = I.altered_base()[0]
    rng = np.random.RandomState(seed)
    out = []
    for k in range(64):
        at = int(rng.randint(4, len(s)))
        if k % 4 == 2:
            out.append(s[:at])
        elif k % 4 == 3:
            out.append(s[:at] + bytes([int(rng.randint(0, 256))]) + s[at:])
        else:
            out.append(D.flip(s, int(rng.randint(32, 8 * len(s)))))
    return tuple(out)


ALTERED_SEEDS = (31, 32)


@functools.lru_cache(maxsize=None)
def chunks():
    """I P B B P B B (32 x 32), three I pictures (32 x 32), I P P (48 x 32), I P (16 x 16): 15 pictures"""
    rng = np.random.RandomState(9400)
    ionly = MW.stream(32, 32, [C.intra_picture(rng, 2, 2, gop=(k == 0)) for k in range(3)])[0]
    ipp = MW.stream(48, 32, [C.intra_picture(rng, 3, 2), C.random_p(rng, 3, 2), C.random_p(rng, 3, 2)])[0]
    return (ipbbpbb()[0], ionly, ipp, good(3, 16, 16))


CHUNK_TYPES = ((1, 2, 3, 3, 2, 3, 3), (1, 1, 1), (1, 2, 2), (1, 2))


@functools.lru_cache(maxsize=None)
def late():
    """[good, the I P B B P B B stream with a bit of its LAST slice flipped so that the definition refuses exactly that slice, good]"""
    s, L = ipbbpbb()
    last = [a for k, a in L["units"] if k == "slice"][-1]
    end = [a for k, a in L["units"] if k == "end"][0]
    for bit in range(8 * (last + 5), 8 * end):
        x = D.flip(s, bit)
        a = alone(x, 3)
        if a["stage"] == "slice" and a["err_offset"] == last:
            return (good(1), x, good(2)), last
    raise AssertionError("no flip of the last slice is refused there")


@functools.lru_cache(maxsize=None)
def cap_batch():
    return (good(1), ipbbpbb()[0], good(2, 48, 32), good(3, 16, 16))


@functools.lru_cache(maxsize=None)
def tiny():
    """a main-syntax 1 x 1 I P P stream: frame_bytes 3, a room of 9 bytes (what stands behind it starts at an odd output address)"""
    rng = np.random.RandomState(9500)
    return MW.stream(1, 1, _ip(rng, 1, 1) + [C.random_p(rng, 1, 1)], tail=2)[0]


@functools.lru_cache(maxsize=None)
def alignment():
    """-> (streams, data, segments): sixteen streams - 1 x 1 (frame_bytes 3) and 16 x 16 (384) in turn, each ending in two zero bytes - at
    segment offsets = 0 .. 15 mod 16.  Every gap begins with 01 B3 (with the zeros in front of it a sequence_header_code that straddles
    the segment's end), holds a whole picture_start_code and ends with 00 00 01 (a start code with the next segment's first byte)"""
    rng = np.random.RandomState(9600)
    sixteen = MW.stream(16, 16, _ip(rng, 1, 1), tail=2)[0]
    streams = [tiny() if k & 1 == 0 else sixteen for k in range(16)]
    data, seg = bytearray(), []
    for k, s in enumerate(streams):
        gap = b"\x01\xb3\x00\x00\x01\x00\xff" + b"\x00\x00\x01"
        data += gap
        while len(data) % 16 != k:
            data[-3:-3] = b"\xff"
        seg.append((len(data), len(s)))
        data += s
    data += b"\x01\xb3\x00\x00\x01"
    return tuple(streams), bytes(data), tuple(seg)


SHORT_USER = ("user", b"\x00\x00\x01\xb2\x55")                 # the shortest user_data that says anything


@functools.lru_cache(maxsize=None)
def events():
    """(stream, log): 16 x 16, 300 pictures - an I picture every 50, still P pictures between - each with three short user_data units behind its
    coding extension: more start codes than the first guess of the event list holds"""
    rng = np.random.RandomState(9700)
    pics = []
    for k in range(300):
        p = C.intra_picture(rng, 1, 1, gop=(k % 50 == 0)) if k % 50 == 0 else dict(C.still_p(1, 1), gop=False)
        pics.append(dict(p, extras=[SHORT_USER] * 3))
    return MW.stream(16, 16, pics)


def event_guess(nbytes):
    """the first guess of a stream's event list (csrc/m2v_decode_streams_main.hip)"""
    return max(256, nbytes // 16 + 64)


@functools.lru_cache(maxsize=None)
def many():
    """4096 streams of 16 x 16: one I picture each, every 64th an I P B B stream"""
    rng = np.random.RandomState(9800)
    one = MW.stream(16, 16, [C.intra_picture(rng, 1, 1)])[0]
    four = BW.stream(16, 16, B.order_pictures(rng, "IPBB", 1, 1))[0]
    return tuple(four if k % 64 == 63 else one for k in range(4096))


def batches():
    """name -> (streams, flags): the batches that are run as they stand (the others have functions of their own above)"""
    v = tuple(s for _, s in verdicts())
    out = {"mixed": (mixed(), 3), "mixed_reversed": (mixed()[::-1], 3), "verdicts": (v, 3), "chunks": (chunks(), 3), "late": (late()[0], 3),
           "cap": (cap_batch(), 3), "events": ((good(1), events()[0], good(2)), 0), "many": (many(), 1)}
    for f in ALL_FLAGS:
        out["flags_%d" % f] = (mixed(), f)
    for seed in ALTERED_SEEDS:
        out["altered_%d" % seed] = (altered(seed), 3)
    return out


NAMES = ("mixed", "mixed_reversed", "verdicts", "chunks", "late", "cap", "events", "many", "flags_0", "flags_1", "flags_2", "flags_3", "altered_31", "altered_32")


# ---- the host build ----
_HARNESS = r"""
#include "dec_streams_main_host.hpp"
using namespace dec_streams_main_host;
extern "C" int dsm_host_decode(const uint8_t *es, const uint64_t *off, const uint64_t *nb, uint64_t n, int layout, unsigned flags, uint8_t *out, uint64_t cap,
                               uint64_t decode_batch, uint64_t level_bytes, StreamRecord *recs)
{
    std::vector<Segment> seg(n);
    for (uint64_t b = 0; b < n; ++b) seg[b] = Segment{es + off[b], nb[b]};
    const std::vector<StreamRecord> r = decode_streams(seg.data(), n, layout, flags, out, cap, decode_batch, level_bytes ? level_bytes : m2v::dec::kStreamsLevelBytes);
    for (uint64_t b = 0; b < n; ++b) { recs[b] = r[b]; recs[b].es_offset = off[b]; }
    return 0;
}
// plan_streams_main over stated streams: n streams of 16 x 16 (one macroblock), types one behind the other, counts[b] pictures each.
// Per chunk into out: first stream, its picture, pictures, steps, B pictures, carry0_from, carry1_from (in pictures of 384 bytes: 0 and 1
// the carried slots, 2 + k the chunk's k-th picture; -1 none); per picture into refs: fwd and bwd slot in the same unit.  -> chunks
extern "C" int dsm_host_plan(const uint8_t *types, const uint32_t *counts, uint64_t n, uint64_t decode_batch, int b_pictures, int64_t *out, int max, int64_t *refs)
{
    std::vector<m2v::dec::MainStreamInfo> info(n);
    const uint8_t *t = types;
    for (uint64_t b = 0; b < n; ++b) { info[b] = m2v::dec::MainStreamInfo{0, counts[b], 16, 16, 1, t}; t += counts[b]; }
    const m2v::dec::MainStreamsPlan P = m2v::dec::plan_streams_main(info.data(), n, ~0ull, false, decode_batch, b_pictures != 0);
    if (P.carry != 384) return -1;
    int k = 0;
    for (const m2v::dec::MainStreamsChunk &C : P.chunks) {
        if (C.buf_bytes != (2 + C.count) * 384) return -2;
        if (k < max) {
            int64_t *o = out + 7 * k;
            o[0] = P.pics[C.first].stream; o[1] = P.pics[C.first].pic; o[2] = (int64_t)C.count; o[3] = (int64_t)C.steps.size(); o[4] = (int64_t)C.b.count;
            o[5] = C.carry0_from < 0 ? -1 : C.carry0_from / 384; o[6] = C.carry1_from < 0 ? -1 : C.carry1_from / 384;
        }
        ++k;
    }
    for (size_t p = 0; p < P.pics.size(); ++p) {
        refs[3 * p] = (int64_t)(P.pics[p].fwd_off / 384); refs[3 * p + 1] = (int64_t)(P.pics[p].bwd_off / 384);
        refs[3 * p + 2] = (int64_t)((P.pics[p].out_off - P.out_offset[P.pics[p].stream]) / 384);
    }
    return k;
}
"""
_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dsm_host_")
        src, so = os.path.join(d, "dsm_host.cpp"), os.path.join(d, "libdsm_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.dsm_host_decode.argtypes = [ctypes.c_char_p, u64p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                      ctypes.c_uint64, ctypes.POINTER(StreamStat)]
        L.dsm_host_plan.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                    ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        _host = L
    return _host


def host_decode_streams(data, seg, flags=3, layout="i420", cap=None, probe=False, decode_batch=0, level_bytes=0):
    """-> ([dict per stream], the destination: GUARD + the rooms (cap, if that is more) + GUARD bytes, output byte 0 at index GUARD; None
    for a probe).  cap None: exactly the rooms, asked of a probe first"""
    L = host_lib()
    n = len(seg)
    off, nb = (ctypes.c_uint64 * n)(*[a for a, _ in seg]), (ctypes.c_uint64 * n)(*[b for _, b in seg])
    recs = (StreamStat * n)()
    L.dsm_host_decode(bytes(data), off, nb, n, M.LAYOUTS_420[layout], flags, None, 0, decode_batch, level_bytes, recs)
    if probe:
        return records_of(recs), None
    total = max(r["out_offset"] + r["out_bytes"] for r in records_of(recs))
    cap = total if cap is None else cap
    room = max(cap, total)
    buf = np.full(2 * GUARD + room, FILL, np.uint8)
    L.dsm_host_decode(bytes(data), off, nb, n, M.LAYOUTS_420[layout], flags, buf.ctypes.data + GUARD, cap, decode_batch, level_bytes, recs)
    return records_of(recs), buf


def host_plan(types, decode_batch, b_pictures=True):
    """types: per stream the picture types in coded order (16 x 16 streams) -> ([(first stream, its picture, pictures, anchor steps, B
    pictures, carry0_from, carry1_from)] per chunk, [(fwd slot, bwd slot, display index)] per picture)"""
    flat = bytes(t for s in types for t in s)
    counts = (ctypes.c_uint32 * len(types))(*[len(s) for s in types])
    out, refs = (ctypes.c_int64 * (7 * 256))(), (ctypes.c_int64 * (3 * len(flat)))()
    n = host_lib().dsm_host_plan(flat, counts, len(types), decode_batch, int(b_pictures), out, 256, refs)
    assert 0 <= n <= 256, n
    return [tuple(out[7 * k:7 * k + 7]) for k in range(n)], [tuple(refs[3 * p:3 * p + 3]) for p in range(len(flat))]


def pack_batches(items):
    """[(streams, flags, layout, cap or None, decode_batch)] -> the file tools/dec_streams_main_host_check reads (its header says the format)"""
    out = [struct.pack("<I", len(items))]
    for streams, flags, layout, cap, decode_batch in items:
        out.append(struct.pack("<IIQII", flags, M.LAYOUTS_420[layout], 0xFFFFFFFFFFFFFFFF if cap is None else cap, decode_batch, len(streams)))
        for s in streams:
            out += [struct.pack("<Q", len(s)), bytes(s)]
    return b"".join(out)
