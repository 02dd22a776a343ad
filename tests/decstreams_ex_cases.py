"""A batch of main-syntax streams per call with the extended options (m2v_decode_streams_main_ex_device, flags M2V_DECS_EXTENDED = 4 and
M2V_DECS_MB_TOOLS = 8 beside the two of m2v_decode_streams_main_device): the batches it is tried on and what it must answer - shared by
tests/test_decstreams_ex_cases.py (CPU, the host build tools/dec_streams_ex_host.hpp) and tests/test_gpu_decode_streams_ex.py.

The model is decstreams_main_cases' with the two further flags: stream by stream what the definition says of that stream ALONE -
decoder.decode(stream, quirks=False, syntax="main", b_pictures=f & 1, interlaced=f & 2, extended=f & 4, mb_tools=f & 8) - composed into
the records, the packed output and a written-mask.  The stage of a refusal is "probe" iff decoder._main_plan(stream, b, i, x, t) raises.
Nothing here looks at what the code under test computes.

The streams come from ext_cases, mbt_cases, plan_cases and decstreams_main_cases and their writers and are small: decoder.py costs about
0.65 ms a macroblock."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import dec_cases as D
import decstreams_cases as S
import decstreams_main_cases as X0
import ext_cases as XC
import ext_writer as XW
import ilace_cases as IC
import main_cases as C
import mbt_cases as TC
import mbt_writer as TW
import plan_cases as PC

M = D.M
decoder = M.decoder
Refused = decoder.Refused
GUARD, FILL = D.GUARD, D.FILL
B_PICTURES, INTERLACED, EXTENDED, MB_TOOLS = 1, 2, 4, 8
LEGAL_FLAGS = (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15)         # MB_TOOLS needs EXTENDED
StreamStat, records_of, check, place = S.StreamStat, S.records_of, S.check, S.place
DECODE_BATCHES = (1, 2, 3, 5, 0)
Q, A, B_ = XW.quant_ext, C.MATRIX_A, C.MATRIX_B


# ---- the model ----
@functools.lru_cache(maxsize=None)
def alone(stream, flags):
    """what the definition says of one stream alone -> dict(stage, err_offset, the sizes, the counts, decoded)"""
    b, i, x, t = (bool(flags & k) for k in (B_PICTURES, INTERLACED, EXTENDED, MB_TOOLS))
    try:
        hdr, pictures = decoder._main_plan(stream, b, i, x, t)[:2]
    except Refused as e:
        return dict(stage="probe", err_offset=e.offset)
    r = dict(stage=None, err_offset=0, pictures=len(pictures), width=hdr["width"], height=hdr["height"],
             frame_bytes=M.frame_bytes(hdr["width"], hdr["height"], "i420"))
    try:
        d = decoder.decode(stream, quirks=False, syntax="main", b_pictures=b, interlaced=i, extended=x, mb_tools=t)
    except Refused as e:
        r.update(stage="slice", err_offset=e.offset)
        return r
    assert (len(d.pictures), d.width, d.height) == (r["pictures"], r["width"], r["height"])
    r.update(gops=len(d.gops), repeated_headers=d.repeated_headers, chains=sum(q["type"] == 1 for q in d.pictures), decoded=d)
    return r


def expected(batch, flags=15, layout="i420", cap=None, probe=False):
    """decstreams_main_cases.expected with this file's alone()"""
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


def stages(batch, flags=15, **kw):
    return [w["stage"] for w in expected(batch, flags, **kw)["records"]]


def slices_of(stream):
    """the slice start codes of every picture of a stream, from its start codes alone"""
    out = []
    for at, code in decoder.start_codes(stream):
        if code == 0x00:
            out.append(0)
        elif 1 <= code <= 0xAF and out:
            out[-1] += 1
    return out


# ---- the streams ----
def _plain():
    """plain main, B and interlaced streams of other sizes (decstreams_main_cases)"""
    return [X0.good(4, 17, 33), X0.ipbbpbb()[0], X0.field48()[0], X0.good(3, 16, 16), X0.tiny()]


@functools.lru_cache(maxsize=None)
def tiny():
    """1 x 1, I P, every slice with intra_slice_flag 1 and extras, a quant_matrix_extension at the P picture: frame_bytes 3"""
    rng = np.random.RandomState(9910)
    pics = XC.with_headers([C.intra_picture(rng, 1, 1), C.random_p(rng, 1, 1)])
    pics[1]["extras"] = [Q(intra=A, non_intra=B_)]
    return XW.stream(1, 1, pics, tail=2)[0]


@functools.lru_cache(maxsize=None)
def tools():
    """every valid stream of ext_cases and mbt_cases, plain main, B and interlaced streams of other sizes between them"""
    plain = _plain() + [tiny()]
    out = []
    for k, (name, v) in enumerate(sorted(XC.cases().items()) + sorted(TC.cases().items())):
        out.append(bytes(v[0]))
        if k % 3 == 0:
            out.append(bytes(plain[(k // 3) % len(plain)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed():
    """a batch whose streams need different flags: plain (none), B pictures (1), field macroblocks (2), slices cut and matrices (4, with 1
    and with 1 | 2), Table B-15 (8, with 1), concealment vectors (8), dual prime (8 | 2), all tools (8 | 2)"""
    x, t = XC.cases(), TC.cases()
    return tuple(bytes(s) for s in (X0.good(4, 17, 33), X0.ipbbpbb()[0], X0.field48()[0], x["ip_cut"][0], x["ipbb_cut"][0], x["fields_cut"][0], x["quant_both"][0],
                                    t["b15_mixed"][0], t["cmv_ip"][0], t["dual_flat"][0], t["all_tools"][0], tiny()))


@functools.lru_cache(maxsize=None)
def verdicts():
    """[(what, stream)]: the 30 hand-stated refusals of ext_cases and the 24 of mbt_cases, each between two good streams"""
    goods = (X0.good(1), bytes(XC.cases()["ip_cut"][0]), bytes(TC.cases()["cmv_ip"][0]))
    cases = [("ext_" + n, bytes(v[0])) for n, v in sorted(XC.refusals().items())] + [("mbt_" + n, bytes(v[0])) for n, v in sorted(TC.refusals().items())]
    out = [("good", goods[0])]
    for k, (what, s) in enumerate(cases):
        out += [(what, s), ("good", goods[(k + 1) % 3])]
    return tuple(out)


CONTINUITY = ("ext_gap", "ext_overlap", "ext_row_starts_at_column_1", "ext_row_ends_short", "ext_last_slice_ends_short")      # judged behind the walk


def _dual(v, dmv):
    return dict(kind="pred", motion="dual", fwd=(tuple(v), tuple(dmv)), bwd=None)


def _dual_p(rng, q=3):
    """a P picture of 3 x 2 macroblocks with frame_pred_frame_dct 0: dual prime at both ends of each row (vectors that keep all four
    reads inside their field), a frame-predicted macroblock with residual between them"""
    rows = []
    for row, (v, dmv) in enumerate((((0, 2), (0, 1)), ((0, -2), (0, -1)))):
        mid = IC.coded(rng, IC.frmb((1, 0)), int(rng.randint(1, 64)))
        rows.append(dict(q=q, mbs=[_dual(v, dmv), mid, _dual((0, v[1]), (0, 0))]))
    return dict(type=2, field=True, slices=rows)


CHUNK_LETTERS = "IPBBPBIPB"
CHUNK_CUTS = ((), (1,), (1, 2))                                  # one, two, three slices a row, in turn


@functools.lru_cache(maxsize=None)
def chunk_stream():
    """(stream, log): 48 x 32 of frame_pred_frame_dct 0 (two macroblock rows), I P B B P B | I P B with one, two and three slices a
    row in turn where a row has no skipped macroblock at the cut.  Picture 0 loads both matrices by quant_matrix_extension: they are
    in force up to picture 5 - with "decode_batch" 1 and 2 more than two chunks on - and picture 6's repeated sequence header puts the
    sequence's back.  The P pictures are dual prime at both ends of every row: with "decode_batch" 1 each is the first anchor of its
    chunk and reads both predictions from a carried slot, and every B picture has both anchors carried"""
    rng = np.random.RandomState(9920)
    pics = []
    for k, c in enumerate(CHUNK_LETTERS):
        p = _dual_p(rng) if c == "P" else IC.random_il(rng, " IPB".index(c), 3, 2, most=3)
        pics.append(p)
    pics = XC.cycle_cuts(pics, CHUNK_CUTS)
    pics[0]["extras"] = [Q(intra=A, non_intra=B_)]
    pics[6].update(seq=True, gop=True)
    for k, p in enumerate(pics):
        p.setdefault("gop", k == 0)
    return TW.stream(48, 32, pics, seq=dict(intra_matrix=B_))


@functools.lru_cache(maxsize=None)
def chunks():
    """the chunk stream beside an I P B B P B B stream (32 x 32), a cut I P stream (48 x 32) and a 16 x 16 one"""
    return (X0.ipbbpbb()[0], chunk_stream()[0], bytes(XC.cases()["ip_cut"][0]), X0.good(3, 16, 16))


def _flat_i(rows=2):
    """an I picture of rows x 3 macroblocks whose DC differentials are all 0 (a macroblock may start a slice as it is)"""
    return dict(type=1, slices=[dict(q=4, mbs=[dict(kind="intra", blocks=[dict(dc=0, coefs=[(1, 3, False)]) for _ in range(6)]) for _ in range(3)]) for _ in range(rows)])


@functools.lru_cache(maxsize=None)
def late():
    """((good, x, good), offset): x is 48 x 32, three I pictures - three chunks at "decode_batch" 1 - and the last picture's second row is
    cut into macroblock 0 and macroblock 2: the slice behind the gap is readable and is refused, at its own start code, for continuity"""
    p = _flat_i()
    r = p["slices"]
    p["slices"] = [dict(r[0], code=1), dict(r[1], code=2, mbs=[dict(r[1]["mbs"][0], incr=1)]), dict(r[1], code=2, mbs=[dict(r[1]["mbs"][2], incr=3)])]
    s, L = XW.stream(48, 32, [_flat_i(), dict(_flat_i(), gop=False), dict(p, gop=False)])
    return (X0.good(1), s, bytes(XC.cases()["ip_cut"][0])), [a for k, a in L["units"] if k == "slice"][-1]


@functools.lru_cache(maxsize=None)
def long_batch():
    """plan_cases' long_t and long_x (2 071 events, 9 to a range of the plan: ranges with several pictures, loads and a reset) between
    short streams"""
    return (X0.good(3, 16, 16), PC.cases()["long_t"][0], bytes(XC.cases()["ip_cut"][0]), PC.cases()["long_x"][0], tiny())


@functools.lru_cache(maxsize=None)
def alignment():
    """-> (streams, data, segments): sixteen streams - tiny() (frame_bytes 3) and a 48 x 16 I P stream whose row is cut in two in turn,
    each ending in two zero bytes - at segment offsets 0 .. 15 mod 16, the gaps as in decstreams_main_cases.alignment"""
    rng = np.random.RandomState(9930)
    cut = XW.stream(48, 16, XC.cycle_cuts([C.intra_picture(rng, 3, 1), C.random_p(rng, 3, 1)], ((1,), (2,))), tail=2)[0]
    streams = [tiny() if k & 1 == 0 else cut for k in range(16)]
    data, seg = bytearray(), []
    for k, s in enumerate(streams):
        data += b"\x01\xb3\x00\x00\x01\x00\xff" + b"\x00\x00\x01"
        while len(data) % 16 != k:
            data[-3:-3] = b"\xff"
        seg.append((len(data), len(s)))
        data += s
    data += b"\x01\xb3\x00\x00\x01"
    return tuple(streams), bytes(data), tuple(seg)


@functools.lru_cache(maxsize=None)
def cap_batch():
    x, t = XC.cases(), TC.cases()
    return (bytes(x["ip_cut"][0]), bytes(t["all_tools"][0]), bytes(x["fields_cut"][0]), X0.good(3, 16, 16))


@functools.lru_cache(maxsize=None)
def many():
    """1 024 streams of 16 x 16 with one, two and three slices (pictures of one macroblock: I; I P; I P P with Table B-15), in turn"""
    rng = np.random.RandomState(9940)
    pics = [C.intra_picture(rng, 1, 1), C.random_p(rng, 1, 1), C.random_p(rng, 1, 1)]
    three = [XW.stream(16, 16, pics[:1])[0], XW.stream(16, 16, XC.with_headers(pics[:2]))[0], TW.stream(16, 16, TC.with_flags(pics, ivf=1))[0]]
    return tuple(three[k % 3] for k in range(1024))


# 64 of the alterations of ext_cases.altered() / mbt_cases.altered(), drawn by a seeded permutation.  The seeds are chosen on decoder.py
# alone so that each batch holds at least 16 accepted streams, 16 refused at the slice stage and 8 at the probe stage
# (test_batches_hold_what_they_say asserts it on the model)
ALTERED = (("ext", 12), ("mbt", 1))


@functools.lru_cache(maxsize=None)
def altered(kind, seed):
    src = XC.altered() if kind == "ext" else TC.altered()
    return tuple(bytes(src[k][1]) for k in np.random.RandomState(seed).permutation(len(src))[:64])


def batches():
    """name -> (streams, flags): the batches that are run as they stand (alignment has a function of its own)"""
    out = {"tools": (tools(), 15), "verdicts": (tuple(s for _, s in verdicts()), 15), "verdicts_7": (tuple(s for _, s in verdicts()), 7),
           "chunks": (chunks(), 15), "late": (late()[0], 15), "long": (long_batch(), 15), "cap": (cap_batch(), 15), "many": (many(), 13)}
    for f in LEGAL_FLAGS:
        out["flags_%d" % f] = (mixed(), f)
    for kind, seed in ALTERED:
        out["altered_%s" % kind] = (altered(kind, seed), 15)
    return out


NAMES = ("tools", "verdicts", "verdicts_7", "chunks", "late", "long", "cap", "many") + tuple("flags_%d" % f for f in LEGAL_FLAGS) + ("altered_ext", "altered_mbt")


# ---- the host build ----
_HARNESS = r"""
#include "dec_streams_ex_host.hpp"
using namespace dec_streams_ex_host;
extern "C" int dsx_host_decode(const uint8_t *es, const uint64_t *off, const uint64_t *nb, uint64_t n, int layout, unsigned flags, uint8_t *out, uint64_t cap,
                               uint64_t decode_batch, uint64_t level_bytes, StreamRecord *recs)
{
    std::vector<Segment> seg(n);
    for (uint64_t b = 0; b < n; ++b) seg[b] = Segment{es + off[b], nb[b]};
    const std::vector<StreamRecord> r = decode_streams(seg.data(), n, layout, flags, out, cap, decode_batch, level_bytes ? level_bytes : m2v::dec::kStreamsLevelBytes);
    for (uint64_t b = 0; b < n; ++b) { recs[b] = r[b]; recs[b].es_offset = off[b]; }
    return 0;
}
// plan_streams_main_ex over stated streams: n streams of 16 x 16 (one macroblock), types and slice counts one behind the other, counts[b]
// pictures each.  Per chunk into out: first stream, its picture, pictures, slices, carry0_from, carry1_from (in pictures of 384 bytes: 0
// and 1 the carried slots, 2 + k the chunk's k-th picture; -1 none); per picture into refs: slice0, fwd and bwd slot in the same unit;
// per picture of a cut stream into pre: slice0; pre_slices: their slices and how many pictures.  -> chunks
extern "C" int dsx_host_plan(const uint8_t *types, const uint32_t *nslices, const uint32_t *counts, uint64_t n, uint64_t decode_batch, int b_pictures, int mb_tools,
                             int64_t *out, int max, int64_t *refs, int64_t *pre, int64_t *pre_slices)
{
    std::vector<m2v::dec::ExStreamInfo> info(n);
    const uint8_t *t = types;
    const uint32_t *s = nslices;
    for (uint64_t b = 0; b < n; ++b) { info[b] = m2v::dec::ExStreamInfo{m2v::dec::MainStreamInfo{0, counts[b], 16, 16, 1, t}, s}; t += counts[b]; s += counts[b]; }
    const m2v::dec::MainStreamsPlan P = m2v::dec::plan_streams_main_ex(info.data(), n, ~0ull, false, decode_batch, b_pictures != 0, mb_tools != 0);
    if (P.carry != 384) return -1;
    int k = 0;
    for (const m2v::dec::MainStreamsChunk &C : P.chunks) {
        if (C.buf_bytes != (2 + C.count) * 384) return -2;
        if (k < max) {
            int64_t *o = out + 6 * k;
            o[0] = P.pics[C.first].stream; o[1] = P.pics[C.first].pic; o[2] = (int64_t)C.count; o[3] = (int64_t)C.slices;
            o[4] = C.carry0_from < 0 ? -1 : C.carry0_from / 384; o[5] = C.carry1_from < 0 ? -1 : C.carry1_from / 384;
        }
        ++k;
    }
    for (size_t p = 0; p < P.pics.size(); ++p) {
        refs[3 * p] = (int64_t)P.pics[p].slice0; refs[3 * p + 1] = (int64_t)(P.pics[p].fwd_off / 384); refs[3 * p + 2] = (int64_t)(P.pics[p].bwd_off / 384);
    }
    for (size_t p = 0; p < P.pre.size(); ++p) pre[p] = (int64_t)P.pre[p].slice0;
    pre_slices[0] = (int64_t)P.pre_slices; pre_slices[1] = (int64_t)P.pre.size();
    return k;
}
"""
_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dsx_host_")
        src, so = os.path.join(d, "dsx_host.cpp"), os.path.join(d, "libdsx_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        u64p, u32p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64)
        L.dsx_host_decode.argtypes = [ctypes.c_char_p, u64p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                      ctypes.c_uint64, ctypes.POINTER(StreamStat)]
        L.dsx_host_plan.argtypes = [ctypes.c_char_p, u32p, u32p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, i64p, ctypes.c_int, i64p, i64p, i64p]
        _host = L
    return _host


def host_decode_streams(data, seg, flags=15, layout="i420", cap=None, probe=False, decode_batch=0, level_bytes=0):
    """-> ([dict per stream], the destination: GUARD + the rooms (cap, if that is more) + GUARD bytes, output byte 0 at index GUARD; None
    for a probe).  cap None: exactly the rooms, asked of a probe first"""
    L = host_lib()
    n = len(seg)
    off, nb = (ctypes.c_uint64 * n)(*[a for a, _ in seg]), (ctypes.c_uint64 * n)(*[b for _, b in seg])
    recs = (StreamStat * n)()
    L.dsx_host_decode(bytes(data), off, nb, n, M.LAYOUTS_420[layout], flags, None, 0, decode_batch, level_bytes, recs)
    if probe:
        return records_of(recs), None
    total = max(r["out_offset"] + r["out_bytes"] for r in records_of(recs))
    cap = total if cap is None else cap
    room = max(cap, total)
    buf = np.full(2 * GUARD + room, FILL, np.uint8)
    L.dsx_host_decode(bytes(data), off, nb, n, M.LAYOUTS_420[layout], flags, buf.ctypes.data + GUARD, cap, decode_batch, level_bytes, recs)
    return records_of(recs), buf


def host_plan(types, nslices, decode_batch, b_pictures=True, mb_tools=True):
    """types, nslices: per stream the picture types in coded order and the slices of each (16 x 16 streams) -> ([(first stream, its
    picture, pictures, slices, carry0_from, carry1_from)] per chunk, [(slice0, fwd slot, bwd slot)] per picture, [slice0] per picture of
    the verdict pass, pre_slices)"""
    flat = bytes(t for s in types for t in s)
    sl = [k for s in nslices for k in s]
    assert len(sl) == len(flat)
    counts = (ctypes.c_uint32 * len(types))(*[len(s) for s in types])
    out, refs, pre, total = (ctypes.c_int64 * (6 * 256))(), (ctypes.c_int64 * (3 * len(flat)))(), (ctypes.c_int64 * max(1, len(flat)))(), (ctypes.c_int64 * 2)()
    n = host_lib().dsx_host_plan(flat, (ctypes.c_uint32 * len(sl))(*sl), counts, len(types), decode_batch, int(b_pictures), int(mb_tools), out, 256, refs, pre, total)
    assert 0 <= n <= 256, n
    return [tuple(out[6 * k:6 * k + 6]) for k in range(n)], [tuple(refs[3 * p:3 * p + 3]) for p in range(len(flat))], list(pre[:total[1]]), total[0]


def pack_batches(items):
    """[(streams, flags, layout, cap or None, decode_batch)] -> the file tools/dec_streams_ex_host_check reads (its header says the format)"""
    out = [struct.pack("<I", len(items))]
    for streams, flags, layout, cap, decode_batch in items:
        out.append(struct.pack("<IIQII", flags, M.LAYOUTS_420[layout], 0xFFFFFFFFFFFFFFFF if cap is None else cap, decode_batch, len(streams)))
        for s in streams:
            out += [struct.pack("<Q", len(s)), bytes(s)]
    return b"".join(out)
