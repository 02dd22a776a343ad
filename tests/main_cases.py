"""The main syntax of the device decoder (option "decode_syntax" = main): the streams it is tried on and what it must answer - shared by
tests/test_main_cases.py (CPU) and tests/test_gpu_decode_main.py.  The definition is the expectation: decoder.decode(stream,
quirks=False, syntax="main") - its frames, or the offset its Refused names.  Nothing here looks at what the device computes.

The streams are written by tests/main_writer.py at the smallest shapes that reach the syntax: 48 x 32 for types, precisions, scans,
matrices and quantisers, 160 x 96 for f_codes, 1088 x 16 for address increments with escapes.

host_lib(): the main_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_main_host.hpp compiled with g++."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import dec_cases as D
import dec_writer as W
import main_writer as MW

M = D.M
Refused = M.decoder.Refused


def spec(stream):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main"), None
    except Refused as e:
        return None, e.offset


_HARNESS = r"""
#include "dec_main_host.hpp"
extern "C" long long dec_main_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_main_host::decode(es, n, layout, cap, frames);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
extern "C" unsigned dec_main_host_increment(unsigned w11) { return m2v::dec::vlc_increment(w11); }
extern "C" int dec_main_host_vector(int pmv, int code, int residual, int r_size) { return m2v::dec::main_vector(pmv, code, residual, r_size); }
extern "C" int dec_main_host_scale(unsigned code, unsigned type) { return m2v::dec::main_scale(code, type); }
extern "C" int dec_main_host_scan(int alt, unsigned k) { return alt ? m2v::dec::alternate_to_raster(k) : m2v::dec::scan_to_raster(k); }
extern "C" int dec_main_host_zigzag_position(unsigned i) { return m2v::dec::zigzag_position(i); }
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_main_host_")
        src, so = os.path.join(d, "dec_main_host.cpp"), os.path.join(d, "libdec_main_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_main_host_decode.restype = ctypes.c_longlong
        L.dec_main_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(D.Stat)]
        L.dec_main_host_increment.restype = ctypes.c_uint
        _host = L
    return _host


def host_decode(stream, layout="i420", cap=None):
    """-> (frames [n, frame bytes] or None, the record as a dict)"""
    stream = bytes(stream)
    room = (1 << 24) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = D.Stat()
    host_lib().dec_main_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    if r["status"] != D.OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r      # (no picture at all: an empty array)


def record_of(d, stream):
    """the fields of m2v_decode_stat that the definition fixes"""
    return dict(pictures=len(d.pictures), gops=len(d.gops), width=d.width, height=d.height, repeated_headers=d.repeated_headers,
                chains=sum(p["type"] == 1 for p in d.pictures), es_bytes=len(stream), frame_bytes=M.frame_bytes(d.width, d.height, "i420"))


# ---- content ----
def block(rng, intra, dc=40):
    return W.random_block(rng, intra, dc=dc)


def blocks_for(rng, kind, cbp=63):
    return [block(rng, kind == "intra") for _ in range(6 if kind == "intra" else bin(cbp).count("1"))]


def mb(rng, kind, col=0, row=0, mbw=3, mbh=2, quant=None, incr=1, most=6, cbp=None):
    m = dict(kind=kind, incr=incr)
    if quant is not None:
        m["quant"] = quant
    if kind in ("coded", "not_coded"):
        m["mv"] = W.legal_vector(rng, col, row, mbw, mbh, most=most)
    if kind in ("coded", "nomc"):
        m["cbp"] = cbp if cbp is not None else int(rng.randint(1, 64))
    m["blocks"] = blocks_for(rng, kind, m.get("cbp", 63)) if kind != "not_coded" else []
    return m


def intra_picture(rng, mbw, mbh, q=4, **params):
    return dict(type=1, slices=[dict(q=q, mbs=[mb(rng, "intra") for _ in range(mbw)]) for _ in range(mbh)], **params)


def random_p(rng, mbw, mbh, q=4, most=6, **params):
    """a P picture of every kind of macroblock, skipped ones (never a row's first or last) and a macroblock quantiser now and then"""
    slices = []
    for row in range(mbh):
        mbs, col, pending = [], 0, 1
        while col < mbw:
            if 0 < col < mbw - 1 and rng.randint(5) == 0:
                col, pending = col + 1, pending + 1
                continue
            kind = ("coded", "nomc", "not_coded", "intra")[int(rng.randint(4))]
            quant = int(rng.randint(1, 32)) if kind != "not_coded" and rng.randint(4) == 0 else None
            mbs.append(mb(rng, kind, col, row, mbw, mbh, quant=quant, incr=pending, most=most))
            col, pending = col + 1, 1
        slices.append(dict(q=q, mbs=mbs))
    return dict(type=2, slices=slices, **params)


def still_p(mbw, mbh, kind="not_coded", **params):
    """a P picture that changes nothing: "MC not coded" with the zero vector, or every macroblock but the rows' ends skipped"""
    if kind == "skipped":
        row = [dict(kind="not_coded", mv=(0, 0))] + ([dict(kind="not_coded", mv=(0, 0), incr=mbw - 1)] if mbw > 1 else [])
    else:
        row = [dict(kind="not_coded", mv=(0, 0)) for _ in range(mbw)]
    return dict(type=2, slices=[dict(q=3, mbs=[dict(m) for m in row]) for _ in range(mbh)], **params)


MATRIX_A = [8 + (3 * i) % 57 for i in range(64)]                 # weights 8 .. 64, none of them the default's pattern
MATRIX_B = [16 + (5 * i) % 40 for i in range(64)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (stream, log): every valid main-syntax stream of the suite"""
    out = {}
    rng = np.random.RandomState(2024)
    # every type of tables B-2 and B-3, skipped macroblocks, 48 x 32
    i0 = dict(type=1, slices=[dict(q=3, mbs=[mb(rng, "intra"), mb(rng, "intra", quant=7), mb(rng, "intra")]),
                              dict(q=5, mbs=[mb(rng, "intra", quant=2), mb(rng, "intra"), mb(rng, "intra", quant=31)])])
    p1 = dict(type=2, slices=[dict(q=3, mbs=[mb(rng, "coded", 0, 0), mb(rng, "nomc"), mb(rng, "not_coded", 2, 0)]),
                              dict(q=4, mbs=[mb(rng, "intra"), mb(rng, "coded", 1, 1, quant=9), mb(rng, "nomc", quant=12)])])
    p2 = dict(type=2, slices=[dict(q=6, mbs=[mb(rng, "intra", quant=3), mb(rng, "coded", 2, 0, incr=2)]),
                              dict(q=2, mbs=[mb(rng, "not_coded", 0, 1), mb(rng, "nomc", incr=2)])])
    out["types"] = MW.stream(48, 32, [i0, p1, p2])
    # the four precisions, an I and a P picture each
    pics = []
    for prec in (0, 1, 2, 3):
        pics += [intra_picture(rng, 3, 2, prec=prec, gop=prec == 0), random_p(rng, 3, 2, prec=prec)]
    out["precisions"] = MW.stream(48, 32, pics)
    # both scale types at codes 1, 8, 9, 31: in the slice header and as macroblock quantisers
    pics = []
    for qst in (0, 1):
        for codes in ((1, 8), (9, 31)):
            pics.append(dict(type=1, qst=qst, gop=not pics, slices=[dict(q=c, mbs=[mb(rng, "intra"), mb(rng, "intra", quant=codes[1 - k]), mb(rng, "intra")])
                                                                   for k, c in enumerate(codes)]))
            pics.append(dict(type=2, qst=qst, slices=[dict(q=c, mbs=[mb(rng, "coded", 0, k), mb(rng, "nomc", quant=codes[1 - k]), mb(rng, "coded", 2, k, quant=c)])
                                                      for k, c in enumerate(codes)]))
    out["scales"] = MW.stream(48, 32, pics)
    # both scans, changing from picture to picture
    out["scans"] = MW.stream(48, 32, [intra_picture(rng, 3, 2, alt=1), random_p(rng, 3, 2, alt=1), random_p(rng, 3, 2, alt=0), intra_picture(rng, 3, 2, alt=0, gop=True),
                                      random_p(rng, 3, 2, alt=1)])
    # matrices: either alone and both
    for name, seq in (("matrix_intra", dict(intra_matrix=MATRIX_A)), ("matrix_non_intra", dict(non_intra_matrix=MATRIX_B)),
                      ("matrix_both", dict(intra_matrix=MATRIX_A, non_intra_matrix=MATRIX_B))):
        out[name] = MW.stream(48, 32, [intra_picture(rng, 3, 2), random_p(rng, 3, 2), intra_picture(rng, 3, 2, seq=True, gop=True), random_p(rng, 3, 2, qst=1)], seq=seq)
    # f_codes 1 .. 9 at 160 x 96: residuals of every size; wraps in both directions where the picture is wide enough for the range
    pics = [intra_picture(rng, 10, 6)]
    for f in range(1, 10):
        pics.append(fcode_picture(rng, f))
    out["fcodes"] = MW.stream(160, 96, pics)
    # f_codes 6 .. 9 in a picture wide enough for their ranges: wraps in both directions up to f_code 8
    out["fcodes_wide"] = MW.stream(1088, 16, [intra_picture(rng, 68, 1, q=8)] + [wide_fcode_picture(f) for f in (6, 7, 8, 9)])
    # address increments 1, 2, 33, 34 (one escape) and 67 (two escapes) in a row of 68 macroblocks
    zero = lambda incr=1: dict(kind="not_coded", mv=(0, 0), incr=incr)
    pics = [intra_picture(rng, 68, 1, q=6)]
    pics.append(dict(type=2, slices=[dict(q=3, mbs=[mb(rng, "coded", 0, 0, 68, 1), zero(67)])]))
    pics.append(dict(type=2, slices=[dict(q=3, mbs=[zero(), mb(rng, "nomc", incr=34), mb(rng, "coded", 67, 0, 68, 1, incr=33)])]))
    pics.append(dict(type=2, slices=[dict(q=3, mbs=[zero(), zero(2)] + [zero() for _ in range(64)] + [mb(rng, "intra")])]))
    out["escapes"] = MW.stream(1088, 16, pics)
    # each optional unit missing, one at a time and all together; zero bytes behind the last unit; an interlaced sequence
    body = lambda: [intra_picture(rng, 3, 2), random_p(rng, 3, 2)]
    out["no_display"] = MW.stream(48, 32, body(), seq=dict(display=False))
    out["no_gop"] = MW.stream(48, 32, [dict(p, gop=False) for p in body()])
    out["no_end"] = MW.stream(48, 32, body(), end=False)
    out["no_end_tail"] = MW.stream(48, 32, body(), end=False, tail=37)
    out["end_tail"] = MW.stream(48, 32, body(), tail=5)
    out["bare"] = MW.stream(48, 32, [dict(p, gop=False) for p in body()], seq=dict(display=False, progressive=0), end=False)
    out["odd_size"] = MW.stream(45, 19, body(), tail=3)
    # every transparent unit in every place it may stand
    U, C, PD = MW.USER, MW.COPYRIGHT, MW.PICTURE_DISPLAY
    pics = [intra_picture(rng, 3, 2, gop_extras=[U], extras=[U, C, PD, U]), random_p(rng, 3, 2, extras=[PD]), random_p(rng, 3, 2, extras=[C, U]),
            intra_picture(rng, 3, 2, seq=True, gop=True, gop_extras=[U, U], extras=[PD, C])]
    out["transparent"] = MW.stream(48, 32, pics, seq=dict(extras=[U], extras_behind=[U, U]))
    out["transparent_no_display"] = MW.stream(48, 32, body(), seq=dict(display=False, extras=[U, U]))
    # repeated sequence headers with matrices: in front of a GOP header and in front of a picture header
    pics = [intra_picture(rng, 3, 2), random_p(rng, 3, 2), intra_picture(rng, 3, 2, seq=True, gop=True), intra_picture(rng, 3, 2, seq=True, gop=False), random_p(rng, 3, 2)]
    out["repeats"] = MW.stream(48, 32, pics, seq=dict(intra_matrix=MATRIX_A, non_intra_matrix=MATRIX_B))
    # everything changes from picture to picture
    pics = [intra_picture(rng, 3, 2, prec=0, qst=1, alt=1, f_code=(15, 15)), random_p(rng, 3, 2, prec=3, qst=0, alt=0, f_code=(2, 1), most=6),
            random_p(rng, 3, 2, prec=1, qst=1, alt=1, f_code=(1, 3)), intra_picture(rng, 3, 2, prec=2, qst=0, alt=0, f_code=(4, 4), gop=True),
            random_p(rng, 3, 2, prec=0, qst=1, alt=0, f_code=(3, 2)), random_p(rng, 3, 2, prec=2, qst=0, alt=1, f_code=(1, 1)),
            random_p(rng, 3, 2, prec=1, qst=1, alt=0, f_code=(9, 9))]
    out["changing"] = MW.stream(48, 32, pics, seq=dict(non_intra_matrix=MATRIX_B))
    return out


def fcode_picture(rng, f):
    """160 x 96, P, f_code (f, f): not-coded macroblocks whose vectors need residuals of f - 1 bits; up to f_code 5 row 2 holds the two
    wraps - a large vector to the right followed by one to the left that the decoder reaches by leaving the range and coming back on
    the other side, and the other way round.  The range is +-8 << (f - 1) pel: from f_code 6 on (+-256 pel) no two vectors that stay
    inside a picture 160 wide are more than half the range apart, so no wrap can land inside it"""
    F = 1 << (f - 1)
    slices = []
    for row in range(6):
        mbs = []
        for col in range(10):
            # whole- and half-pel vectors pointing inward, as large as the picture and the range allow
            reach = min(16 * F - 1, 2 * 16 * (9 - col if col < 5 else col), 255)
            x = int(rng.randint(0, reach + 1)) * (1 if col < 5 else -1)
            reach = min(16 * F - 1, 2 * 16 * (5 - row if row < 3 else row))
            y = int(rng.randint(0, reach + 1)) * (1 if row < 3 else -1)
            mbs.append(dict(kind="not_coded", mv=(x, y)))
        slices.append(dict(q=2, mbs=mbs))
    if f <= 5:
        hi, lo = 16 * F - 1, -16 * F
        row = slices[2]["mbs"]
        # +80 pel at most from column 4, -80 from column 5, +48 from column 6: each delta the short way round leaves the range
        row[4], row[5], row[6] = (dict(kind="not_coded", mv=(v, 0)) for v in (min(hi, 160), max(lo, -160), min(hi, 96)))
    return dict(type=2, f_code=(f, f), slices=slices)


def wide_fcode_picture(f):
    """1088 x 16, P, f_code (f, 1): not-coded macroblocks with the zero vector but for two pairs.  Columns 30 and 31 carry +592 and -480
    pel (as far right and left as the picture lets them), columns 40 and 41 -640 and +416 pel, each cut to the f_code's range
    +-8 << (f - 1) pel: the two of a pair lie more than half the range apart up to f_code 8, so the delta the short way round leaves the
    range and the decoder wraps - to the left in the first pair, to the right in the second.  f_code 9 has a range of +-2048 pel: a
    wrap needs consecutive vectors more than 2048 pel apart, which no picture of at most 2048 holds; its picture carries the same
    vectors, with residuals of 8 bits and deltas beyond f_code 8's range, and no wrap"""
    F = 1 << (f - 1)
    hi, lo = 16 * F - 1, -16 * F
    even = lambda v: v - (v & 1)                                  # whole samples
    row = [dict(kind="not_coded", mv=(0, 0)) for _ in range(68)]
    for col, v in ((30, min(even(hi), 1184)), (31, max(lo, -960)), (40, max(lo, -1280)), (41, min(even(hi), 832))):
        row[col] = dict(kind="not_coded", mv=(v, 0))
    return dict(type=2, f_code=(f, 1), slices=[dict(q=2, mbs=row)])


# ---- known answers ----
def flat_intra(value, prec):
    """48 x 32, one I picture whose every block is DC only: the first block of a component codes value, the others 0 differentials"""
    diff = (value - 128) << prec                                # dct_dc = value * 8 / intra_dc_mult, relative to the reset value 128 * 8 / intra_dc_mult
    slices = []
    for row in range(2):
        mbs = []
        for col in range(3):
            first = col == 0
            mbs.append(dict(kind="intra", blocks=[dict(dc=diff if first and b in (0, 4, 5) else 0, coefs=[]) for b in range(6)]))
        slices.append(dict(q=4, mbs=mbs))
    return MW.stream(48, 32, [dict(type=1, prec=prec, slices=slices)])[0]


# ---- the refusals: one per line of the header's "still refused" list, and the forbidden values ----
@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (stream, kind of the unit the definition must name, its ordinal among the units of that kind)"""
    rng = np.random.RandomState(77)
    out = {}

    def base():
        r = np.random.RandomState(5)
        return [intra_picture(r, 3, 2), random_p(r, 3, 2)]

    def of(pics, unit, nth=0, **kw):
        s, L = MW.stream(48, 32, pics, strict=False, **kw)
        at = [a for k, a in L["units"] if k == unit][nth]
        return s, at

    p = base(); p[1]["type"] = 3
    out["b_picture"] = of(p, "picture", 1)
    p = base(); p[0]["type"] = 4
    out["d_picture"] = of(p, "picture", 0)
    for name, ext in (("field_picture", dict(picture_structure=1)), ("frame_pred_frame_dct_0", dict(frame_pred_frame_dct=0)),
                      ("concealment_vectors", dict(concealment=1)), ("intra_vlc_format_1", dict(intra_vlc_format=1))):
        p = base(); p[1]["ext"] = ext
        out[name] = of(p, "picture_ext", 1)
    quant_matrix = ("quant_matrix", b"\x00\x00\x01\xb5" + bytes([0x30, 0x00]))
    p = base(); p[0]["extras"] = [quant_matrix]
    out["quant_matrix_extension"] = of(p, "quant_matrix")
    out["scalable_extension"] = of(base(), "scalable", seq=dict(extras=[("scalable", b"\x00\x00\x01\xb5" + bytes([0x50, 0x00]))]))
    out["size_extension"] = of(base(), "sequence_ext", seq=dict(size_ext=4))
    out["chroma_422"] = of(base(), "sequence_ext", seq=dict(chroma_format=2))
    s, L = MW.stream(2064, 16, [dict(type=1, slices=[dict(q=4, mbs=[])])], strict=False)
    out["size_over_2048"] = (s, 0)
    p = base(); p[0]["slices"] = [dict(p[0]["slices"][0], code=1), dict(p[0]["slices"][0], code=1)]
    out["two_slices_in_a_row"] = of(p, "slice", 1)
    p = base(); p[1]["slices"][0]["mbs"] = [mb(rng, "nomc", incr=2), mb(rng, "nomc")]
    out["first_increment_2"] = of(p, "slice", 2)
    p = base(); p[0]["slices"][1]["mbs"] = [mb(rng, "intra"), mb(rng, "intra", incr=2)]
    out["skipped_in_i_picture"] = of(p, "slice", 1)
    p = base(); p[1]["slices"][1]["mbs"] = [mb(rng, "nomc"), mb(rng, "nomc")]
    out["skipped_last_of_row"] = of(p, "slice", 3)
    p = base(); p[1]["slices"][0]["mbs"] = [mb(rng, "nomc"), mb(rng, "nomc", incr=3)]
    out["increment_past_the_row"] = of(p, "slice", 2)
    p = base(); p[1]["slices"][0]["mbs"] = [mb(rng, "nomc"), mb(rng, "nomc", incr=35), mb(rng, "nomc")]
    out["escape_past_the_row"] = of(p, "slice", 2)
    p = base(); p[0]["slices"][0]["mbs"][1] = dict(mb(rng, "intra"), quant=0)
    out["macroblock_quant_0"] = of(p, "slice", 0)
    p = base(); p[1]["slices"][1]["mbs"] = [dict(kind="not_coded", mv=(-1, 0)), dict(kind="not_coded", mv=(0, 0)), dict(kind="not_coded", mv=(0, 0))]
    out["vector_outside"] = of(p, "slice", 3)
    p = base(); p[1].update(f_code=(3, 3)); p[1]["slices"][1]["mbs"] = [dict(kind="not_coded", mv=(0, 0)), dict(kind="not_coded", mv=(40, 0)), dict(kind="not_coded", mv=(0, 0))]
    out["vector_outside_f_code_3"] = of(p, "slice", 3)
    p = base(); p[1].update(f_code=(10, 1))
    out["f_code_10"] = of(p, "picture_ext", 1)
    p = base(); p[1].update(f_code=(15, 15))
    out["f_code_15_in_p"] = of(p, "picture_ext", 1)
    bad = list(MATRIX_A); bad[17] = 0
    out["matrix_weight_0"] = of(base(), "sequence", seq=dict(intra_matrix=bad))
    # a repeated header that says something else: written with another matrix behind the first pictures
    s1, L1 = MW.stream(48, 32, base() + [intra_picture(rng, 3, 2, seq=True, gop=True)], seq=dict(intra_matrix=MATRIX_A))
    at = [a for k, a in L1["units"] if k == "sequence"][1]
    s2 = bytearray(s1); s2[at + 12 + 20] ^= 0x02                                      # a weight in the middle of the repeated matrix
    out["repeated_header_differs"] = (bytes(s2), at)
    s, L = MW.stream(48, 32, base())
    at = [a for k, a in L["units"] if k == "slice"][1]
    out["user_data_behind_a_slice"] = (s[:at] + MW.USER[1] + s[at:], at)
    s, L = MW.stream(48, 32, base(), end=False)
    last = [a for k, a in L["units"] if k == "slice"][-1]
    out["last_slice_missing"] = (s[:last], [a for k, a in L["units"] if k == "slice"][-2])
    p = base(); p[1]["ext"] = dict(composite_display_flag=1)
    out["composite_display_flag"] = of(p, "picture_ext", 1)
    p = base(); p[1]["slices"][1]["intra_slice_flag"] = 1
    out["intra_slice_flag"] = of(p, "slice", 3)
    out["copyright_behind_gop"] = of([dict(base()[0], gop_extras=[MW.COPYRIGHT])] + base()[1:], "copyright")
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    """32 x 32, an I and a P picture with a matrix, user data, skipped macroblocks, f_code 2 and a macroblock quantiser: the stream the
    altered ones are made of"""
    rng = np.random.RandomState(99)
    pics = [intra_picture(rng, 2, 2, prec=1, extras=[MW.USER]), random_p(rng, 2, 2, f_code=(2, 2), qst=1, alt=1, most=4)]
    pics[1]["slices"][0]["mbs"][0]["quant"] = 5
    return MW.stream(32, 32, pics, seq=dict(non_intra_matrix=MATRIX_B))


@functools.lru_cache(maxsize=None)
def altered(flips=400, edits=100):
    """[(name, stream)]: every bit of every header flipped (the matrix's bytes: one bit each), seeded flips, cuts and insertions in slice data"""
    s, L = altered_base()
    first_slice = [a for k, a in L["units"] if k == "slice"][0]
    seq_end = [a for k, a in L["units"] if k == "sequence_ext"][0]
    out = []
    for bit in range(8 * first_slice):
        in_matrix = 12 <= (bit >> 3) < seq_end - 1
        if not in_matrix or bit % 8 == (bit >> 3) % 8:
            out.append(("bit%d" % bit, D.flip(s, bit)))
    # the headers of the second picture too
    p1 = [a for k, a in L["units"] if k == "picture"][1]
    s1 = [a for k, a in L["units"] if k == "slice"][2]
    out += [("bit%d" % bit, D.flip(s, bit)) for bit in range(8 * p1, 8 * s1)]
    rng = np.random.RandomState(1)
    lo, hi = 8 * (first_slice + 4), 8 * len(s)
    out += [("flip%d" % bit, D.flip(s, int(bit))) for bit in rng.randint(lo, hi, size=flips)]
    for k in range(edits):
        at = int(rng.randint(lo // 8, hi // 8))
        out.append(("cut%d" % at, s[:at]) if k % 2 else ("ins%d" % at, s[:at] + bytes([int(rng.randint(0, 256))]) + s[at:]))
    return out


_specs = {}


def spec_cached(stream):
    if stream not in _specs:
        _specs[stream] = spec(stream)
    return _specs[stream]
