"""Several slices a row, slice header extras, quant_matrix_extension and composite_display_flag 1 in the device decoder (option
"decode_extended" on top of the main syntax, "decode_b_pictures" and "decode_interlaced" either way): the streams it is tried on and what
it must answer - shared by tests/test_ext_cases.py (CPU) and tests/test_gpu_decode_ext.py.  The definition is the expectation:
decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=..., extended=True) - its frames, or the offset its
Refused names.  The known answers are frames the new code did not make: those of the definition WITH THE OPTION OFF on a twin stream
the existing decoder accepts (the same macroblocks with one slice a row, the same matrices in the sequence header, the same stream
without the slice extras, with composite_display_flag 0), and literal pictures.  Nothing here looks at what the device computes.

The streams are written by tests/ext_writer.py at the smallest shapes at which each rule can go wrong: 48 x 32 (3 x 2 macroblocks:
rows cut 3, 1 + 2, 2 + 1, 1 + 1 + 1), 80 x 16 (a skipped run inside a slice with a cut on either side), 48 x 48 with field pictures
(four rows), 560 x 16 (a first increment behind macroblock_escape), 64 x 128 with one macroblock per slice (288 slices).

host_lib(): the x_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_x_host.hpp compiled with g++."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import bpic_cases as BC
import dec_cases as D
import dec_writer as W
import ext_writer as XW
import ilace_cases as IC
import main_cases as C
import main_writer as MW

M = D.M
Refused = M.decoder.Refused


def spec(stream, b_pictures, interlaced, extended=True):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures, interlaced=interlaced, extended=extended), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, b_pictures, interlaced, extended=True):
    key = (stream, bool(b_pictures), bool(interlaced), bool(extended))
    if key not in _specs:
        _specs[key] = spec(stream, b_pictures, interlaced, extended)
    return _specs[key]


_HARNESS = r"""
#include "dec_x_host.hpp"
extern "C" long long dec_x_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, int b_pictures, int interlaced, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_x_host::decode(es, n, layout, cap, b_pictures != 0, interlaced != 0, frames);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
extern "C" unsigned dec_x_host_span(int ok, unsigned code, int first, int last) { return m2v::dec::x_span_pack(ok != 0, code, first, last); }
extern "C" int dec_x_host_continuous(unsigned cur, unsigned front, unsigned k, unsigned nslices, unsigned mbw) { return m2v::dec::x_continuous(cur, front, k, nslices, mbw); }
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_x_host_")
        src, so = os.path.join(d, "dec_x_host.cpp"), os.path.join(d, "libdec_x_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_x_host_decode.restype = ctypes.c_longlong
        L.dec_x_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(D.Stat)]
        L.dec_x_host_span.restype = ctypes.c_uint
        _host = L
    return _host


def host_decode(stream, b_pictures, interlaced, layout="i420", cap=None):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict)"""
    stream = bytes(stream)
    room = (1 << 24) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = D.Stat()
    host_lib().dec_x_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, int(bool(b_pictures)), int(bool(interlaced)), ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    if r["status"] != D.OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r


record_of = C.record_of


def pack_streams(items):
    """[(stream, b_pictures, interlaced)] -> the file tools/dec_x_host_check reads"""
    out = [struct.pack("<I", len(items))]
    for stream, b, i in items:
        out += [struct.pack("<IQ", int(bool(b)) | int(bool(i)) << 1, len(stream)), bytes(stream)]
    return b"".join(out)


# ---- content ----
PATTERNS = ((), (1,), (2,), (1, 2))                              # a row of three macroblocks cut 3, 1 + 2, 2 + 1, 1 + 1 + 1


def written(pic):
    """per row the columns at which a macroblock is written"""
    out = []
    for sl in pic["slices"]:
        col, cols = -1, []
        for m in sl["mbs"]:
            col += m.get("incr", 1)
            cols.append(col)
        out.append(cols)
    return out


def cycle_cuts(pics, patterns=PATTERNS):
    """every picture with cuts cycling over rows and pictures; a cut next to a skipped macroblock is left out (it has no place)"""
    out = []
    for k, pic in enumerate(pics):
        cols = written(pic)
        out.append(dict(pic, cuts=[[c for c in patterns[(k + row) % len(patterns)] if c in cols[row] and c - 1 in cols[row]] for row in range(len(cols))]))
    return out


def all_cuts(pics):
    """one macroblock per slice wherever a macroblock is written"""
    return [dict(pic, cuts=[[c for c in cols[1:] if c - 1 in cols] for cols in written(pic)]) for pic in pics]


def uncut(pics):
    return [{k: v for k, v in pic.items() if k != "cuts"} for pic in pics]


def ipbb(seed=31):
    """48 x 32, I P B B.  The P picture: row 0 uncut with a skipped macroblock inside its slice, row 1 three macroblocks with vectors that
    are not zero, so that a cut resets a vector's predictor"""
    rng = np.random.RandomState(seed)
    i0 = C.intra_picture(rng, 3, 2)
    i0["slices"][1]["mbs"][1]["quant"] = 9                       # a macroblock quantiser in front of a cut
    p1 = dict(type=2, slices=[dict(q=3, mbs=[C.mb(rng, "coded", 0, 0), C.mb(rng, "coded", 2, 0, incr=2)]),
                              dict(q=4, mbs=[dict(kind="not_coded", mv=(3, -2)), dict(kind="not_coded", mv=(-5, -3)), dict(C.mb(rng, "coded", 2, 1), mv=(-4, -1))])])
    b2 = BC.b_picture([[BC.pred((2, 1), (1, 1), rng, cbp=33), BC.pred((3, 1), None), BC.pred((-3, 2), (-2, 1), rng, cbp=12, quant=7)],
                       [BC.pred(None, (4, -2)), BC.pred((-1, -1), (-2, -2), incr=2)]])
    b3 = BC.random_b(rng, 3, 2)
    return [i0, p1, b2, b3]


def skip_run():
    """80 x 16 (5 x 1), I P: the P picture's slice in the middle is macroblock 1, a skipped one, macroblock 3 - a cut in front of the
    macroblock a skipped run follows and behind the one that ends it"""
    rng = np.random.RandomState(32)
    p = dict(type=2, cuts=[[1, 4]], slices=[dict(q=3, mbs=[C.mb(rng, "coded", 0, 0, 5, 1), C.mb(rng, "coded", 1, 0, 5, 1), C.mb(rng, "coded", 3, 0, 5, 1, incr=2),
                                                          C.mb(rng, "coded", 4, 0, 5, 1)])])
    return [dict(C.intra_picture(rng, 5, 1), cuts=[[2]]), p]


def fields():
    """48 x 48, progressive_sequence 0, I P B B of pictures with frame_pred_frame_dct 0 (four rows)"""
    rng = np.random.RandomState(33)
    pics = IC.pictures(rng, "IPBB", 3, 4, most=5)
    # row 1 of the P picture: three field-based macroblocks, cut 1 + 1 + 1 (its pattern), so field vectors stand on either side of a cut
    pics[1]["slices"][1]["mbs"] = [IC.fmb(0, (2, 1), 1, (1, 2)), IC.fmb(1, (-3, 1), 0, (2, -1)), IC.fmb(1, (-1, -2), 1, (-2, 2))]
    return pics


def many():
    """64 x 128 (4 x 8), nine pictures I P B B P B B P B, every macroblock written: with all_cuts 288 slices"""
    rng = np.random.RandomState(34)
    pics = []
    for c in "IPBBPBBPB":
        if c == "I":
            pics.append(C.intra_picture(rng, 4, 8))
        elif c == "P":
            pics.append(dict(type=2, slices=[dict(q=3, mbs=[C.mb(rng, ("coded", "not_coded", "nomc", "intra")[(col + row) % 4], col, row, 4, 8, most=5, cbp=1 << (col + row) % 6)
                                                            for col in range(4)]) for row in range(8)]))
        else:
            rows = []
            for row in range(8):
                mbs = []
                for col in range(4):
                    d = ((1, 0), (0, 1), (1, 1))[(col + row) % 3]
                    mv = [W.legal_vector(rng, col, row, 4, 8, most=5) if d[k] else None for k in (0, 1)]
                    mbs.append(BC.pred(mv[0], mv[1], rng, cbp=(1 << (col % 6)) if (col + row) % 2 else None))
                rows.append(mbs)
            pics.append(BC.b_picture(rows))
    return pics


def with_headers(pics):
    """every slice with intra_slice_flag 1: 0, 1 and 3 information bytes, intra_slice either way, cycling"""
    out = []
    n = 0
    for pic in pics:
        slices = []
        for sl in pic["slices"]:
            slices.append(dict(sl, header=dict(intra_slice=n & 1, reserved=(37 * n) & 127, info=[(91 * n + k) & 255 for k in range((0, 1, 3)[n % 3])])))
            n += 1
        out.append(dict(pic, slices=slices))
    return out


A, B_ = C.MATRIX_A, C.MATRIX_B
Q = XW.quant_ext


def _ip(seed):
    rng = np.random.RandomState(seed)
    return [C.intra_picture(rng, 3, 2), C.random_p(rng, 3, 2)]


def all_intra(rng, ptype, mbw=3, mbh=2):
    """a picture of type ptype whose every macroblock is intra: it reads no reference, so an I picture of the same blocks is its twin"""
    return dict(type=ptype, slices=[dict(q=5, mbs=[C.mb(rng, "intra") for _ in range(mbw)]) for _ in range(mbh)])


# ---- the valid cases: name -> (stream, log, b_pictures, interlaced) ----
@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    out["ipbb_cut"] = XW.stream(48, 32, cycle_cuts(ipbb())) + (True, False)
    out["ipbb_cut_shifted"] = XW.stream(48, 32, cycle_cuts(ipbb(), PATTERNS[1:] + PATTERNS[:1])) + (True, True)
    out["ip_cut"] = XW.stream(48, 32, cycle_cuts(ipbb()[:2], PATTERNS[3:] + PATTERNS[:3])) + (False, False)
    out["skip_run"] = XW.stream(80, 16, skip_run()) + (False, False)
    out["fields_cut"] = XW.stream(48, 48, cycle_cuts(fields(), PATTERNS[1:] + PATTERNS[:1])) + (True, True)
    out["fields_ip_cut"] = XW.stream(48, 48, cycle_cuts(fields()[:2], PATTERNS[1:] + PATTERNS[:1])) + (False, True)
    rng = np.random.RandomState(35)
    out["escape"] = XW.stream(560, 16, [dict(C.intra_picture(rng, 35, 1), cuts=[[33, 34]])]) + (False, False)
    out["many"] = XW.stream(64, 128, all_cuts(many())) + (True, False)
    out["headers"] = XW.stream(48, 32, with_headers(cycle_cuts(ipbb()))) + (True, False)
    out["headers_fields"] = XW.stream(48, 48, with_headers(fields())) + (True, True)
    for name, kw in (("intra", dict(intra=A)), ("non_intra", dict(non_intra=B_)), ("both", dict(intra=A, non_intra=B_)), ("neither", {})):
        p = _ip(36)
        p[0]["extras"] = [Q(**kw)]
        out["quant_" + name] = XW.stream(48, 32, p) + (False, False)
    for k, extras in enumerate(([MW.USER, Q(intra=A)], [Q(intra=A), MW.PICTURE_DISPLAY], [MW.PICTURE_DISPLAY, Q(intra=A), MW.USER, MW.COPYRIGHT])):
        p = _ip(36)
        p[0]["extras"] = extras
        out["quant_beside_%d" % k] = XW.stream(48, 32, p) + (False, False)
    out["quant_per_picture"] = XW.stream(48, 32, quant_per_picture()[0]) + (False, False)
    out["quant_coded_order"] = XW.stream(48, 32, quant_coded_order()[0]) + (True, False)
    out["quant_bbb"] = XW.stream(48, 32, quant_bbb()) + (True, False)
    p = _ip(37)
    p[0]["ext"] = dict(composite_display_flag=1)
    p[1]["ext"] = dict(composite_display_flag=1)
    out["composite"] = XW.stream(48, 32, cycle_cuts(p)) + (False, True)
    return out


def quant_per_picture():
    """I pictures only: none; loads intra A; carried; loads intra B_ (each matrix on its own: non-intra has no say here); a repeated
    sequence header puts the sequence's back; -> (pictures, the intra matrix in force per picture)"""
    rng = np.random.RandomState(38)
    pics = [C.intra_picture(rng, 3, 2) for _ in range(6)]
    pics[1]["extras"] = [Q(intra=A)]
    pics[3]["extras"] = [Q(intra=B_, non_intra=A)]
    pics[4]["extras"] = [Q(non_intra=B_)]
    pics[5].update(seq=True, gop=True)
    return pics, [None, A, A, B_, B_, None]


def quant_coded_order():
    """I B B P in display order, coded I P B B, every macroblock intra: the P picture loads A, and the B pictures behind it in coded
    order - in front of it on the screen - are dequantised with A; -> (pictures, the intra matrix per coded picture)"""
    rng = np.random.RandomState(39)
    pics = [all_intra(rng, t) for t in (1, 2, 3, 3)]
    pics[1]["extras"] = [Q(intra=A)]
    return pics, [None, A, A, A]


def quant_bbb():
    """I P B B B B with matrices that change at every B picture: for "decode_batch" 1, 2, 3 and 5 a chunk's edge falls between them"""
    rng = np.random.RandomState(40)
    pics = [C.intra_picture(rng, 3, 2), C.random_p(rng, 3, 2)] + [BC.random_b(rng, 3, 2) for _ in range(4)]
    pics[2]["extras"] = [Q(non_intra=B_)]
    pics[3]["extras"] = [Q(intra=A)]
    pics[4]["extras"] = [Q(non_intra=A, intra=B_)]
    pics[5]["extras"] = [Q()]
    return cycle_cuts(pics)


def flags(name):
    return cases()[name][2:]


# ---- known answers: name -> (stream, b, i, [expected (Y, U, V) per output frame]) ----
def _off(stream, b, i):
    """the frames of the definition with the option off: the existing decoder's answer"""
    d, at = spec(stream, b, i, extended=False)
    assert d is not None, at
    return d.frames


@functools.lru_cache(maxsize=None)
def known():
    out = {}
    c = cases()
    # the same macroblocks with one slice a row
    for name, w, h, pics in (("ipbb_cut", 48, 32, ipbb()), ("ipbb_cut_shifted", 48, 32, ipbb()), ("ip_cut", 48, 32, ipbb()[:2]), ("skip_run", 80, 16, skip_run()),
                             ("fields_cut", 48, 48, fields()), ("fields_ip_cut", 48, 48, fields()[:2]), ("many", 64, 128, many())):
        s, L, b, i = c[name]
        twin = XW.stream(w, h, uncut(pics))[0]
        assert twin != s
        out[name] = (s, b, i, _off(twin, b, i))
    rng = np.random.RandomState(35)
    out["escape"] = c["escape"][:1] + (False, False, _off(XW.stream(560, 16, [C.intra_picture(rng, 35, 1)])[0], False, False))
    # the same stream without the slice extras
    out["headers"] = (c["headers"][0], True, False, _off(XW.stream(48, 32, uncut(ipbb()))[0], True, False))
    out["headers_fields"] = (c["headers_fields"][0], True, True, _off(XW.stream(48, 48, fields())[0], True, True))
    # the same matrices loaded in the sequence header
    for name, seq in (("intra", dict(intra_matrix=A)), ("non_intra", dict(non_intra_matrix=B_)), ("both", dict(intra_matrix=A, non_intra_matrix=B_)), ("neither", {})):
        twin = XW.stream(48, 32, _ip(36), seq=seq)[0]
        out["quant_" + name] = (c["quant_" + name][0], False, False, _off(twin, False, False))
    for k in range(3):
        out["quant_beside_%d" % k] = (c["quant_beside_%d" % k][0], False, False, _off(XW.stream(48, 32, _ip(36), seq=dict(intra_matrix=A))[0], False, False))
    # per picture: an I-only twin per matrix, the picture's frame taken from the twin with its matrix
    for name, (pics, mats), b in (("quant_per_picture", quant_per_picture(), False), ("quant_coded_order", quant_coded_order(), True)):
        plain = [dict({k: v for k, v in p.items() if k != "extras"}, type=1, seq=n == 0, gop=n == 0) for n, p in enumerate(pics)]
        twins = {None: _off(XW.stream(48, 32, plain)[0], False, False)}
        for m in (A, B_):
            twins[id(m)] = _off(XW.stream(48, 32, plain, seq=dict(intra_matrix=m))[0], False, False)
        coded = [twins[None if m is None else id(m)][n] for n, m in enumerate(mats)]
        order = M.decoder.display_order([p["type"] for p in pics])
        frames = [None] * len(coded)
        for n, d in enumerate(order):
            frames[d] = coded[n]
        out[name] = (c[name][0], b, False, frames)
    # composite_display_flag 0
    p = _ip(37)
    out["composite"] = (c["composite"][0], False, True, _off(XW.stream(48, 32, p)[0], False, True))
    # literal pictures that no decoder made: flat pictures - a loaded intra matrix changes nothing but the DC path, which has no weight
    flat = lambda v: (np.full((32, 48), v, np.uint8), np.full((16, 24), v, np.uint8), np.full((16, 24), v, np.uint8))
    heavy = [99] * 64
    pics = [dict(BC.flat(70, 1), extras=[Q(intra=heavy, non_intra=heavy)], cuts=[[1], [2]]), dict(C.still_p(3, 2), cuts=[[2], [1, 2]]),
            dict(BC.flat(200, 2), extras=[Q(intra=[255] * 64)], cuts=[[1, 2], []])]
    out["flat_literal"] = (XW.stream(48, 32, pics)[0], False, False, [flat(70), flat(70), flat(200)])
    # a single AC coefficient, 7.4.2.3 by hand: F = 2 * QF * W * quantiser_scale / 32.  Level 2 under a loaded weight of 32 and level 4
    # under the default matrix's 16 (W[0][1]) are both 4 * quantiser_scale: the twin is the level-4 stream, which the existing decoder
    # reads with the default matrix
    def ac_picture(level):
        mbs = [dict(kind="intra", blocks=[dict(dc=10 if b in (0, 4, 5) and col == 0 else 0, coefs=[(0, level, False)] if b == 0 else []) for b in range(6)]) for col in range(3)]
        return dict(type=1, slices=[dict(q=6, mbs=[dict(m) for m in mbs]) for _ in range(2)])
    loaded = list(MW_default_intra())
    loaded[1] = 32
    assert MW_default_intra()[1] == 16
    s = XW.stream(48, 32, [dict(ac_picture(2), extras=[Q(intra=loaded)], cuts=[[1], [1, 2]])])[0]
    out["ac_by_hand"] = (s, False, False, _off(XW.stream(48, 32, [ac_picture(4)])[0], False, False))
    return out


def MW_default_intra():
    """6.3.11: the default intra matrix, raster order (typed from the standard's table; decoder.py's copy is not consulted)"""
    return (8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
            22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83)


# ---- the refusals: name -> (stream, b, i, the offset of the unit the definition must name) ----
@functools.lru_cache(maxsize=None)
def refusals():
    out = {}

    def base(rows=2):
        r = np.random.RandomState(41)
        return [C.intra_picture(r, 3, rows), C.random_p(r, 3, rows)]

    def of(pics, unit, nth, w=48, h=32, b=False, i=False, **kw):
        s, L = XW.stream(w, h, pics, **kw)
        return s, b, i, [a for k, a in L["units"] if k == unit][nth]

    def pieces(sl, code, *ranges):
        """slices of macroblocks [a, b) of a row's slice, each starting at its column"""
        return [dict(sl, code=code, mbs=[dict(m, incr=a + 1) if n == 0 else dict(m) for n, m in enumerate(sl["mbs"][a:b])]) for a, b in ranges]

    def I(rows=2):
        """an I picture of rows x 3 macroblocks whose DC differentials are all 0 (a macroblock may start a slice as it is)"""
        return dict(type=1, slices=[dict(q=4, mbs=[dict(kind="intra", blocks=[dict(dc=0, coefs=[(1, 3, False)]) for _ in range(6)]) for _ in range(3)]) for _ in range(rows)])

    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=1)] + pieces(r[1], 2, (0, 1), (2, 3))
    out["gap"] = of([p], "slice", 2)
    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=1)] + pieces(r[1], 2, (0, 2), (1, 3))
    out["overlap"] = of([p], "slice", 2)
    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=2), dict(r[1], code=2)]
    out["first_code_2"] = of([p], "slice", 0)
    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=1)] + pieces(r[1], 2, (1, 3))
    out["row_starts_at_column_1"] = of([p], "slice", 1)
    p = I(); r = p["slices"]
    p["slices"] = pieces(r[0], 1, (1, 3)) + [dict(r[1], code=2)]
    out["picture_starts_at_column_1"] = of([p], "slice", 0)
    p = I(3); r = p["slices"]
    p["slices"] = [dict(r[0], code=1), dict(r[1], code=2), dict(r[0], code=1), dict(r[2], code=3)]
    out["code_goes_down"] = of([p], "slice", 2, h=48)
    p = I(3); r = p["slices"]
    p["slices"] = [dict(r[0], code=1), dict(r[2], code=3)]
    out["code_jumps_by_2"] = of([p], "slice", 1, h=48)
    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=1)] + pieces(r[1], 2, (0, 1), (1, 2))
    out["last_slice_ends_short"] = of([p, C.still_p(3, 2)], "slice", 2)
    p = I(); r = p["slices"]
    p["slices"] = pieces(r[0], 1, (0, 2)) + [dict(r[1], code=2)]
    out["row_ends_short"] = of([p], "slice", 1)                    # the next row's first slice finds the row in front of it not full
    p = I(3); r = p["slices"]
    p["slices"] = [dict(r[0], code=1), dict(r[1], code=2)]
    out["ends_behind_code_mbh_minus_1"] = of([p, C.still_p(3, 3)], "picture", 1, h=48)
    out["ends_behind_code_mbh_minus_1_at_end"] = of([p], "end", 0, h=48)
    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=1), dict(r[1], code=2, mbs=[]), dict(r[1], code=2)]
    out["no_macroblock"] = of([p], "slice", 1)
    p = I(); r = p["slices"]
    p["slices"] = [dict(r[0], code=1, mbs=r[0]["mbs"] + r[0]["mbs"][:1]), dict(r[1], code=2)]
    out["one_macroblock_too_many"] = of([p], "slice", 0)
    p = I(); r = p["slices"]
    p["slices"] = pieces(r[0], 1, (0, 2)) + [dict(r[0], code=1, mbs=[dict(r[0]["mbs"][2], incr=3), dict(r[0]["mbs"][0])]), dict(r[1], code=2)]
    out["one_too_many_behind_a_cut"] = of([p], "slice", 1)
    for zeros in (23, 24, 25, 26, 27, 28, 29, 30):                 # data behind 23 zero bits and more: at every alignment but the start code's own
        p = I()
        p["slices"][0]["tail"] = "0" * zeros + "1"
        s, b, i, at = of([p], "slice", 0)
        if len(M.decoder.start_codes(s)) == len(M.decoder.start_codes(XW.stream(48, 32, [I()])[0])):      # (no start code came of it)
            out["data_behind_%d_zero_bits" % zeros] = (s, b, i, at)
    assert "data_behind_23_zero_bits" in out
    # the closing 0 of the extras missing: two information bytes end the unit at a byte's edge, the next bit is not there
    p = I(); p["slices"][1] = dict(p["slices"][1], mbs=[], header=dict(info=[200, 17], closing=False))
    s, b, i, at = of([p], "slice", 1)
    assert s[at + 8:] == b"\x00\x00\x01\xb7"                    # the unit is its start code and 32 bits: the end code follows at once
    out["closing_bit_missing"] = (s, b, i, at)
    # quant_matrix_extension
    bad = list(A); bad[17] = 0
    for name, unit in (("chroma_intra_flag", Q(intra=A, chroma=(1, 0))), ("chroma_non_intra_flag", Q(chroma=(0, 1))), ("weight_0", Q(non_intra=bad)),
                       ("truncated", Q(intra=A, non_intra=B_, cut=90)), ("truncated_in_flags", Q(intra=A, cut=68))):
        p = base(); p[1]["extras"] = [MW.USER, unit]
        out["quant_" + name] = of(p, "quant_matrix", 0)
    p = base(); p[0]["extras"] = [Q(intra=A), MW.USER, Q(non_intra=B_)]
    out["quant_twice"] = of(p, "quant_matrix", 1)
    out["quant_behind_sequence_extension"] = of(base(), "quant_matrix", 0, seq=dict(extras=[Q(intra=A)]))
    s, L = XW.stream(48, 32, base())
    at = [a for k, a in L["units"] if k == "slice"][1]
    out["quant_behind_a_slice"] = (s[:at] + Q(intra=A)[1] + s[at:], False, False, at)
    return out


ACCEPTED_NOW = {"quant_matrix_extension", "two_slices_in_a_row", "first_increment_2", "composite_display_flag", "intra_slice_flag"}


@functools.lru_cache(maxsize=None)
def older_refusals():
    """every refusal of main_cases, bpic_cases and ilace_cases that is not about a construct the option accepts:
    name -> (stream, b, i, offset) - refused at the same unit with the option on"""
    out = {}
    for name, (s, at) in C.refusals().items():
        if name not in ACCEPTED_NOW:
            out["main_" + name] = (s, False, False, at)
    for name, (s, at) in BC.refusals().items():
        if name == "skipped_last_of_row":                          # its slice ends short of the row and is not the picture's last: a slice that
            at = s.index(b"\x00\x00\x01", at + 4)                 # may be continued now, so the rule names the one behind it, which does not
        if name not in ACCEPTED_NOW:
            out["bpic_" + name] = (s, True, False, at)
    for name, (s, b, at) in IC.refusals().items():
        if name not in ACCEPTED_NOW:
            out["ilace_" + name] = (s, b, True, at)
    return out


@functools.lru_cache(maxsize=None)
def older_valid():
    """the valid cases of main_cases, bpic_cases and ilace_cases: name -> (stream, b, i) - the invariant's streams"""
    out = {}
    for name, (s, L) in C.cases().items():
        out["main_" + name] = (s, False, False)
    for name, (s, L) in BC.cases().items():
        out["bpic_" + name] = (s, True, False)
    for name, (s, L) in IC.cases().items():
        out["ilace_" + name] = (s, IC.b_flag(name, L), True)
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    """48 x 32, I P B B cut into slices, with slice extras and a quant_matrix_extension in the P picture: the stream the altered ones
    are made of"""
    pics = with_headers(cycle_cuts(ipbb(43)))
    pics[1]["extras"] = [Q(intra=A, non_intra=B_)]
    return XW.stream(48, 32, pics)


@functools.lru_cache(maxsize=None)
def altered(n=300):
    """[(name, stream)]: seeded bit flips in the slice headers (their first four bytes behind the start code), in the slice data and in
    the extension; cuts and insertions in the slice data (decoded with "decode_b_pictures" on, "decode_interlaced" off)"""
    s, L = altered_base()
    rng = np.random.RandomState(6)
    slices = [a for k, a in L["units"] if k == "slice"]
    quant = [a for k, a in L["units"] if k == "quant_matrix"][0]
    ends = {a: (L["units"][n + 1][1] if n + 1 < len(L["units"]) else len(s)) for n, (k, a) in enumerate(L["units"])}
    out = []
    for k in range(n):
        kind = k % 6
        at = slices[int(rng.randint(len(slices)))]
        if kind == 0:                                              # a slice header
            bit = 8 * (at + 4) + int(rng.randint(0, 32))
            out.append(("head%d" % bit, D.flip(s, bit)))
        elif kind == 1:                                            # the extension
            bit = int(rng.randint(8 * (quant + 4), 8 * ends[quant]))
            out.append(("quant%d" % bit, D.flip(s, bit)))
        elif kind in (2, 3):                                       # slice data
            bit = int(rng.randint(8 * (at + 4), 8 * ends[at]))
            out.append(("flip%d" % bit, D.flip(s, bit)))
        elif kind == 4:
            cut = int(rng.randint(at + 5, ends[at] + 1))
            out.append(("cut%d" % cut, s[:cut]))
        else:
            ins = int(rng.randint(at + 4, ends[at]))
            out.append(("ins%d" % ins, s[:ins] + bytes([int(rng.randint(0, 256))]) + s[ins:]))
    return out


def altered_sample():
    """an evenly sampled half, for the GPU test"""
    return altered()[::2]


def all_streams():
    """every stream of this file: (name, stream, b_pictures, interlaced)"""
    out = [(n, v[0], v[2], v[3]) for n, v in sorted(cases().items())]
    out += [("known_" + n, v[0], v[1], v[2]) for n, v in sorted(known().items())]
    out += [("refusal_" + n, v[0], v[1], v[2]) for n, v in sorted(refusals().items())]
    out += [("older_" + n, v[0], v[1], v[2]) for n, v in sorted(older_refusals().items())]
    return out + [(n, s, True, False) for n, s in altered()]
