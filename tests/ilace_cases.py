"""Interlaced frame pictures in the device decoder (option "decode_interlaced" on top of the main syntax, "decode_b_pictures" either
way): the streams it is tried on and what it must answer - shared by tests/test_ilace_cases.py (CPU) and
tests/test_gpu_decode_ilace.py.  The definition is the expectation: decoder.decode(stream, quirks=False, syntax="main", b_pictures=...,
interlaced=True) - its frames, or the offset its Refused names.  The known answers carry their expected pictures as literal arrays
that no decoder made.  Nothing here looks at what the device computes.

The streams are written by tests/ilace_writer.py at the smallest shapes at which each rule can go wrong: 32 x 32 and 48 x 48 (a field
vector needs a neighbour row and column each way; a progressive_sequence 0 stream of 48 lines is coded with four macroblock rows),
16 x 16 coded 16 x 32, 9 pictures of 32 x 128 (72 slices), and I P B B for the chunks of "decode_batch" 2.

host_lib(): the il_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_i_host.hpp compiled with g++."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import dec_cases as D
import dec_writer as W
import ilace_writer as IW
import main_cases as C

M = D.M
Refused = M.decoder.Refused


def spec(stream, b_pictures, interlaced=True):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures, interlaced=interlaced), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, b_pictures):
    key = (stream, bool(b_pictures))
    if key not in _specs:
        _specs[key] = spec(stream, b_pictures)
    return _specs[key]


_HARNESS = r"""
#include "dec_i_host.hpp"
extern "C" long long dec_i_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, int b_pictures, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_i_host::decode(es, n, layout, cap, b_pictures != 0, frames);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
extern "C" unsigned dec_i_host_rows(unsigned height, unsigned progressive) { return m2v::dec::il_mbh(height, progressive); }
extern "C" unsigned dec_i_host_type(unsigned w6, unsigned ptype) { return m2v::dec::il_type_ip(w6, ptype); }
extern "C" int dec_i_host_field_inside(int col, int row, int mvx, int mvy, int mbw, int mbh) { return m2v::dec::il_field_inside(col, row, mvx, mvy, mbw, mbh); }
extern "C" unsigned dec_i_host_row_map(unsigned x, unsigned y, unsigned dct_type) { return m2v::dec::il_luma_block(x, y, dct_type) << 8 | m2v::dec::il_luma_row(y, dct_type); }
extern "C" unsigned dec_i_host_record_bytes(void) { return (unsigned)sizeof(m2v::dec::IMb); }
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_i_host_")
        src, so = os.path.join(d, "dec_i_host.cpp"), os.path.join(d, "libdec_i_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_i_host_decode.restype = ctypes.c_longlong
        L.dec_i_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(D.Stat)]
        for f in (L.dec_i_host_rows, L.dec_i_host_type, L.dec_i_host_row_map, L.dec_i_host_record_bytes):
            f.restype = ctypes.c_uint
        _host = L
    return _host


def host_decode(stream, b_pictures, layout="i420", cap=None):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict)"""
    stream = bytes(stream)
    room = (1 << 24) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = D.Stat()
    host_lib().dec_i_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, int(bool(b_pictures)), ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    if r["status"] != D.OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r


record_of = C.record_of


def pack_streams(items):
    """[(stream, b_pictures)] -> the file tools/dec_i_host_check reads"""
    out = [struct.pack("<I", len(items))]
    for stream, b in items:
        out += [struct.pack("<IQ", int(bool(b)), len(stream)), bytes(stream)]
    return b"".join(out)


# ---- content ----
def intra_levels(mbw, mbh, levels, dct=0, ptype=1, **params):
    """a picture of intra macroblocks with DC-only blocks: levels(row, col) -> the six blocks' sample values (intra_dc_precision 0:
    one step of DC is 1)"""
    slices = []
    for row in range(mbh):
        pred, mbs = [128, 128, 128], []
        for col in range(mbw):
            lv = levels(row, col)
            blocks = []
            for b in range(6):
                comp = 0 if b < 4 else b - 3
                blocks.append(dict(dc=lv[b] - pred[comp], coefs=[]))
                pred[comp] = lv[b]
            mbs.append(dict(kind="intra", dct=dct, blocks=blocks))
        slices.append(dict(q=4, mbs=mbs))
    return dict(type=ptype, field=True, prec=0, slices=slices, **params)


A_, B_, CH = 60, 200, 90                                          # the two luma levels of the alternating picture, its chroma
ROWS = (40, 90, 140, 190)                                          # L_r: the flat luma levels of the macroblock rows of a 48 x 48 picture (four rows)
CROWS = (50, 100, 150, 200)                                        # C_r: the chroma levels


def ab_picture(mbw, mbh, dct):
    """blocks 0 / 1 of level A, 2 / 3 of level B: with dct_type 1 rows that alternate A, B; with 0 eight rows of A over eight of B"""
    return intra_levels(mbw, mbh, lambda r, c: (A_, A_, B_, B_, CH, CH), dct=dct)


def rows_picture(mbw, mbh, luma=ROWS, chroma=CROWS):
    return intra_levels(mbw, mbh, lambda r, c: (luma[r],) * 4 + (chroma[r],) * 2)


def fmb(s0, v0, s1, v1, direction="fwd", **kw):
    """a field-based macroblock: select and vector of the top-field lines, then of the bottom-field lines"""
    return dict(dict(kind="pred", motion="field", **{direction: ((s0, tuple(v0)), (s1, tuple(v1)))}), **kw)


def frmb(v, direction="fwd", **kw):
    return dict(dict(kind="pred", motion="frame", **{direction: tuple(v)}), **kw)


def pred_picture(ptype, mbw, mbh, fn, q=3, **params):
    return dict(type=ptype, field=True, slices=[dict(q=q, mbs=[m for m in (fn(row, col) for col in range(mbw)) if m is not None]) for row in range(mbh)], **params)


def legal_field(rng, col, row, mbw, mbh, most):
    for _ in range(8):
        mv = (int(rng.randint(-most, most + 1)), int(rng.randint(-most, most + 1)))
        if IW.field_inside(col, row, mv, mbw, mbh):
            return mv
    return (0, 0)


def coded(rng, m, cbp, intra=False):
    m.update(cbp=None if intra else cbp, dct=int(rng.randint(2)), blocks=[C.block(rng, intra) for _ in range(6 if intra else bin(cbp).count("1"))])
    return m


def random_il(rng, ptype, mbw, mbh, q=4, most=5, f_code=(1, 1, 1, 1), residual=2, **params):
    """a picture with frame_pred_frame_dct 0 of every kind of macroblock: intra with either dct_type, frame- and field-based in every
    direction the type allows with random selects, coded (one in `residual`) with either dct_type or not, a P picture's without a
    vector, a quantiser now and then, skipped ones (never a row's first or last; a B picture's never behind an intra macroblock and
    only where PMV[0][s], read as a frame vector, stays inside the picture)"""
    slices = []
    for row in range(mbh):
        mbs, col, pending, front, pm = [], 0, 1, None, [(0, 0), (0, 0)]      # pm: PMV[0][s] read as a frame vector
        while col < mbw:
            if 0 < col < mbw - 1 and ptype != 1 and rng.randint(4) == 0 and \
                    (ptype == 2 or (front is not None and all(W.inside(col, row, pm[s], mbw, mbh) for s in (0, 1) if front[s]))):
                if ptype == 2:
                    pm = [(0, 0), (0, 0)]
                col, pending = col + 1, pending + 1
                continue
            k = int(rng.randint(8))
            quant = int(rng.randint(1, 32)) if rng.randint(4) == 0 else None
            if ptype == 1 or k == 7:
                m = coded(rng, dict(kind="intra", incr=pending), 63, intra=True)
                front, pm = None, [(0, 0), (0, 0)]
            elif ptype == 2 and k == 6:
                m = coded(rng, dict(kind="nomc", incr=pending), int(rng.randint(1, 64)))
                front, pm = (1, 0), [(0, 0), (0, 0)]
            else:
                d = (1, 0) if ptype == 2 else ((1, 0), (0, 1), (1, 1))[k % 3]
                field = int(rng.randint(2))
                vs = []
                for s in (0, 1):
                    if not d[s]:
                        vs.append(None)
                    elif field:
                        v = tuple((int(rng.randint(2)), legal_field(rng, col, row, mbw, mbh, most)) for r in (0, 1))
                        vs.append(v)
                        pm[s] = (v[0][1][0], 2 * v[0][1][1])
                    else:
                        vs.append(W.legal_vector(rng, col, row, mbw, mbh, most=most))
                        pm[s] = vs[-1]
                m = dict(kind="pred", motion="field" if field else "frame", fwd=vs[0], bwd=vs[1], incr=pending)
                if rng.randint(residual) == 0:
                    coded(rng, m, int(rng.randint(1, 64)))
                else:
                    quant = None
                front = d
            if quant is not None:
                m["quant"] = quant
            mbs.append(m)
            col, pending = col + 1, 1
        slices.append(dict(q=q, mbs=mbs))
    return dict(type=ptype, field=True, f_code=f_code, slices=slices, **params)


def pictures(rng, letters, mbw, mbh, **kw):
    return [random_il(rng, " IPB".index(c), mbw, mbh, **kw) for c in letters]


# ---- the known answers: name -> (stream, log, [expected (Y, U, V) per output frame; None: not stated]) ----
def _planes(y, cu, w, h):
    """(Y, U, V) from luma rows y (a list of h row levels, or an array) and chroma row levels cu"""
    Y = np.repeat(np.asarray(y, np.uint8)[:h, None], w, axis=1) if np.ndim(y) == 1 else np.asarray(y, np.uint8)[:h, :w]
    Cc = np.repeat(np.asarray(cu, np.uint8)[:(h + 1) // 2, None], (w + 1) // 2, axis=1)
    return (Y, Cc, Cc.copy())


@functools.lru_cache(maxsize=None)
def known():
    out = {}
    alt = [A_, B_] * 16                                            # 32 rows that alternate A, B
    halves = ([A_] * 8 + [B_] * 8) * 2
    flat_c = [CH] * 16
    # field DCT: the same bits but for dct_type
    for dct, rows in ((1, alt), (0, halves)):
        s, L = IW.stream(32, 32, [ab_picture(2, 2, dct)])
        out["field_dct_%d" % dct] = (s, L, [_planes(rows, flat_c, 32, 32)])
    # field selects on the alternating picture: zero vectors, no residual
    for (s0, s1), rows in (((1, 0), [B_, A_] * 16), ((0, 0), [A_] * 32), ((1, 1), [B_] * 32), ((0, 1), alt)):
        p = pred_picture(2, 2, 2, lambda r, c: fmb(s0, (0, 0), s1, (0, 0)))
        s, L = IW.stream(32, 32, [ab_picture(2, 2, 1), p])
        out["selects_%d%d" % (s0, s1)] = (s, L, [_planes(alt, flat_c, 32, 32), _planes(rows, flat_c, 32, 32)])
    # the field vector's scale, the predictor doubled for a frame vector and halved again for a field vector: 48 x 48 is four
    # macroblock rows of levels L_r; column 0 field-based with vertical 16 (8 field lines = 16 frame lines), column 1 frame-based
    # and column 2 field-based, both with zero deltas (the log says so); the last row stands still
    ref = rows_picture(3, 4)
    ref_rows = [ROWS[y // 16] for y in range(64)]
    ref_c = [CROWS[y // 8] for y in range(32)]

    def scale(r, c):
        if r == 3:
            return fmb(0, (0, 0), 1, (0, 0))
        return (fmb(0, (0, 16), 1, (0, 16)), frmb((0, 32)), fmb(0, (0, 16), 1, (0, 16)))[c]
    s, L = IW.stream(48, 48, [ref, pred_picture(2, 3, 4, scale, f_code=(1, 3, 1, 1))])
    up_rows = [ROWS[min(y // 16 + 1, 3)] for y in range(64)]
    up_c = [CROWS[min(y // 8 + 1, 3)] for y in range(32)]
    out["vector_scale"] = (s, L, [_planes(ref_rows, ref_c, 48, 48), _planes(up_rows, up_c, 48, 48)])
    # a frame vector of 16 moves the picture only 8 lines
    s, L = IW.stream(48, 48, [ref, pred_picture(2, 3, 4, lambda r, c: frmb((0, 16) if r < 3 else (0, 0)), f_code=(1, 3, 1, 1))])
    eight = [ROWS[min((y + 8) // 16, 3)] if y < 48 else ROWS[3] for y in range(64)]
    eight_c = [CROWS[min((y + 4) // 8, 3)] if y < 24 else CROWS[3] for y in range(32)]
    out["frame_vector_16"] = (s, L, [_planes(ref_rows, ref_c, 48, 48), _planes(eight, eight_c, 48, 48)])
    # the field half-sample: vertical 1 in the top field of the alternating picture lies between A and A; a frame half-sample would
    # give (A + B + 1) >> 1.  Both halves from the top field (the last row stands still, from its own parities)
    p = pred_picture(2, 2, 2, lambda r, c: fmb(0, (0, 1), 0, (0, 1)) if r == 0 else fmb(0, (0, 0), 1, (0, 0)))
    s, L = IW.stream(32, 32, [ab_picture(2, 2, 1), p])
    out["field_half_sample"] = (s, L, [_planes(alt, flat_c, 32, 32), _planes([A_] * 16 + alt[16:], flat_c, 32, 32)])
    # the chroma vector: vertical -1 and -3 in macroblock row 1 over flat luma and chroma rows C_r: / 2 toward zero is 0 and -1 (a
    # shift would say -1 and -2).  0 reads the row's own lines; -1 is a half sample up: the first line of either field is the mean
    # with the row above, the other three are the row's own
    flat_l = (120, 120, 120, 120)
    for vy, first in ((-1, CROWS[1]), (-3, (CROWS[0] + CROWS[1] + 1) >> 1)):
        p = pred_picture(2, 3, 4, lambda r, c: fmb(0, (0, vy), 1, (0, vy)) if r == 1 else fmb(0, (0, 0), 1, (0, 0)), f_code=(1, 1, 1, 1))
        s, L = IW.stream(48, 48, [rows_picture(3, 4, luma=flat_l), p])
        c_rows = list(ref_c)
        c_rows[8] = c_rows[9] = first
        out["chroma_vector_%d" % -vy] = (s, L, [_planes([120] * 64, ref_c, 48, 48), _planes([120] * 64, c_rows, 48, 48)])
    # a B picture's skipped macroblock behind a field-based one: PMV[0][0] read as a frame vector is twice the field vector's 16 -
    # sixteen lines, the next row's level; the field vector itself read as a frame vector would move eight
    def skip(r, c):
        if r == 3:
            return fmb(0, (0, 0), 1, (0, 0))
        return (fmb(0, (0, 16), 1, (0, 16)), None, frmb((0, 32), incr=2))[c]
    still = dict(C.still_p(3, 4), ext=dict(progressive_frame=0))
    s, L = IW.stream(48, 48, [ref, still, pred_picture(3, 3, 4, skip, f_code=(1, 3, 1, 1))])
    same = _planes(ref_rows, ref_c, 48, 48)
    out["b_skip"] = (s, L, [same, _planes(up_rows, up_c, 48, 48), same])
    # sixteen lines: two macroblock rows, two slices, the second cropped away
    s, L = IW.stream(16, 16, [rows_picture(1, 2, luma=(70, 180), chroma=(110, 30))])
    out["sixteen_lines"] = (s, L, [_planes([70] * 16, [110] * 8, 16, 16)])
    return out


# ---- the valid cases ----
@functools.lru_cache(maxsize=None)
def cases():
    """name -> (stream, log): every valid stream of the suite, the known answers among them"""
    out = {name: (s, L) for name, (s, L, _) in known().items()}
    rng = np.random.RandomState(7117)
    out["ip_32"] = IW.stream(32, 32, pictures(rng, "IPP", 2, 2))
    out["ipb_32"] = IW.stream(32, 32, pictures(rng, "IPBB", 2, 2))
    out["ip_48"] = IW.stream(48, 48, pictures(rng, "IPP", 3, 4, most=9, f_code=(2, 2, 1, 1)))
    out["ipb_48"] = IW.stream(48, 48, pictures(rng, "IPBBPB", 3, 4, most=9, f_code=(2, 3, 3, 2)))
    out["ipb_16"] = IW.stream(16, 16, pictures(rng, "IPB", 1, 2))
    # pictures with frame_pred_frame_dct 1 between field pictures in one stream; both scans, both scale types, a precision, a matrix
    mixed = [random_il(rng, 1, 3, 4, alt=1, prec=1), dict(C.random_p(rng, 3, 4), ext=dict(progressive_frame=0)), random_il(rng, 3, 3, 4, qst=1, alt=1, tff=0, rff=1),
             random_il(rng, 2, 3, 4, qst=1, prec=3, chroma_420_type=1)]
    out["mixed"] = IW.stream(48, 48, mixed, seq=dict(non_intra_matrix=C.MATRIX_B, intra_matrix=C.MATRIX_A), end=False, tail=3)
    # 72 slices: more than one wavefront of the slice walk
    out["wide"] = IW.stream(32, 128, pictures(rng, "IPBBPBBPB", 2, 8, residual=6))
    # I P B B for "decode_batch" 2: the B pictures' field predictions read anchors carried between chunks
    out["ipbb"] = IW.stream(48, 48, pictures(rng, "IPBB", 3, 4, most=7))
    # an odd number of progressive macroblock rows: 40 lines are three rows there, four here
    out["crop_40"] = IW.stream(40, 40, pictures(rng, "IPB", 3, 4))
    return out


def b_flag(name, L=None):
    """whether a case is decoded with "decode_b_pictures" on: always where it has B pictures, and for every second one of the others"""
    L = L or cases()[name][1]
    return 3 in L["pictures"] or sorted(cases()).index(name) % 2 == 0


# ---- the refusals ----
@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (stream, b_pictures, the offset of the unit the definition must name)"""
    out = {}

    def base():
        r = np.random.RandomState(61)
        return pictures(r, "IPB", 2, 2)

    def of(pics, unit, nth, b=True, w=32, h=32, **kw):
        s, L = IW.stream(w, h, pics, strict=False, **kw)
        return s, b, [a for k, a in L["units"] if k == unit][nth]

    still = lambda: fmb(0, (0, 0), 1, (0, 0))
    for bits in (0, 3):
        p = base(); p[1]["slices"][1]["mbs"] = [dict(still(), motion_bits=bits), still()]
        out["frame_motion_type_%d" % bits] = of(p, "slice", 3)
        p = base(); p[2]["slices"][0]["mbs"] = [still(), dict(fmb(0, (0, 0), 1, (0, 0), "bwd"), motion_bits=bits)]
        out["frame_motion_type_%d_in_b" % bits] = of(p, "slice", 4)
    out["field_in_progressive_sequence"] = of(base(), "picture_ext", 0, seq=dict(progressive=1))
    p = base(); p[1]["ext"] = dict(progressive_frame=1)
    out["field_in_progressive_frame"] = of(p, "picture_ext", 1)
    # one half sample outside each of the four field edges, in luma
    for name, row, col, v in (("left", 0, 0, (-1, 0)), ("right", 0, 1, (1, 0)), ("top", 0, 1, (0, -1)), ("bottom", 1, 0, (0, 1))):
        for r in (0, 1):
            p = base()
            mbs = [still(), still()]
            mbs[col] = fmb(0, v if r == 0 else (0, 0), 1, v if r == 1 else (0, 0))
            p[1]["slices"][row]["mbs"] = mbs
            out["field_vector_%s_%d" % (name, r)] = of(p, "slice", 2 + row)
    p = base(); p[2]["slices"][1]["mbs"] = [still(), fmb(1, (0, 0), 0, (0, 1), "bwd")]
    out["backward_field_vector_bottom"] = of(p, "slice", 5)
    # a B picture's skipped macroblock carries PMV[0][0] to the next column, where it leaves the picture
    p = pictures(np.random.RandomState(62), "IPB", 3, 2)
    p[2]["f_code"] = (3, 1, 3, 1)
    p[2]["slices"][0]["mbs"] = [fmb(0, (34, 0), 1, (34, 0)), dict(still(), incr=2)]
    out["skipped_vector_leaves"] = of(p, "slice", 4, w=48)
    p = pictures(np.random.RandomState(63), "IPB", 3, 2)
    p[2]["slices"][0]["mbs"] = [dict(kind="intra", blocks=[dict(dc=0, coefs=[]) for _ in range(6)]), dict(still(), incr=2)]
    out["skipped_behind_intra"] = of(p, "slice", 4, w=48)
    p = pictures(np.random.RandomState(64), "IPB", 3, 2)
    p[0]["slices"][0]["mbs"] = [p[0]["slices"][0]["mbs"][0], dict(p[0]["slices"][0]["mbs"][2], incr=2)]
    out["skipped_in_i"] = of(p, "slice", 0, w=48)
    # a B picture with "decode_b_pictures" off: at its picture header
    out["b_picture_with_b_off"] = of(base(), "picture", 2, b=False)
    # the slice code past the rows of the rule: a third slice row in a 32-line picture
    p = base(); p[0]["slices"].append(dict(p[0]["slices"][1]))
    out["third_slice"] = of(p, "slice", 2)
    # sixteen lines written with one macroblock row, as a progressive sequence would: the picture is short of a slice
    out["sixteen_lines_one_row"] = of(pictures(np.random.RandomState(65), "IP", 1, 1), "picture", 1, w=16, h=16, rows=1)
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    """32 x 32, I P B B of field pictures: the stream the altered ones are made of"""
    rng = np.random.RandomState(515)
    return IW.stream(32, 32, pictures(rng, "IPBB", 2, 2, most=4, f_code=(2, 1, 1, 2)))


@functools.lru_cache(maxsize=None)
def altered(flips=240, edits=60):
    """[(name, stream)]: seeded bit flips, cuts and insertions in the slice data of every picture (decoded with "decode_b_pictures" on)"""
    s, L = altered_base()
    first = [a for k, a in L["units"] if k == "slice"][0]
    rng = np.random.RandomState(4)
    lo, hi = 8 * (first + 4), 8 * len(s)
    slices = [a for k, a in L["units"] if k == "slice"] + [len(s)]
    others = [a for k, a in L["units"] if k != "slice"]

    def in_slice(byte):
        return max(a for a in slices[:-1] + others if a <= byte) in slices
    out = []
    while len(out) < flips:
        bit = int(rng.randint(lo, hi))
        if in_slice(bit >> 3):
            out.append(("flip%d" % bit, D.flip(s, bit)))
    k = 0
    while k < edits:
        at = int(rng.randint(lo // 8, hi // 8))
        if not in_slice(at):
            continue
        out.append(("cut%d" % at, s[:at]) if k % 2 else ("ins%d" % at, s[:at] + bytes([int(rng.randint(0, 256))]) + s[at:]))
        k += 1
    return out


def all_streams():
    """every stream of this file: (name, stream, b_pictures)"""
    out = [(n, s, b_flag(n, L)) for n, (s, L) in sorted(cases().items())] + [("refusal_" + n, s, b) for n, (s, b, _) in sorted(refusals().items())]
    return out + [(n, s, True) for n, s in altered()]
