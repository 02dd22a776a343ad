"""B pictures in the device decoder (option "decode_b_pictures" on top of the main syntax): the streams it is tried on and what it
must answer - shared by tests/test_bpic_cases.py (CPU) and tests/test_gpu_decode_bpic.py.  The definition is the expectation:
decoder.decode(stream, quirks=False, syntax="main", b_pictures=True) - its frames in display order, or the offset its Refused names.
Nothing here looks at what the device computes.

The streams are written by tests/bpic_writer.py, 48 x 32 unless a case says otherwise (160 x 96 for the wraps, 40 x 24 and 17 x 17 for
the crop, 32 x 32 for the altered streams, 336 x 64 for the one size above the small ones).

host_lib(): the bp_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_b_host.hpp compiled with g++."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import bpic_writer as BW
import dec_cases as D
import dec_writer as W
import main_cases as C
import main_writer as MW

M = D.M
Refused = M.decoder.Refused


def spec(stream, b_pictures=True):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream):
    if stream not in _specs:
        _specs[stream] = spec(stream)
    return _specs[stream]


_HARNESS = r"""
#include "dec_b_host.hpp"
extern "C" long long dec_b_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_b_host::decode(es, n, layout, cap, frames);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
extern "C" unsigned dec_b_host_type(unsigned w6) { return m2v::dec::vlc_type_b(w6); }
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_b_host_")
        src, so = os.path.join(d, "dec_b_host.cpp"), os.path.join(d, "libdec_b_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_b_host_decode.restype = ctypes.c_longlong
        L.dec_b_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(D.Stat)]
        L.dec_b_host_type.restype = ctypes.c_uint
        _host = L
    return _host


def host_decode(stream, layout="i420", cap=None):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict)"""
    stream = bytes(stream)
    room = (1 << 24) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = D.Stat()
    host_lib().dec_b_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    if r["status"] != D.OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r


record_of = C.record_of


# ---- content ----
def flat(value, ptype, mbw=3, mbh=2, **params):
    """an I picture, or a P picture of intra macroblocks, whose every sample is `value` (intra_dc_precision 0: one step of DC is 1)"""
    slices = []
    for row in range(mbh):
        mbs = [dict(kind="intra", blocks=[dict(dc=(value - 128) if col == 0 and b in (0, 4, 5) else 0, coefs=[]) for b in range(6)]) for col in range(mbw)]
        slices.append(dict(q=4, mbs=mbs))
    return dict(type=ptype, prec=0, slices=slices, **params)


def pred(fwd=None, bwd=None, rng=None, cbp=None, quant=None, incr=1):
    """a predicted macroblock of a B picture; with rng and cbp: coded, with blocks"""
    m = dict(kind="pred", fwd=fwd, bwd=bwd, incr=incr)
    if cbp:
        m.update(cbp=cbp, blocks=[C.block(rng, False) for _ in range(bin(cbp).count("1"))])
    if quant is not None:
        m["quant"] = quant
    return m


def intra_mb(rng, quant=None, incr=1):
    m = dict(kind="intra", incr=incr, blocks=[C.block(rng, True) for _ in range(6)])
    if quant is not None:
        m["quant"] = quant
    return m


def b_picture(rows, q=3, **params):
    return dict(type=3, slices=[dict(q=q, mbs=list(r)) for r in rows], **params)


def still_b(direction, mbw=3, mbh=2, skipped=False):
    """a B picture that predicts with zero vectors and no residual; skipped: all but the rows' ends skipped"""
    kw = dict(fwd=(0, 0) if "f" in direction else None, bwd=(0, 0) if "b" in direction else None)
    row = [pred(**kw), pred(incr=mbw - 1, **kw)] if skipped else [pred(**kw) for _ in range(mbw)]
    return b_picture([[dict(m) for m in row] for _ in range(mbh)])


def random_b(rng, mbw, mbh, q=4, most=6, f_code=(1, 1, 1, 1), **params):
    """a B picture of every kind of macroblock: each direction and both, coded or not, a quantiser now and then, intra, skipped ones
    (never a row's first or last, never behind an intra macroblock) whose inherited vectors stay inside the picture"""
    slices = []
    for row in range(mbh):
        mbs, col, pending, front, pmv = [], 0, 1, None, [(0, 0), (0, 0)]
        while col < mbw:
            if 0 < col < mbw - 1 and front is not None and rng.randint(4) == 0 and all(W.inside(col, row, pmv[d], mbw, mbh) for d in (0, 1) if front[d]):
                col, pending = col + 1, pending + 1
                continue
            kind = int(rng.randint(8))
            if kind == 7:
                mbs.append(intra_mb(rng, quant=int(rng.randint(1, 32)) if rng.randint(3) == 0 else None, incr=pending))
                front, pmv = None, [(0, 0), (0, 0)]
            else:
                d = (1, 0) if kind < 2 else (0, 1) if kind < 4 else (1, 1)
                mv = [W.legal_vector(rng, col, row, mbw, mbh, most=most) if d[k] else None for k in (0, 1)]
                coded = rng.randint(2) == 1
                quant = int(rng.randint(1, 32)) if coded and rng.randint(3) == 0 else None
                mbs.append(pred(mv[0], mv[1], rng, cbp=int(rng.randint(1, 64)) if coded else None, quant=quant, incr=pending))
                front, pmv = d, [mv[k] if d[k] else pmv[k] for k in (0, 1)]
            col, pending = col + 1, 1
        slices.append(dict(q=q, mbs=mbs))
    return dict(type=3, f_code=f_code, slices=slices, **params)


ORDERS = ("IPBBPBB", "IPBPBBBP", "IPPBIBBP", "IPBBI")


def order_pictures(rng, letters, mbw=3, mbh=2):
    """the coded sequence `letters` with random content; no GOP header but the stream's first, and an open-GOP one in front of an I
    picture that is not the first"""
    pics = []
    for k, c in enumerate(letters):
        if c == "I":
            pics.append(C.intra_picture(rng, mbw, mbh, gop=True, open_gop=True) if k else C.intra_picture(rng, mbw, mbh))
        elif c == "P":
            pics.append(C.random_p(rng, mbw, mbh))
        else:
            pics.append(random_b(rng, mbw, mbh))
    return pics


def half_pel_pictures(rng):
    """two B pictures of 48 x 32 whose twelve macroblocks carry the four (hx, hy) combinations forward, backward and in both
    directions - different vectors in the two directions -, f_codes that differ between the directions"""
    cells = [(d, hx, hy) for d in ("f", "b", "fb") for hx in (0, 1) for hy in (0, 1)]
    pics = []
    for k in range(2):
        rows = []
        for row in range(2):
            mbs = []
            for col in range(3):
                d, hx, hy = cells[6 * k + 3 * row + col]
                sx, sy = (1 if col < 2 else -1), (1 if row == 0 else -1)
                f = (sx * (2 * (col == 0) + hx), sy * (2 + hy))
                b = (sx * (4 * (col != 1) + hx), sy * hy)
                mbs.append(pred(f if "f" in d else None, b if "b" in d else None, rng, cbp=(0b100001 if col == 1 else None)))
            rows.append(mbs)
        pics.append(b_picture(rows, f_code=(2, 3, 4, 1) if k else (1, 2, 3, 3)))
    return pics


def wrap_picture(f):
    """160 x 96, B, every f_code f (1 .. 4): zero vectors in both directions but for row 2 (forward) and row 3 (backward), whose columns
    4, 5, 6 carry +80, -80 and +48 pel at most, cut to the range: each delta the short way round leaves the range and the decoder wraps
    (main_cases.fcode_picture's construction, once per direction)"""
    F = 1 << (f - 1)
    hi, lo = 16 * F - 1, -16 * F
    vs = {4: (min(hi, 160), 0), 5: (max(lo, -160), 0), 6: (min(hi, 96), 0)}
    rows = []
    for row in range(6):
        if row == 2:
            rows.append([pred(fwd=vs.get(col, (0, 0))) for col in range(10)])
        elif row == 3:
            rows.append([pred(bwd=vs.get(col, (0, 0))) for col in range(10)])
        else:
            rows.append([pred(fwd=(0, 0), bwd=(0, 0)) for col in range(10)])
    return b_picture(rows, f_code=(f, f, f, f))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (stream, log): every valid stream with B pictures of the suite"""
    out = {}
    rng = np.random.RandomState(3003)
    anchors = lambda mbw=3, mbh=2: [C.intra_picture(rng, mbw, mbh), C.random_p(rng, mbw, mbh)]
    # every line of Table B-4 in two pictures, a macroblock quantiser on the three lines that carry one (and on the intra one)
    b1 = b_picture([[pred((2, 1), (1, 2)), pred((1, 1), (-1, 0), rng, cbp=45), pred(None, (-3, 1))],
                    [pred(None, (2, -2), rng, cbp=7), pred((3, -1), None), pred((-2, -2), None, rng, cbp=32)]])
    b2 = b_picture([[intra_mb(rng), pred((1, 0), (0, 1), rng, cbp=63, quant=9), pred((-1, 2), None, rng, cbp=12, quant=2)],
                    [pred(None, (1, -1), rng, cbp=1, quant=31), intra_mb(rng, quant=5), pred((-2, -1), (-1, -1))]])
    out["types"] = BW.stream(48, 32, anchors() + [b1, b2])
    # skipped behind forward-only, backward-only and bidirectional macroblocks, with vectors the skipped one carries to its column
    b1 = b_picture([[pred((5, 3), None, rng, cbp=9), pred((-2, 3), None, incr=2)],
                    [pred(None, (4, -3)), pred(None, (-1, -2), rng, cbp=3, incr=2)]])
    b2 = b_picture([[pred((3, 2), (6, 1)), pred((0, 0), (-4, 0), incr=2)],
                    [pred((1, -1), None), pred(None, (-1, -3), incr=2)]])
    out["skips"] = BW.stream(48, 32, anchors() + [b1, b2])
    # an intra macroblock between two predicted ones; the unused direction's predictor surviving a macroblock that does not use it
    b1 = b_picture([[pred((4, 2), (2, 4)), intra_mb(rng), pred((-2, 2), (-4, 2))],
                    [pred((4, -2), (6, 0)), pred((2, -2), None, rng, cbp=5), pred(None, (-2, -4))]])
    out["predictors"] = BW.stream(48, 32, anchors() + [b1])
    # known answers: flat anchors of 100 and 103
    for name, b in (("still_forward", still_b("f")), ("still_backward", still_b("b")), ("still_both", still_b("fb")), ("still_skipped", still_b("fb", skipped=True))):
        out[name] = BW.stream(48, 32, [flat(100, 1), flat(103, 2), b])
    # half-pel in every combination and direction
    out["half_pel"] = BW.stream(48, 32, anchors() + half_pel_pictures(rng))
    # a wrap in each direction for f_codes 1 .. 4
    out["wraps"] = BW.stream(160, 96, [C.intra_picture(rng, 10, 6), C.still_p(10, 6)] + [wrap_picture(f) for f in (1, 2, 3, 4)])
    # coded orders
    for letters in ORDERS:
        out["order_" + letters] = BW.stream(48, 32, order_pictures(rng, letters))
    # the crop
    out["size_40x24"] = BW.stream(40, 24, order_pictures(rng, "IPBB", 3, 2))
    out["size_17x17"] = BW.stream(17, 17, order_pictures(rng, "IPBB", 2, 2))
    # parameters of the main syntax inside B pictures: both scans, both scale types, a matrix, precisions; transparent units behind a B picture's extension
    pics = [C.intra_picture(rng, 3, 2, prec=1, alt=1), C.random_p(rng, 3, 2, qst=1, f_code=(2, 2)),
            random_b(rng, 3, 2, alt=1, qst=1, prec=3, f_code=(2, 1, 1, 3), extras=[MW.USER, MW.PICTURE_DISPLAY]), random_b(rng, 3, 2, alt=0, qst=0, f_code=(3, 3, 2, 2))]
    out["params"] = BW.stream(48, 32, pics, seq=dict(non_intra_matrix=C.MATRIX_B, intra_matrix=C.MATRIX_A), end=False, tail=3)
    return out


@functools.lru_cache(maxsize=None)
def wide():
    """336 x 64 (21 x 4 macroblocks), I P and sixteen B pictures - 72 slices: more than one wavefront of the slice launch, mbw over 16.
    Mostly predicted macroblocks without residual (the definition reads them quickly), a coded and a skipped one in every row"""
    rng = np.random.RandomState(336)
    mbw, mbh = 21, 4
    pics = [C.intra_picture(rng, mbw, mbh), C.still_p(mbw, mbh)]
    for k in range(16):
        rows = []
        for row in range(mbh):
            sy = 1 if row < 2 else -1
            mbs = []
            for col in range(mbw):
                sx = 1 if col < 10 else -1
                f, b = (sx * ((k + col) % 7), sy * ((k + row) % 5)), (sx * ((2 * k + col) % 9), sy * ((k + 3 * row) % 6))
                d = (k + col + row) % 3
                m = pred(f if d != 1 else None, b if d != 0 else None, rng, cbp=33 if col == 5 else None)
                if col == 12:                                       # skipped: column 12 is left out, 13 carries the increment
                    continue
                if col == 13:
                    m["incr"] = 2
                if col in (11, 13):                                 # the vectors in front of and behind the skipped one: small, inward for all three columns
                    m.update(fwd=(-2, sy) if m["fwd"] else None, bwd=(-1, 2 * sy) if m["bwd"] else None)
                mbs.append(m)
            rows.append(mbs)
        pics.append(b_picture(rows))
    return BW.stream(336, 64, pics)


# ---- the refusals ----
@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (stream, the offset of the unit the definition must name)"""
    out = {}

    def base():
        r = np.random.RandomState(6)
        return [C.intra_picture(r, 3, 2), C.random_p(r, 3, 2), random_b(r, 3, 2)]

    def of(pics, unit, nth, **kw):
        s, L = BW.stream(48, 32, pics, strict=False, **kw)
        return s, [a for k, a in L["units"] if k == unit][nth]

    rng = np.random.RandomState(78)
    p = base()
    out["b_second"] = of([p[0], p[2]], "picture", 1)
    out["b_first"] = of([p[2], p[0], p[1]], "picture", 0)
    out["b_second_no_display"] = of([p[0], p[2]], "picture", 1, seq=dict(display=False))
    for v in (0, 10, 15):
        p = base(); p[2]["ext_f_code"] = (1, 1, v, 1)
        out["backward_f_code_%d" % v] = of(p, "picture_ext", 2)
    p = base(); p[2]["ext_f_code"] = (1, 1, 1, 0)
    out["backward_f_code_v_0"] = of(p, "picture_ext", 2)
    p = base(); p[2]["ext_f_code"] = (15, 1, 1, 1)
    out["forward_f_code_15_in_b"] = of(p, "picture_ext", 2)
    p = base(); p[2]["full_pel_backward"] = 1
    out["full_pel_backward_vector"] = of(p, "picture", 2)
    p = base(); p[2]["slices"][1]["mbs"] = [intra_mb(rng), pred((0, 0), None, incr=2)]
    out["skipped_behind_intra"] = of(p, "slice", 5)
    p = base(); p[2]["slices"][0]["mbs"] = [pred((0, 0), None), dict(pred((0, 0), None), type_bits="000000"), pred((0, 0), None)]
    out["type_000000"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][0]["mbs"] = [pred((0, 0), (-1, 0)), pred((0, 0), None), pred((0, 0), None)]
    out["backward_vector_outside"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][1]["mbs"] = [pred((0, 0), (0, 1)), pred((0, 0), None), pred((0, 0), None)]
    out["backward_vector_below"] = of(p, "slice", 5)
    p = base(); p[2]["f_code"] = (3, 1, 3, 1); p[2]["slices"][0]["mbs"] = [pred((34, 0), None), pred((0, 0), None, incr=2)]
    out["skipped_vector_leaves"] = of(p, "slice", 4)
    p = base(); p[2]["f_code"] = (3, 1, 3, 1); p[2]["slices"][0]["mbs"] = [pred(None, (34, 0)), pred(None, (0, 0), incr=2)]
    out["skipped_backward_vector_leaves"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][0]["mbs"] = [pred((0, 0), None, incr=2), pred((0, 0), None)]
    out["first_increment_2"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][0]["mbs"] = [pred((0, 0), None), pred((0, 0), None)]
    out["skipped_last_of_row"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][0]["mbs"] = [pred((0, 0), None), pred((0, 0), None, incr=3)]
    out["increment_past_the_row"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][0]["mbs"][0] = dict(intra_mb(rng), quant=0)
    out["macroblock_quant_0"] = of(p, "slice", 4)
    p = base(); p[2] = dict(C.intra_picture(rng, 3, 2), type=4)
    out["d_picture"] = of(p, "picture", 2)
    p = base(); p[2]["ext"] = dict(frame_pred_frame_dct=0)
    out["frame_pred_frame_dct_0"] = of(p, "picture_ext", 2)
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    """32 x 32, I P B B: the stream the altered ones are made of"""
    rng = np.random.RandomState(199)
    pics = [C.intra_picture(rng, 2, 2), C.random_p(rng, 2, 2, most=4), random_b(rng, 2, 2, most=4, f_code=(2, 1, 1, 2)), random_b(rng, 2, 2, most=4)]
    return BW.stream(32, 32, pics)


@functools.lru_cache(maxsize=None)
def altered(flips=260, edits=80):
    """[(name, stream)]: every bit of the first B picture's header and coding extension flipped; seeded flips, cuts and insertions in
    the slices of the B pictures"""
    s, L = altered_base()
    pic = [a for k, a in L["units"] if k == "picture"][2]
    first = [a for k, a in L["units"] if k == "slice"][4]
    out = [("bit%d" % bit, D.flip(s, bit)) for bit in range(8 * pic, 8 * first)]
    rng = np.random.RandomState(2)
    lo, hi = 8 * (first + 4), 8 * len(s)
    out += [("flip%d" % bit, D.flip(s, int(bit))) for bit in rng.randint(lo, hi, size=flips)]
    for k in range(edits):
        at = int(rng.randint(lo // 8, hi // 8))
        out.append(("cut%d" % at, s[:at]) if k % 2 else ("ins%d" % at, s[:at] + bytes([int(rng.randint(0, 256))]) + s[at:]))
    return out


def all_streams():
    """every stream of this file: (name, stream)"""
    out = [(n, s) for n, (s, _) in sorted(cases().items())] + [("refusal_" + n, s) for n, (s, _) in sorted(refusals().items())]
    return out + list(altered())
