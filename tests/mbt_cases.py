"""Table B-15, concealment motion vectors and dual prime in the device decoder (option "decode_mb_tools" on top of "decode_extended",
"decode_b_pictures" and "decode_interlaced" either way): the streams it is tried on and what it must answer - shared by
tests/test_mbt_cases.py (CPU) and tests/test_gpu_decode_mbt.py.  The definition is the expectation:
decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=..., extended=True, mb_tools=True) - its frames, or the
offset its Refused names.  The known answers are frames the new code did not make:
   Table B-15     the definition WITH THE OPTION OFF on the twin stream: the same macroblocks written with intra_vlc_format 0
   concealment    the same on the twin written without the flag and without the vectors
   dual prime     there is no twin syntax: tests/mbt_ref.py computes the frames from what the writer was told to write, and one
                  picture is a literal
Nothing here looks at what the device computes.

The streams are written by tests/mbt_writer.py at the smallest shapes at which each rule can go wrong: 48 x 32 where the rule is not
about fields, 48 x 64 with progressive_sequence 0 (four macroblock rows: a dual-prime vector with vy near 0 reads field line -1 in the
top row and is refused there), 16 x 272 for every code of Table B-15 with both signs.

host_lib(): the t_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_t_host.hpp compiled with g++."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import arith_cases as AC
import bpic_cases as BC
import dec_cases as D
import ext_cases as X
import ilace_cases as IC
import ilace_writer as IW
import main_cases as C
import mbt_ref as TR
import mbt_writer as TW

M = D.M
Refused = M.decoder.Refused


def spec(stream, b_pictures, interlaced, mb_tools=True, extended=True):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures, interlaced=interlaced, extended=extended,
                                mb_tools=mb_tools), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, b_pictures, interlaced, mb_tools=True, extended=True):
    key = (stream, bool(b_pictures), bool(interlaced), bool(mb_tools), bool(extended))
    if key not in _specs:
        _specs[key] = spec(stream, b_pictures, interlaced, mb_tools, extended)
    return _specs[key]


_HARNESS = r"""
#include "dec_t_host.hpp"
extern "C" long long dec_t_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, int b_pictures, int interlaced, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_t_host::decode(es, n, layout, cap, b_pictures != 0, interlaced != 0, frames);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
// vlc_ac15 over every window of `bits` bits (the rest of the 32 zero, then one): out[w] = length | run << 8 | level << 16, or 0
extern "C" void dec_t_host_ac15(unsigned bits, unsigned fill, uint32_t *out)
{
    for (uint32_t w = 0; w < (1u << bits); ++w) out[w] = m2v::dec::vlc_ac15(w << (32u - bits) | (fill ? (1u << (32u - bits)) - 1u : 0u));
}
extern "C" int dec_t_host_half(int a) { return m2v::dec::t_half(a); }
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_t_host_")
        src, so = os.path.join(d, "dec_t_host.cpp"), os.path.join(d, "libdec_t_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_t_host_decode.restype = ctypes.c_longlong
        L.dec_t_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(D.Stat)]
        L.dec_t_host_ac15.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
        _host = L
    return _host


def host_decode(stream, b_pictures, interlaced, layout="i420", cap=None):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict)"""
    stream = bytes(stream)
    room = (1 << 22) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = D.Stat()
    host_lib().dec_t_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, int(bool(b_pictures)), int(bool(interlaced)), ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    if r["status"] != D.OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r


record_of = C.record_of
pack_streams = X.pack_streams


# ---- Table B-15 ----
def b15_pairs():
    return sorted(TW.b15_codes())


def every_code():
    """16 x 272, one I picture: every (run, level) of Table B-15 with both signs, an end of block directly behind the DC, escapes at
    both ends of the level range and of the run, and pairs the table has no code for"""
    todo = [(r, s * l, False) for r, l in b15_pairs() for s in (1, -1)]
    todo += [(0, 2047, False), (0, -2047, False), (63 - 1, 1, True), (0, 41, False), (1, -19, False), (32, 1, False), (5, 4, False), (0, 1, True)]
    blocks, cur, k = [], [], 1
    for run, lvl, esc in todo:
        if k + run >= 64:
            blocks.append(cur)
            cur, k = [], 1
        cur.append((run, lvl, esc))
        k += run + 1
    blocks.append(cur)
    blocks.append([])                                               # the end of block directly behind the DC
    while len(blocks) % 6:
        blocks.append([(len(blocks) % 5, 3, False)])
    mbs = [dict(kind="intra", blocks=[dict(dc=(7 * (n + b)) % 23 - 11, coefs=c) for b, c in enumerate(blocks[n:n + 6])]) for n in range(0, len(blocks), 6)]
    assert len(mbs) <= 17, len(mbs)
    rng = np.random.RandomState(52)
    while len(mbs) < 17:
        mbs.append(C.mb(rng, "intra"))
    return [dict(type=1, q=2, slices=[dict(q=1 + n % 3, mbs=[m]) for n, m in enumerate(mbs)])]


def mixed(seed=53):
    """48 x 32, I P B B: intra macroblocks in the P and the B pictures beside coded non-intra ones in the same slice, the second
    picture in the alternate scan, rows cut into slices"""
    rng = np.random.RandomState(seed)
    i0 = C.intra_picture(rng, 3, 2)
    p1 = dict(type=2, alt=1, slices=[dict(q=3, mbs=[C.mb(rng, "coded", 0, 0), C.mb(rng, "intra"), C.mb(rng, "coded", 2, 0)]),
                                     dict(q=5, mbs=[C.mb(rng, "intra"), C.mb(rng, "nomc", cbp=41), dict(C.mb(rng, "intra"), quant=7)])])
    b2 = BC.b_picture([[BC.pred((2, 1), (1, 1), rng, cbp=33), BC.intra_mb(rng), BC.pred((-3, 2), (-2, 1), rng, cbp=12, quant=7)],
                       [BC.intra_mb(rng, quant=4), BC.pred(None, (4, -2), rng, cbp=63), BC.pred((-1, -1), None)]])
    b3 = BC.b_picture([[BC.intra_mb(rng), BC.intra_mb(rng), BC.pred((-1, 0), None, rng, cbp=1)], [BC.pred((0, 0), (0, 0)), BC.intra_mb(rng), BC.intra_mb(rng)]], alt=1)
    return X.cycle_cuts([i0, p1, b2, b3], X.PATTERNS[1:] + X.PATTERNS[:1])


def field_pictures(seed=54):
    """48 x 64, progressive_sequence 0, I P B B with frame_pred_frame_dct 0: field DCT in intra macroblocks, the alternate scan"""
    rng = np.random.RandomState(seed)
    pics = IC.pictures(rng, "IPBB", 3, 4, most=5)
    pics[0]["alt"] = 1
    pics[2]["alt"] = 1
    return pics


def with_flags(pics, **kw):
    return [dict(p, **kw) for p in pics]


# ---- concealment vectors ----
def conceal_p():
    """48 x 32, I P with concealment vectors in both.  The P picture's row 0: an intra macroblock whose vector (4, -2) is the predictor of
    the vector behind it - read without it, that vector is another one and the frames differ; row 1: an intra macroblock behind a
    predicted one, its concealment vector equal to the predictor (a delta of 0), so that the vector behind it is read right only where
    the predictors are kept, not reset"""
    rng = np.random.RandomState(55)
    i0 = C.intra_picture(rng, 3, 2)
    for sl in i0["slices"]:
        for k, m in enumerate(sl["mbs"]):
            m["cmv"] = ((5, -3), (-7, 2), (0, 6))[k]
    p1 = dict(type=2, f_code=(2, 2), slices=[
        dict(q=3, mbs=[dict(C.mb(rng, "intra"), cmv=(4, -2)), dict(kind="not_coded", mv=(5, 1)), C.mb(rng, "coded", 2, 0)]),
        dict(q=4, mbs=[dict(kind="not_coded", mv=(3, -2)), dict(C.mb(rng, "intra"), cmv=(3, -2)), dict(kind="not_coded", mv=(-6, -3))])])
    return [dict(i0, f_code=(3, 2)), p1]


def conceal_b():
    """48 x 32, I P B: a B picture's intra macroblock with a concealment vector between macroblocks of both directions - the backward
    predictor is kept too"""
    rng = np.random.RandomState(56)
    b2 = BC.b_picture([[BC.pred((2, 1), (1, 1), rng, cbp=33), dict(BC.intra_mb(rng), cmv=(-2, 3)), BC.pred((-3, 2), (-2, 1))],
                       [dict(BC.intra_mb(rng), cmv=(1, 1)), BC.pred((2, -2), (4, -2)), BC.pred((-1, -1), None)]], f_code=(2, 2, 2, 2))
    return [C.intra_picture(rng, 3, 2), C.random_p(rng, 3, 2), b2]


def conceal_fields():
    """48 x 64 with frame_pred_frame_dct 0: an intra macroblock's concealment vector sets PMV[1][0] too - the bottom-field vector of
    the field-based macroblock behind it is predicted from it"""
    rng = np.random.RandomState(57)
    pics = IC.pictures(rng, "IP", 3, 4, most=5)
    blocks = lambda: [C.block(rng, True) for _ in range(6)]
    pics[1]["slices"][1]["mbs"] = [IC.fmb(0, (2, 1), 1, (1, 2)), dict(kind="intra", dct=1, cmv=(-5, 6), blocks=blocks()), IC.fmb(1, (-1, -2), 1, (-2, 2))]
    pics[1]["slices"][2]["mbs"] = [dict(kind="intra", cmv=(7, -4), blocks=blocks()), IC.fmb(1, (-3, 1), 0, (2, -1)), dict(kind="pred", fwd=(-1, 3))]
    return pics


def without_vectors(pics):
    return [dict(p, slices=[dict(sl, mbs=[{k: v for k, v in m.items() if k != "cmv"} for m in sl["mbs"]]) for sl in p["slices"]]) for p in pics]


# ---- dual prime: one description -> the stream and the log tests/mbt_ref.py reads (after arith_cases.build) ----
def build(w, h, pictures, seq=None):
    """pictures of rows of macroblocks dict(intra=bool, fwd, motion="frame" | "field" | "dual", dct, cbp, cmv, blocks=[(levels[64] in
    raster order, the intra DC)]) -> (stream, log): the writer's pictures and, for mbt_ref.frames, what they say"""
    seq = dict(seq or {})
    seq.setdefault("progressive", 0)
    mbw, rows = (w + 15) // 16, IW.mb_rows(h, seq["progressive"])
    mats = (tuple(AC.DEFAULT_INTRA), tuple(AC.DEFAULT_NON_INTRA))
    wpics, lpics = [], []
    for pic in pictures:
        ptype, prec, alt = pic["type"], pic.get("prec", 2), pic.get("alt", 0)
        assert len(pic["rows"]) == rows and all(len(r) == mbw for r in pic["rows"]) and ptype in (1, 2)
        slices, lmbs = [], []
        for row, mbs in enumerate(pic["rows"]):
            sl, pred = dict(q=pic.get("q", 2), mbs=[]), [0, 0, 0]
            for col, mb in enumerate(mbs):
                intra = bool(mb.get("intra"))
                fwd = None if intra else mb.get("fwd")
                cbp = 63 if intra else mb.get("cbp", 0)
                if not intra or col == 0:
                    pred = [1 << (7 + prec)] * 3
                blocks, lblocks, src = [], [], iter(mb.get("blocks", ()))
                for b in range(6):
                    if not (cbp >> (5 - b)) & 1:
                        continue
                    lv, dc = next(src)
                    lv = np.asarray(lv, np.int64)
                    comp, diff = (0 if b < 4 else b - 3), 0
                    if intra:
                        diff, pred[comp] = int(dc) - pred[comp], int(dc)
                    blocks.append(AC._writer_block(lv, diff, intra, alt))
                    lblocks.append((lv[list(AC.scan_of(alt))], diff))
                motion = mb.get("motion", "frame")
                m = dict(kind="intra" if intra else "pred" if fwd is not None else "nomc", blocks=blocks, motion=motion, dct=mb.get("dct", 0), fwd=fwd, bwd=None, cbp=cbp)
                if "cmv" in mb:
                    m["cmv"] = mb["cmv"]
                sl["mbs"].append(m)
                lmbs.append(dict(row=row, col=col, first=col == 0, intra=intra, fwd=fwd if (fwd is not None or intra) else (0, 0), bwd=None, nomc=not intra and fwd is None,
                                 motion=motion if fwd is not None else "frame", dct=mb.get("dct", 0) if (intra or cbp) else 0, cbp=cbp, qcode=pic.get("q", 2), blocks=lblocks))
            slices.append(sl)
        f_code = tuple(pic.get("f_code", (1, 1, 1, 1)))
        wpics.append(dict(type=ptype, prec=prec, alt=alt, field=True, slices=slices, f_code=f_code, tff=pic.get("tff", 1), ivf=pic.get("ivf", 0), cmv=pic.get("cmv", 0)))
        lpics.append(dict(type=ptype, prec=prec, qst=0, scan=list(AC.scan_of(alt)), matrices=mats, mbs=lmbs, tff=pic.get("tff", 1), f_code=f_code, field=True,
                          cmv=pic.get("cmv", 0)))
    s, L = TW.stream(w, h, wpics, seq=seq)
    return s, dict(w=w, h=h, mbw=mbw, rows=rows, pictures=lpics, writer=L)


def _textured(rng):
    """an intra macroblock with a few low coefficients in every block: a reference with content in both fields"""
    blocks = []
    for b in range(6):
        lv = np.zeros(64, np.int64)
        for k in (1, 8, 9, 2, 16):
            lv[k] = int(rng.randint(-9, 10))
        blocks.append((lv, int(rng.randint(60, 200))))
    return dict(intra=True, dct=int(rng.randint(2)), blocks=blocks)


def textured_i(seed, mbw=3, rows=4):
    rng = np.random.RandomState(seed)
    return dict(type=1, prec=0, q=3, rows=[[_textured(rng) for _ in range(mbw)] for _ in range(rows)])


def dp(v, dmv=(0, 0), **kw):
    return dict(fwd=(tuple(v), tuple(dmv)), motion="dual", **kw)


def fld(s0, v0, s1, v1, **kw):
    return dict(fwd=((s0, tuple(v0)), (s1, tuple(v1))), motion="field", **kw)


def residual(rng):
    lv = np.zeros(64, np.int64)
    for k in (0, 1, 8):
        lv[k] = int(rng.randint(-4, 5)) or 1
    return (lv, 0)


@functools.lru_cache(maxsize=None)
def dual_cases():
    """name -> (stream, log, the wrong forms of mbt_ref that must change its frames).  48 x 64, four macroblock rows; the vectors of
    rows 0 and 3 keep every read inside the field"""
    out = {}
    rng = np.random.RandomState(58)
    ref = textured_i(59)
    # vectors with odd and even, positive and negative components in both dimensions; every dmvector
    p = dict(type=2, q=2, rows=[[dp((3, 5), (1, 1)), dp((-3, 4), (0, 1), cbp=63, blocks=[residual(rng) for _ in range(6)]), dp((-1, 3), (-1, 0))],
                                [dp((5, -3), (1, -1)), dp((2, -1), (0, 0), cbp=33, dct=1, blocks=[residual(rng), residual(rng)]), dp((-1, 1), (-1, 1))],
                                [dp((5, 3), (-1, -1)), dp((-2, -3), (1, 0)), dp((0, 0), (0, 0))],
                                [dp((1, -5), (0, -1)), dp((-3, -7), (1, -1)), dp((-4, -4), (-1, 1))]])
    out["vectors"] = build(48, 64, [ref, p]) + (("half_floor", "half_up", "factors_swapped", "e_swapped", "e_none", "selects_swapped", "mean_trunc", "chroma_joint"),)
    out["bottom_field_first"] = build(48, 64, [ref, dict(p, tff=0)]) + (("tff_ignored", "factors_swapped"),)
    # PMV[1][0]: a field-based macroblock, a dual-prime one, a field-based one whose bottom-field vector is predicted from it; a skipped
    # macroblock cannot stand here (build writes every macroblock), a frame-based one shows that PMV[0][0] is the vector with its
    # vertical component doubled
    q = dict(type=2, q=2, rows=[[fld(0, (2, 1), 1, (1, 3)), dp((-3, 2), (1, 1)), fld(1, (-2, 3), 0, (-4, 1))],
                                [dp((2, -2), (0, -1)), dict(fwd=(3, -5)), fld(0, (-1, 1), 0, (-2, -2))],
                                [dict(fwd=(4, 2)), dp((4, 1), (-1, 0)), dict(fwd=(-5, 3))],
                                [fld(1, (0, -3), 1, (2, -2)), dp((-1, -2), (0, 0)), dp((-2, -3), (1, -1))]])
    out["predictors"] = build(48, 64, [ref, q]) + (("pmv1_kept",),)
    return out


FIELD_A, FIELD_B = 60, 201


def flat_fields():
    """a reference whose top-field lines are FIELD_A and bottom-field lines FIELD_B in luma (field DCT: blocks 0 / 1 the top lines,
    2 / 3 the bottom lines), chroma 128, and a P picture of dual-prime macroblocks without residual: every luma sample is the mean of
    one sample of each field - (FIELD_A + FIELD_B + 1) >> 1 = 131, a literal"""
    z = np.zeros(64, np.int64)
    mb = dict(intra=True, dct=1, blocks=[(z, FIELD_A), (z, FIELD_A), (z, FIELD_B), (z, FIELD_B), (z, 128), (z, 128)])
    ref = dict(type=1, prec=0, q=3, rows=[[dict(mb) for _ in range(3)] for _ in range(4)])
    p = dict(type=2, q=2, rows=[[dp((2, 1), (0, 1)), dp((-1, 0), (1, 1)), dp((0, 2), (-1, 0))],
                                [dp((3, -3), (1, -1)), dp((-2, 5), (0, 0)), dp((-1, 1), (0, 1))],
                                [dp((0, 0), (0, 0)), dp((-5, -2), (1, 1)), dp((-4, 3), (-1, -1))],
                                [dp((1, -1), (0, -1)), dp((0, -4), (0, 0)), dp((-3, -2), (1, 0))]])
    return build(48, 64, [ref, p])


def all_tools():
    """48 x 64, I P P: Table B-15, concealment vectors and dual prime together, field-based and frame-based macroblocks between them,
    several slices a row"""
    rng = np.random.RandomState(60)
    ref = textured_i(61)
    for r in ref["rows"]:
        for k, m in enumerate(r):
            m["cmv"] = (2 * k - 3, 5 - k)
    p1 = dict(type=2, q=3, ivf=1, cmv=1, rows=[
        [dp((3, 5), (1, 1)), dict(_textured(rng), cmv=(-3, 2)), dp((-2, 3), (0, 1), cbp=63, blocks=[residual(rng) for _ in range(6)])],
        [dict(_textured(rng), cmv=(6, -2)), fld(0, (5, -1), 1, (4, -2)), dp((-2, -2), (-1, 0))],
        [dict(fwd=(2, 2), cbp=5, blocks=[residual(rng), residual(rng)]), dict(), dict(_textured(rng), cmv=(0, 0))],
        [dp((1, -3), (0, 0)), dict(fwd=(-3, -4)), dict(_textured(rng), cmv=(-8, 7))]])
    p1["rows"][2][1] = dict(cbp=16, blocks=[residual(rng)])          # no vector: the predictors reset
    p2 = dict(p1, tff=0, alt=1)
    return [dict(ref, ivf=1, cmv=1), p1, p2]


# ---- the valid cases: name -> (stream, log, b_pictures, interlaced) ----
@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    out["b15_every_code"] = TW.stream(16, 272, with_flags(every_code(), ivf=1)) + (False, False)
    out["b15_mixed"] = TW.stream(48, 32, with_flags(mixed(), ivf=1)) + (True, False)
    out["b15_fields"] = TW.stream(48, 64, with_flags(field_pictures(), ivf=1)) + (True, True)
    out["cmv_ip"] = TW.stream(48, 32, with_flags(conceal_p(), cmv=1)) + (False, False)
    out["cmv_b"] = TW.stream(48, 32, with_flags(conceal_b(), cmv=1)) + (True, False)
    out["cmv_fields"] = TW.stream(48, 64, with_flags(conceal_fields(), cmv=1, f_code=(2, 2, 1, 1))) + (False, True)
    out["cmv_b15"] = TW.stream(48, 32, with_flags(conceal_p(), cmv=1, ivf=1)) + (False, False)
    for name, (s, log, wrong) in dual_cases().items():
        out["dual_" + name] = (s, log["writer"], False, True)
    s, log = flat_fields()
    out["dual_flat"] = (s, log["writer"], False, True)
    s, log = build(48, 64, all_tools())
    out["all_tools"] = (s, log["writer"], False, True)
    return out


def settings(b, i):
    """every setting of "decode_b_pictures" / "decode_interlaced" that accepts a stream which needs (b, i)"""
    return [(bb, ii) for bb in (False, True) for ii in (False, True) if bb >= b and ii >= i]


# ---- known answers: name -> (stream, b, i, [expected (Y, U, V) per output frame]) ----
def _off(stream, b, i, extended=True):
    """the frames of the definition with the option off: the existing decoder's answer"""
    d, at = spec(stream, b, i, mb_tools=False, extended=extended)
    assert d is not None, at
    return d.frames


@functools.lru_cache(maxsize=None)
def known():
    out = {}
    c = cases()
    for name, w, h, pics, ext in (("b15_every_code", 16, 272, every_code(), False), ("b15_mixed", 48, 32, mixed(), True), ("b15_fields", 48, 64, field_pictures(), False)):
        s, L, b, i = c[name]
        twin = TW.stream(w, h, with_flags(pics, ivf=0))[0]
        assert twin != s
        out[name] = (s, b, i, _off(twin, b, i, ext))
    for name, w, h, pics in (("cmv_ip", 48, 32, conceal_p()), ("cmv_b", 48, 32, conceal_b()), ("cmv_fields", 48, 64, conceal_fields())):
        s, L, b, i = c[name]
        kw = dict(f_code=(2, 2, 1, 1)) if name == "cmv_fields" else {}
        twin = TW.stream(w, h, with_flags(without_vectors(pics), cmv=0, **kw))[0]
        assert twin != s
        out[name] = (s, b, i, _off(twin, b, i, False))
    out["cmv_b15"] = (c["cmv_b15"][0], False, False, out["cmv_ip"][3])
    for name, (s, log, wrong) in dual_cases().items():
        out["dual_" + name] = (s, False, True, TR.frames(log))
    s, log = flat_fields()
    mean = (FIELD_A + FIELD_B + 1) >> 1
    assert mean == 131
    rows = np.where(np.arange(64)[:, None] % 2 == 0, FIELD_A, FIELD_B) * np.ones((1, 48), np.int64)
    grey = np.full((32, 24), 128, np.uint8)
    out["dual_flat"] = (s, False, True, [(rows.astype(np.uint8), grey, grey), (np.full((64, 48), 131, np.uint8), grey, grey)])
    return out


# ---- the refusals: name -> (stream, b, i, mb_tools, the offset of the unit the definition must name) ----
@functools.lru_cache(maxsize=None)
def refusals():
    out = {}

    def of(pics, unit, nth, w=48, h=32, b=False, i=False, t=True, **kw):
        s, L = TW.stream(w, h, pics, **kw)
        return s, b, i, t, [a for k, a in L["units"] if k == unit][nth]

    def ip(seed=62):
        rng = np.random.RandomState(seed)
        return [C.intra_picture(rng, 3, 2), C.random_p(rng, 3, 2)]

    # with the option off each flag refuses the stream at the coding extension that carries it (the second picture's here)
    p = ip(); p[1]["ivf"] = 1
    out["off_intra_vlc_format"] = of(p, "picture_ext", 1, t=False)
    p = ip(); p[1]["cmv"] = 1
    out["off_concealment"] = of(p, "picture_ext", 1, t=False)
    p = ip(); p[0].update(ivf=1, cmv=1)
    out["off_both"] = of(p, "picture_ext", 0, t=False)
    s, log = flat_fields()                                          # dual prime with the option off: at the first slice that has it
    out["off_dual_prime"] = (s, False, True, False, [a for k, a in log["writer"]["units"] if k == "slice"][4])
    # the marker bit
    p = with_flags(conceal_p(), cmv=1); p[1]["slices"][1]["mbs"][1]["marker"] = 0
    out["marker_0"] = of(p, "slice", 3)
    # f_code 15 in an I picture with concealment vectors
    p = with_flags(conceal_p(), cmv=1); p[0]["ext_f_code"] = (15, 15, 15, 15)
    out["i_picture_f_code_15"] = of(p, "picture_ext", 0)
    p = with_flags(conceal_p(), cmv=1); p[0]["ext_f_code"] = (3, 15, 15, 15)
    out["i_picture_f_code_15_vertical"] = of(p, "picture_ext", 0)
    # dual prime where it is not legal
    rng = np.random.RandomState(63)
    pics = IC.pictures(rng, "IPB", 3, 4, most=5)
    pics[2]["slices"][1]["mbs"] = [dict(kind="pred", fwd=(1, 1), bwd=None), dict(kind="pred", motion="dual", fwd=((2, 2), (0, 0)), bwd=None), dict(kind="pred", fwd=None, bwd=(0, 0))]
    out["dual_in_b_picture"] = of(pics, "slice", 9, h=64, b=True, i=True)
    p = ip()
    p[1] = dict(type=2, force_modes=True, slices=[dict(q=3, mbs=[dict(kind="pred", fwd=(1, 1)), dict(kind="pred", motion="dual", fwd=((2, 6), (1, 1))), dict(kind="pred", fwd=(0, 0))]),
                                                  dict(q=3, mbs=[dict(kind="pred", fwd=(0, 0)) for _ in range(3)])])
    out["dual_with_frame_pred_frame_dct_1"] = of(p, "slice", 2)
    # a derived vector outside its field: vy = 0 and dmvector 0 in the top row make T read field line -1 / 2
    for name, row, v, dmv in (("top", 0, (0, 0), (0, 0)), ("bottom", 3, (0, 0), (0, 0)), ("left", 1, (0, 2), (-1, 0)), ("right", 2, (0, 2), (1, 0))):
        ref = textured_i(64)
        rows = [[dp((0, 2), (0, 1)) for _ in range(3)], [dp((0, 0), (0, 0)) for _ in range(3)], [dp((0, 0), (0, 0)) for _ in range(3)], [dp((0, -2), (0, -1)) for _ in range(3)]]
        rows[row][0 if name != "right" else 2] = dp(v, dmv)
        s, log = build(48, 64, [ref, dict(type=2, q=2, rows=rows)])
        out["derived_outside_" + name] = (s, False, True, True, [a for k, a in log["writer"]["units"] if k == "slice"][4 + row])
    # a B-14 codeword of one of the ten pairs whose code moved, inside a B-15 block
    b14 = {pair: format(code, "0%db" % length) for pair, (code, length) in TW.W._tabs()["ac"].items()}
    for pair in TW.B15_MOVED:
        blocks = [dict(dc=3, coefs=[(1, 2, False), (pair[0], pair[1], False)], codes={pair: b14[pair]})] + [dict(dc=0, coefs=[]) for _ in range(5)]
        pic = dict(type=1, ivf=1, slices=[dict(q=4, mbs=[dict(kind="intra", blocks=[dict(dc=0, coefs=[(0, 2, False)]) for _ in range(6)]) for _ in range(3)]),
                                          dict(q=4, mbs=[dict(kind="intra", blocks=blocks)] + [dict(kind="intra", blocks=[dict(dc=0, coefs=[]) for _ in range(6)]) for _ in range(2)])])
        out["b14_code_of_%d_%d" % pair] = of([pic], "slice", 1)
    # the reserved motion type
    pics = IC.pictures(np.random.RandomState(65), "IP", 3, 4, most=5)
    pics[1]["slices"][2]["mbs"] = [dict(kind="pred", motion="frame", motion_bits=0, fwd=(1, 1)), dict(kind="pred", fwd=(0, 0)), dict(kind="pred", fwd=(0, 0))]
    out["motion_type_0"] = of(pics, "slice", 6, h=64, i=True)
    return out


# ---- the streams of the extended option: verdicts and bytes as with the option off ----
NEWLY_LEGAL = {"older_main_concealment_vectors", "older_main_intra_vlc_format_1"}      # their flag is legal now: refused at the slice it garbles


@functools.lru_cache(maxsize=None)
def extended_streams():
    """every stream of ext_cases: [(name, stream, b, i)]"""
    return [(n, s, b, i) for n, s, b, i in X.all_streams() if not n.startswith(("flip", "cut", "ins", "head", "quant"))]


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    s, log = build(48, 64, all_tools())
    return s, log["writer"]


@functools.lru_cache(maxsize=None)
def altered(n=300):
    """[(name, stream)]: seeded bit flips, cuts and insertions in the slice data of the stream with all three tools (decoded with
    "decode_b_pictures" off, "decode_interlaced" on)"""
    s, L = altered_base()
    rng = np.random.RandomState(7)
    slices = [a for k, a in L["units"] if k == "slice"]
    ends = {a: (L["units"][k + 1][1] if k + 1 < len(L["units"]) else len(s)) for k, (_, a) in enumerate(L["units"])}
    out = []
    for k in range(n):
        kind = k % 5
        at = slices[int(rng.randint(len(slices)))]
        if kind < 3:
            bit = int(rng.randint(8 * (at + 4), 8 * ends[at]))
            out.append(("flip%d" % bit, D.flip(s, bit)))
        elif kind == 3:
            cut = int(rng.randint(at + 5, ends[at] + 1))
            out.append(("cut%d" % cut, s[:cut]))
        else:
            ins = int(rng.randint(at + 4, ends[at]))
            out.append(("ins%d" % ins, s[:ins] + bytes([int(rng.randint(0, 256))]) + s[ins:]))
    return out


def all_streams():
    """every stream of this file that is decoded with the option on: (name, stream, b_pictures, interlaced)"""
    out = [(n, v[0], v[2], v[3]) for n, v in sorted(cases().items())]
    out += [("refusal_" + n, v[0], v[1], v[2]) for n, v in sorted(refusals().items()) if v[3]]
    return out + [(n, s, False, True) for n, s in altered()]
