"""Field pictures in the device decoder (option "decode_field_pictures" on top of "decode_interlaced", "decode_extended" and
"decode_mb_tools", "decode_b_pictures" either way): the streams it is tried on and what it must answer - shared by
tests/test_fld_cases.py (CPU) and tests/test_gpu_decode_fld.py.  The definition is the expectation:
decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=True, extended=True, mb_tools=True, field_pictures=True) -
its frames, or the offset its Refused names.  The known answers are frames the new code did not make:
   the twin       a stream of field pictures that uses only field-based vectors from the field of the same parity is two progressive
                  streams of half the height woven line by line: the definition WITH THE OPTION OFF decodes each of them
   fld_ref        tests/fld_ref.py computes the frames from what the writer was told to write; each of its wrong forms changes them
   a literal      an I + I pair of flat fields at two greys is a frame of alternating lines
Nothing here looks at what the device computes.

The streams are written by tests/fld_writer.py at the smallest shapes at which each rule can go wrong: 16 x 32 (one macroblock a
field), 48 x 64 (3 x 2 a field, the rows cut 3, 1 + 2 and 1 + 1 + 1), 48 x 48 (an odd count of 32-line rows, cropped), 80 x 32 (skipped
runs).

host_lib(): the fp_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_f_host.hpp compiled with g++."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import dec_cases as D
import fld_writer as FW
import ilace_cases as IC
import main_cases as C
import plan_cases as PC

M = D.M
Refused = M.decoder.Refused


def spec(stream, b_pictures, field_pictures=True):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures, interlaced=True, extended=True, mb_tools=True,
                                field_pictures=field_pictures), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, b_pictures, field_pictures=True):
    key = (stream, bool(b_pictures), bool(field_pictures))
    if key not in _specs:
        _specs[key] = spec(stream, b_pictures, field_pictures)
    return _specs[key]


_HARNESS = r"""
#include "dec_f_host.hpp"
extern "C" long long dec_f_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, int b_pictures, unsigned lanes, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_f_host::decode(es, n, layout, cap, b_pictures != 0, frames, lanes);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_f_host_")
        src, so = os.path.join(d, "dec_f_host.cpp"), os.path.join(d, "libdec_f_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_f_host_decode.restype = ctypes.c_longlong
        L.dec_f_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint,
                                        ctypes.POINTER(D.Stat)]
        _host = L
    return _host


def host_decode(stream, b_pictures, layout="i420", cap=None, lanes=256):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict); lanes: the ranges the plan cuts the events into"""
    stream = bytes(stream)
    room = (1 << 22) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = D.Stat()
    host_lib().dec_f_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, int(bool(b_pictures)), lanes, ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    if r["status"] != D.OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r


record_of = C.record_of


# ---- content: a field picture of random macroblocks whose every read lies inside a field that is there ----
def legal(rng, col, row, mbw, rows, half=None, most=5):
    for _ in range(40):
        v = (int(rng.randint(-most, most + 1)), int(rng.randint(-most, most + 1)))
        if FW.inside(col, row, v, mbw, rows, half):
            return v
    assert FW.inside(col, row, (0, 0), mbw, rows, half)
    return (0, 0)


def near(a):
    return (a + (a > 0)) >> 1


def dual_other(v, dmv, par):
    return (near(v[0]) + dmv[0], near(v[1]) + dmv[1] + (1 if par else -1))


def residual(rng, m, cbp):
    m["cbp"] = cbp
    m["blocks"] = [C.block(rng, False) for _ in range(bin(cbp).count("1"))]
    return m


def field(rng, ptype, ps, mbw, rows, avail=(0, 1), q=4, cuts=None, most=5, only=None, same_parity=False, **params):
    """one field picture.  avail: the parities a forward select may name (a B field has every field); cuts[row]: the columns at which
    row is cut into slices (no macroblock is skipped in such a row); only: the one kind of predicted macroblock to write;
    same_parity: every select names the field's own parity, every vector is field-based"""
    par = ps - 1
    slices = []
    for row in range(rows):
        mbs, col, front, pmv0 = [], 0, None, [(0, 0), (0, 0)]
        cut = bool(cuts and row < len(cuts) and cuts[row])
        while col < mbw:
            incr = 1
            if ptype != 1 and not cut and not same_parity and 0 < col < mbw - 1 and rng.randint(4) == 0:      # a skipped run in front of this macroblock
                run = int(rng.randint(1, mbw - 1 - col + 1))
                if ptype == 2 and par in avail:
                    incr, pmv0 = 1 + run, [(0, 0), (0, 0)]
                elif ptype == 3 and front is not None and all(FW.inside(col + k, row, pmv0[s], mbw, rows) for k in range(run) for s in (0, 1) if front[s]):
                    incr = 1 + run
            col += incr - 1
            kinds = ["intra"] if ptype == 1 else ["intra", "field", "field", "16x8", "16x8"] + (["dual", "dual", "nomc"] if ptype == 2 else [])
            if only and ptype != 1:
                kinds = [only]
            if same_parity and ptype != 1:
                kinds = ["field"]
            kind = kinds[int(rng.randint(len(kinds)))]
            if kind == "dual" and len(avail) < 2:
                kind = "field"
            if kind == "nomc" and par not in avail:
                kind = "field"
            sel = lambda: par if same_parity else avail[int(rng.randint(len(avail)))] if ptype == 2 else int(rng.randint(2))
            m = dict(kind="pred", incr=incr)
            if kind == "intra":
                m = C.mb(rng, "intra", incr=incr)
                front, pmv0 = None, [(0, 0), (0, 0)]
            elif kind == "nomc":
                m = residual(rng, dict(kind="nomc", incr=incr), int(rng.randint(1, 64)))
                front, pmv0 = (1, 0), [(0, 0), (0, 0)]
            else:
                dirs = (1, 0) if ptype == 2 else ((1, 0), (0, 1), (1, 1))[int(rng.randint(3))]
                m["motion"] = kind
                if kind == "dual":
                    for _ in range(60):
                        v, dmv = legal(rng, col, row, mbw, rows, most=most), (int(rng.randint(-1, 2)), int(rng.randint(-1, 2)))
                        if FW.inside(col, row, dual_other(v, dmv, par), mbw, rows):
                            break
                    else:
                        v, dmv = (0, 2 if par == 0 else -2), (0, 0)      # the other field by (0, 0): 1 + 0 - 1, or -1 + 0 + 1
                        assert FW.inside(col, row, v, mbw, rows) or rows == 1
                        if not FW.inside(col, row, v, mbw, rows):
                            m["motion"] = kind = "field"
                    if kind == "dual":
                        m["fwd"] = (v, dmv)
                        pmv0[0] = v
                if kind != "dual":
                    for s, name in ((0, "fwd"), (1, "bwd")):
                        if not dirs[s]:
                            continue
                        if kind == "field":
                            m[name] = (sel(), legal(rng, col, row, mbw, rows, most=most))
                            pmv0[s] = m[name][1]
                        else:
                            m[name] = tuple((sel(), legal(rng, col, row, mbw, rows, half=r, most=most)) for r in (0, 1))
                            pmv0[s] = m[name][0][1]
                if rng.randint(2):
                    residual(rng, m, int(rng.randint(1, 64)))
                front = dirs
            if rng.randint(5) == 0 and (m["kind"] == "intra" or m.get("cbp")):      # (a macroblock without blocks has no quantiser)
                m["quant"] = int(rng.randint(1, 32))
            mbs.append(m)
            col += 1
        slices.append(dict(q=q + row, mbs=mbs))
    out = dict(type=ptype, ps=ps, slices=slices, **params)
    if cuts:
        out["cuts"] = cuts
    return out


def pair(rng, letters, first_ps, mbw, rows, anchor=True, **kw):
    """two field pictures of one frame: letters "II", "IP", "PP" or "BB", the first of structure first_ps; anchor: whether an anchor
    frame stands in front (else a P second field finds only the first field of its own frame)"""
    t1, t2 = (" IPB".index(c) for c in letters)
    other = 3 - first_ps
    a = field(rng, t1, first_ps, mbw, rows, avail=(0, 1), **kw)
    b = field(rng, t2, other, mbw, rows, avail=(0, 1) if anchor or t2 == 3 else (first_ps - 1,), **kw)
    return [a, b]


CUTS = [[], [1], [1, 2]]                                            # the rows cut 3, 1 + 2, 1 + 1 + 1 - and again for the rows behind


def _cuts(rows):
    return [CUTS[r % 3] for r in range(rows)]


# ---- the valid cases: name -> (stream, log, b_pictures) ----
@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    rng = np.random.RandomState(71)
    # 16 x 32: one macroblock a field; either parity first; every kind of pair
    out["one_mb_top_first"] = FW.stream(16, 32, pair(rng, "IP", 1, 1, 1, anchor=False) + pair(rng, "PP", 1, 1, 1) + pair(rng, "BB", 1, 1, 1) + pair(rng, "II", 1, 1, 1)) + (True,)
    out["one_mb_bottom_first"] = FW.stream(16, 32, pair(rng, "II", 2, 1, 1) + pair(rng, "PP", 2, 1, 1) + pair(rng, "BB", 2, 1, 1) + pair(rng, "BB", 1, 1, 1)) + (True,)
    # 48 x 64: 3 x 2 a field, the rows cut
    pics = pair(rng, "IP", 1, 3, 2, anchor=False, cuts=_cuts(2)) + pair(rng, "PP", 2, 3, 2, cuts=_cuts(2)[::-1]) + pair(rng, "BB", 1, 3, 2, cuts=_cuts(2)) + \
        pair(rng, "BB", 2, 3, 2, cuts=[[1, 2], [1, 2]])
    out["cut_rows"] = FW.stream(48, 64, pics) + (True,)
    out["ip_only"] = FW.stream(48, 64, pair(rng, "II", 1, 3, 2) + pair(rng, "PP", 1, 3, 2) + pair(rng, "IP", 2, 3, 2) + pair(rng, "PP", 2, 3, 2), ) + (False,)
    # 48 x 48: an odd count of 32-line rows: two rows a field, the frame cropped
    out["cropped"] = FW.stream(48, 48, pair(rng, "IP", 2, 3, 2, anchor=False) + pair(rng, "PP", 1, 3, 2) + pair(rng, "BB", 2, 3, 2)) + (True,)
    # 80 x 32: skipped runs
    out["skipped_runs"] = FW.stream(80, 32, pair(rng, "II", 1, 5, 1) + pair(rng, "PP", 1, 5, 1) + pair(rng, "BB", 1, 5, 1) + pair(rng, "BB", 2, 5, 1) + pair(rng, "PP", 2, 5, 1)) + (True,)
    # skipped macroblocks of B fields behind a macroblock of both directions, of the forward one alone, of the backward one alone
    pm = lambda fwd, bwd, incr=1: dict(kind="pred", motion="field", fwd=fwd, bwd=bwd, incr=incr)
    b1 = dict(type=3, ps=1, slices=[dict(q=4, mbs=[pm((0, (2, 0)), (1, (4, 0))), pm((1, (-2, 0)), None, 2), residual(rng, pm(None, (0, (-3, 0)), 2), 44)])])
    b2 = dict(type=3, ps=2, slices=[dict(q=5, mbs=[pm(None, (1, (3, 0))), residual(rng, pm((0, (1, 0)), (0, (-1, 0)), 2), 7), pm((1, (-4, 0)), None, 2)])])
    out["skipped_b"] = FW.stream(80, 32, pair(rng, "IP", 2, 5, 1, anchor=False) + pair(rng, "PP", 1, 5, 1) + [b1, b2]) + (True,)
    # every motion type on its own
    for kind in ("field", "16x8", "dual"):
        pics = pair(rng, "II", 1, 3, 2) + pair(rng, "PP", 1, 3, 2, only=kind) + (pair(rng, "BB", 2, 3, 2, only=kind) if kind != "dual" else pair(rng, "PP", 2, 3, 2, only=kind))
        out["only_" + kind] = FW.stream(48, 64, pics) + (kind != "dual",)
    # frame pictures and field pairs in one stream
    frame = lambda c: IC.pictures(rng, c, 3, 4, most=5)[0]
    out["mixed"] = FW.stream(48, 64, [frame("I")] + pair(rng, "PP", 1, 3, 2) + [frame("B")] + pair(rng, "BB", 2, 3, 2) + [frame("P")] + pair(rng, "IP", 2, 3, 2) + [frame("B")]) + (True,)
    # concealment vectors, Table B-15, f_codes above 1, the alternate scan, the other scale
    kw = dict(cmv=1, ivf=1, f_code=(2, 2, 2, 2), alt=1, qst=1)
    pics = pair(rng, "IP", 1, 3, 2, anchor=False, most=9, **kw) + pair(rng, "PP", 2, 3, 2, most=9, **kw) + pair(rng, "BB", 1, 3, 2, most=9, **kw)
    for p in pics:
        for sl in p["slices"]:
            for m in sl["mbs"]:
                if m["kind"] == "intra":
                    m["cmv"] = (int(rng.randint(2)), (int(rng.randint(-20, 21)), int(rng.randint(-20, 21))))
    out["tools"] = FW.stream(48, 64, pics) + (True,)
    return out


def settings(b):
    """every setting of "decode_b_pictures" that accepts a stream which needs b"""
    return [bb for bb in (False, True) if bb >= b]


# ---- one description -> the stream and the log tests/fld_ref.py reads (after mbt_cases.build) ----
def build(w, h, pictures, seq=None):
    """pictures of field pictures dict(type=, ps=, q=, prec=, rows=[[macroblock, ...], ...]) with macroblocks
       dict(intra=True, blocks=[(levels[64] in raster order, the intra DC)] * 6)
       dict(skip=True)                                          a skipped macroblock (not the first or the last of its row)
       dict(motion="field" | "16x8" | "dual", fwd=, bwd=, cbp=, blocks=[(levels[64], 0), ...])      fld_writer's vectors, absolute
       dict(cbp=, blocks=)                                       a P field's macroblock without a vector
    -> (stream, log): the writer's pictures and, for fld_ref.frames, what they say"""
    import arith_cases as AC
    seq = dict(seq or {})
    seq.setdefault("progressive", 0)
    mbw, rows = (w + 15) // 16, (h + 31) // 32
    mats = (tuple(AC.DEFAULT_INTRA), tuple(AC.DEFAULT_NON_INTRA))
    wpics, lpics = [], []
    for pic in pictures:
        ptype, prec, alt = pic["type"], pic.get("prec", 2), pic.get("alt", 0)
        assert len(pic["rows"]) == rows and all(len(r) == mbw for r in pic["rows"])
        slices, lmbs = [], []
        for row, mbs in enumerate(pic["rows"]):
            sl, pred, incr = dict(q=pic.get("q", 2), mbs=[]), [0, 0, 0], 1
            for col, mb in enumerate(mbs):
                if mb.get("skip"):
                    assert 0 < col < mbw - 1 and ptype != 1
                    incr += 1
                    lmbs.append(dict(row=row, col=col, first=False, intra=False, skip=True, nomc=False, motion=None, fwd=None, bwd=None, cbp=0, qcode=pic.get("q", 2), blocks=[]))
                    continue
                intra = bool(mb.get("intra"))
                fwd, bwd = (None, None) if intra else (mb.get("fwd"), mb.get("bwd"))
                cbp = 63 if intra else mb.get("cbp", 0)
                if not intra or col == 0 or incr > 1:
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
                nomc = not intra and fwd is None and bwd is None
                assert not nomc or (ptype == 2 and cbp)
                m = dict(kind="intra" if intra else "nomc" if nomc else "pred", blocks=blocks, motion=mb.get("motion", "field"), fwd=fwd, bwd=bwd, cbp=cbp, incr=incr)
                sl["mbs"].append(m)
                lmbs.append(dict(row=row, col=col, first=col == 0 or incr > 1, intra=intra, skip=False, nomc=nomc, motion=None if intra or nomc else mb.get("motion", "field"),
                                 fwd=fwd, bwd=bwd, cbp=cbp, qcode=pic.get("q", 2), blocks=lblocks))
                incr = 1
            assert incr == 1
            slices.append(sl)
        f_code = tuple(pic.get("f_code", (1, 1, 1, 1)))
        wpics.append(dict(type=ptype, ps=pic["ps"], prec=prec, alt=alt, slices=slices, f_code=f_code))
        lpics.append(dict(type=ptype, ps=pic["ps"], prec=prec, qst=0, scan=list(AC.scan_of(alt)), matrices=mats, mbs=lmbs, f_code=f_code))
    s, L = FW.stream(w, h, wpics, seq=seq)
    return s, dict(w=w, h=h, mbw=mbw, rows=rows, pictures=lpics, writer=L)


FIELD_A, FIELD_B = 60, 201


def flat_pair(first_ps=1):
    """an I + I pair of 48 x 64: the top field flat at FIELD_A, the bottom field flat at FIELD_B, chroma 128"""
    z = np.zeros(64, np.int64)
    flat = lambda v: dict(intra=True, blocks=[(z, v)] * 4 + [(z, 128)] * 2)
    fld = lambda ps: dict(type=1, ps=ps, prec=0, q=3, rows=[[flat(FIELD_A if ps == 1 else FIELD_B) for _ in range(3)] for _ in range(2)])
    return build(48, 64, [fld(first_ps), fld(3 - first_ps)])


# ---- known answers: name -> (stream, b, [expected (Y, U, V) per output frame]) ----
def _as_frame_mb(m):
    """a field picture's macroblock (field-based vectors only) as the macroblock of a progressive frame picture"""
    if m["kind"] != "pred":
        return m
    out = {k: v for k, v in m.items() if k not in ("motion", "fwd", "bwd")}
    out.update(motion="frame", fwd=m["fwd"][1] if m.get("fwd") is not None else None, bwd=m["bwd"][1] if m.get("bwd") is not None else None)
    return out


@functools.lru_cache(maxsize=None)
def twin():
    """48 x 64, I P B B of field pairs, every vector field-based from the field of the same parity -> (the stream, the two progressive
    48 x 32 streams that carry the top fields and the bottom fields)"""
    import mbt_writer as TW
    rng = np.random.RandomState(72)
    pics = []
    for letters, first in (("II", 1), ("PP", 2), ("BB", 1), ("BB", 2)):
        pics += pair(rng, letters, first, 3, 2, same_parity=True)
    s, L = FW.stream(48, 64, pics)
    halves = []
    for ps in (1, 2):
        own = [dict(type=p["type"], slices=[dict(sl, mbs=[_as_frame_mb(m) for m in sl["mbs"]]) for sl in p["slices"]]) for p in pics if p["ps"] == ps]
        halves.append(TW.stream(48, 32, own, seq=dict(progressive=1))[0])
    return s, halves


@functools.lru_cache(maxsize=None)
def known():
    import fld_ref as FR
    out = {}
    s, halves = twin()
    parts = []
    for h in halves:                                                # the definition with every option of this series off, B pictures on
        parts.append(M.decoder.decode(h, quirks=False, syntax="main", b_pictures=True).frames)
    assert len(parts[0]) == len(parts[1]) == 4
    woven = []
    for top, bottom in zip(*parts):
        planes = []
        for a, c in zip(top, bottom):
            p = np.zeros((2 * a.shape[0], a.shape[1]), np.uint8)
            p[0::2], p[1::2] = a, c
            planes.append(p)
        woven.append(tuple(planes))
    out["twin"] = (s, True, woven)
    for name, (st, log, b, wrong) in ref_cases().items():
        out["ref_" + name] = (st, b, FR.frames(log))
    for first in (1, 2):
        s, log = flat_pair(first)
        rows = np.where(np.arange(64)[:, None] % 2 == 0, FIELD_A, FIELD_B) * np.ones((1, 48), np.int64)
        grey = np.full((32, 24), 128, np.uint8)
        out["literal_%s_first" % ("top" if first == 1 else "bottom")] = (s, False, [(rows.astype(np.uint8), grey, grey)])
    return out


def _textured(rng):
    blocks = []
    for b in range(6):
        lv = np.zeros(64, np.int64)
        for k in (1, 8, 9, 2, 16):
            lv[k] = int(rng.randint(-9, 10))
        blocks.append((lv, int(rng.randint(60, 200))))
    return dict(intra=True, blocks=blocks)


def textured(seed, ps, mbw=3, rows=2):
    rng = np.random.RandomState(seed)
    return dict(type=1, ps=ps, prec=0, q=3, rows=[[_textured(rng) for _ in range(mbw)] for _ in range(rows)])


def _res(rng):
    lv = np.zeros(64, np.int64)
    for k in (0, 1, 8):
        lv[k] = int(rng.randint(-4, 5)) or 1
    return (lv, 0)


def fb(sel, v, **kw):
    return dict(motion="field", fwd=(sel, tuple(v)), **kw)


def f168(s0, v0, s1, v1, **kw):
    return dict(motion="16x8", fwd=((s0, tuple(v0)), (s1, tuple(v1))), **kw)


def dp(v, dmv=(0, 0), **kw):
    return dict(motion="dual", fwd=(tuple(v), tuple(dmv)), **kw)


@functools.lru_cache(maxsize=None)
def ref_cases():
    """name -> (stream, log, b, the wrong forms of fld_ref that must change its frames).  48 x 64: 3 x 2 macroblocks a field"""
    out = {}
    rng = np.random.RandomState(73)
    ii = [textured(74, 1), textured(75, 2)]
    # field-based and 16 x 8 vectors with either select, in a P pair whose second field reads the first field of its own frame
    p1 = dict(type=2, ps=1, q=2, rows=[[fb(0, (3, 2)), f168(1, (2, 1), 0, (-3, -2), cbp=63, blocks=[_res(rng) for _ in range(6)]), fb(1, (-1, 3))],
                                       [f168(0, (1, -3), 1, (4, -1)), fb(1, (-2, -3)), f168(1, (-3, -5), 1, (-1, -4))]])
    p2 = dict(type=2, ps=2, q=2, rows=[[fb(0, (2, 3)), f168(0, (4, 2), 1, (-2, 1)), fb(1, (-3, 1), cbp=33, blocks=[_res(rng), _res(rng)])],
                                       [f168(1, (3, -2), 0, (1, -5)), fb(0, (-1, -1)), fb(0, (-4, -3))]])
    out["selects"] = build(48, 64, ii + [p1, p2]) + (False, ("second_reads_previous", "select_inverted", "weave_swapped", "lower_uses_vector_0", "chroma_split_at_8",
                                                             "vector_1_from_pmv_0", "two_stage_mean"))
    out["bottom_first"] = build(48, 64, [textured(75, 2), textured(74, 1), dict(p2, ps=2), dict(p1, ps=1)]) + (False, ("bottom_first_as_top_first", "weave_swapped"))
    # the predictors: a 16 x 8 macroblock behind a field-based one (its second vector is written against PMV[1][s], which followed); a B
    # field's skipped macroblock takes the predictors as they stand - doubled, were they kept as a frame picture keeps field vectors
    q1 = dict(type=2, ps=1, q=2, rows=[[fb(0, (2, 2)), f168(1, (1, 1), 0, (3, 2)), fb(1, (-1, 1))], [fb(1, (1, -2)), f168(0, (2, -1), 0, (2, -3)), fb(0, (-2, -2))]])
    q2 = dict(q1, ps=2)
    bq = lambda ps: dict(type=3, ps=ps, q=2, rows=[[dict(motion="field", fwd=(0, (2, 2)), bwd=(1, (1, 3))), dict(skip=True), dict(motion="field", fwd=(1, (-2, 1)), bwd=None)],
                                                   [dict(motion="field", fwd=None, bwd=(ps - 1, (2, -3))), dict(skip=True), dict(motion="16x8", fwd=((0, (-1, -2)), (1, (-3, -1))), bwd=None)]])
    out["predictors"] = build(48, 64, ii + [q1, q2, bq(1), bq(2)]) + (True, ("pmv_1_not_copied", "vertical_halved"))
    # dual prime in both parities: odd and even, positive and negative components, every dmvector
    d1 = dict(type=2, ps=1, q=2, rows=[[dp((3, 5), (1, 1)), dp((-3, 4), (0, 1), cbp=63, blocks=[_res(rng) for _ in range(6)]), dp((-1, 3), (-1, 0))],
                                       [dp((5, -3), (1, -1)), dp((2, -1), (0, 0)), dp((-1, -5), (-1, 1))]])
    d2 = dict(type=2, ps=2, q=2, rows=[[dp((1, 3), (0, 1)), dp((-5, 7), (1, 0)), dp((-3, 1), (-1, 1))],
                                       [dp((3, -5), (-1, -1)), dp((-2, -3), (1, -1), cbp=5, blocks=[_res(rng), _res(rng)]), dp((-1, -7), (0, -1))]])
    out["dual"] = build(48, 64, ii + [d1, d2]) + (False, ("e_wrong_sign", "e_left_out", "h_floor", "second_reads_previous"))
    # skipped macroblocks: 80 x 32 (one macroblock row a field: every vertical component is 0), a P pair (the zero vector, the same parity) and a B pair (the directions and the predictors in front)
    i5 = [textured(76, 1, 5, 1), textured(77, 2, 5, 1)]
    sp1 = dict(type=2, ps=1, q=2, rows=[[fb(1, (2, 0)), dict(skip=True), fb(0, (-3, 0)), dict(skip=True), fb(1, (-1, 0))]])
    sp2 = dict(type=2, ps=2, q=2, rows=[[fb(0, (1, 0)), dict(skip=True), dict(skip=True), dict(cbp=48, blocks=[_res(rng), _res(rng)]), fb(1, (-2, 0))]])
    bb = lambda ps, a, c: dict(type=3, ps=ps, q=2, rows=[[dict(motion="field", fwd=(a, (3, 0)), bwd=(c, (4, 0))), dict(skip=True), dict(skip=True),
                                                         dict(motion="field", fwd=None, bwd=(a, (1, 0))), dict(motion="field", fwd=(c, (-1, 0)), bwd=None)]])
    out["skipped"] = build(80, 32, i5 + [sp1, sp2, bb(1, 1, 0), bb(2, 0, 1)]) + (True, ("skipped_p_opposite_parity", "skipped_b_zero_vector"))
    return out


# ---- the refusals: name -> (stream, b, the option, the offset of the unit the definition must name) ----
def refusal_base(seed=78, mbw=2, rows=1):
    """32 x 32, I + P, P + P, B + B: the stream every refusal breaks in one place"""
    rng = np.random.RandomState(seed)
    return pair(rng, "IP", 1, mbw, rows, anchor=False) + pair(rng, "PP", 2, mbw, rows) + pair(rng, "BB", 1, mbw, rows)


@functools.lru_cache(maxsize=None)
def refusals():
    out = {}

    def unit(L, kind, nth):
        return [a for k, a in L["units"] if k == kind][nth]

    base = refusal_base

    def of(pics, kind, nth, w=32, h=32, b=True, f=True, **kw):
        s, L = FW.stream(w, h, pics, **kw)
        return s, b, f, unit(L, kind, nth)

    # the coding extension: each rule at the extension that breaks it (the third picture's here)
    out["progressive_sequence_1"] = of(base(), "picture_ext", 0, seq=dict(progressive=1))
    for name, ext in (("progressive_frame_1", dict(progressive_frame=1)), ("frame_pred_frame_dct_1", dict(frame_pred_frame_dct=1)), ("top_field_first_1", dict(top_field_first=1)),
                      ("repeat_first_field_1", dict(repeat_first_field=1)), ("picture_structure_0", dict(picture_structure=0))):
        p = base()
        p[2]["ext"] = ext
        out[name] = of(p, "picture_ext", 2)
    # the pairs: a partner that is not one, at its picture header
    p = base(); p[3]["ps"] = p[2]["ps"]
    out["same_parity"] = of(p, "picture", 3)
    p = base(); p[3] = IC.pictures(np.random.RandomState(79), "P", 2, 2, most=3)[0]
    out["frame_picture_behind_a_first_field"] = of(p, "picture", 3)
    p = base(); p[3] = field(np.random.RandomState(80), 1, 3 - p[2]["ps"], 2, 1)
    out["i_behind_p"] = of(p, "picture", 3)
    p = base(); p[5] = field(np.random.RandomState(81), 2, 3 - p[4]["ps"], 2, 1)
    out["p_behind_b"] = of(p, "picture", 5)
    p = base(); p[3]["tref"] = 5
    out["other_temporal_reference"] = of(p, "picture", 3)
    p = base()
    out["first_field_alone"] = of(p[:5], "picture", 4)
    out["first_field_alone_no_end"] = of(p[:3], "picture", 2, end=False)
    p = base(); del p[2:4]
    out["b_pair_behind_one_anchor_frame"] = of(p, "picture", 2)
    # a header between the two fields, at that unit
    p = base(); p[3]["gop"] = True
    out["gop_between_the_fields"] = of(p, "gop", 1)
    p = base(); p[3]["seq"] = True
    out["sequence_header_between_the_fields"] = of(p, "sequence", 1)
    p = base(); p[3]["between"] = [("end", b"\x00\x00\x01\xb7")]
    out["end_code_between_the_fields"] = of(p, "end", 0)
    # the macroblock layer, at the slice
    p = base(); p[2]["slices"][0]["mbs"] = [dict(kind="pred", motion="field", motion_bits=0, fwd=(0, (0, 0))), dict(kind="pred", motion="field", fwd=(0, (0, 0)))]
    out["field_motion_type_0"] = of(p, "slice", 2)
    p = base(); p[4]["slices"][0]["mbs"] = [dict(kind="pred", motion="dual", fwd=((0, 2), (0, 0)), bwd=None), dict(kind="pred", motion="field", fwd=(0, (0, 0)), bwd=None)]
    out["dual_prime_in_a_b_field"] = of(p, "slice", 4)
    p = base(); p[2]["slices"][0]["mbs"] = [dict(kind="pred", motion="field", fwd=(0, (0, -1))), dict(kind="pred", motion="field", fwd=(1, (0, 0)))]
    out["vector_above_its_field"] = of(p, "slice", 2)
    p = base(); p[3]["slices"][0]["mbs"] = [dict(kind="pred", motion="16x8", fwd=((0, (0, 0)), (1, (0, 1)))), dict(kind="pred", motion="field", fwd=(1, (0, 0)))]
    out["lower_half_below_its_field"] = of(p, "slice", 3)
    p = base(); p[1]["slices"][0]["mbs"] = [dict(kind="pred", motion="field", fwd=(0, (0, 0))), dict(kind="pred", motion="field", fwd=(1, (0, 0)))]
    out["select_without_a_field"] = of(p, "slice", 1)                # the bottom field of the stream's first frame: no bottom field in front
    p = base(); p[1]["slices"][0]["mbs"] = [dict(kind="pred", motion="field", fwd=(0, (0, 0))), dict(kind="nomc", cbp=32, blocks=[C.block(np.random.RandomState(82), False)])]
    out["no_vector_without_a_field"] = of(p, "slice", 1)             # the zero vector reads the field of its own parity
    rng = np.random.RandomState(83)
    p = pair(rng, "II", 1, 3, 2) + pair(rng, "PP", 1, 3, 2)
    p[2]["slices"].append(dict(p[2]["slices"][1], code=3))
    out["slice_code_beyond_the_rows"] = of(p, "slice", 6, w=48, h=64)
    p = [dict(q, cmv=1) for q in base()]
    p[0]["slices"][0]["mbs"][1]["marker"] = 0
    out["marker_bit_0"] = of(p, "slice", 0)
    # the parent's refusal with the option off: at the first field's coding extension
    out["option_off"] = of(base(), "picture_ext", 0, f=False)
    p = [IC.pictures(np.random.RandomState(84), "I", 2, 2, most=3)[0]] + base()[2:4]
    out["option_off_behind_a_frame_picture"] = of(p, "picture_ext", 1, f=False)
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    rng = np.random.RandomState(85)
    return FW.stream(32, 32, pair(rng, "IP", 1, 2, 1, anchor=False) + pair(rng, "PP", 2, 2, 1) + pair(rng, "BB", 1, 2, 1) + pair(rng, "BB", 2, 2, 1))


ALTERED_SEED = 8


@functools.lru_cache(maxsize=None)
def altered(n=300):
    """[(name, stream)]: seeded bit flips, cuts and insertions in the units of an I P B B stream of field pairs - picture headers and
    coding extensions among them, so that the pairs' rules are met too (decoded with "decode_b_pictures" on)"""
    s, L = altered_base()
    rng = np.random.RandomState(ALTERED_SEED)
    units = [a for k, a in L["units"] if k in ("slice", "slice", "picture", "picture_ext")]
    ends = {a: (L["units"][k + 1][1] if k + 1 < len(L["units"]) else len(s)) for k, (_, a) in enumerate(L["units"])}
    out = []
    for k in range(n):
        kind = k % 5
        at = units[int(rng.randint(len(units)))]
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


# ---- plan streams: longer than 256 events, a range's edge at every position of a pair ----
def _plan_pictures(frames, seed, frame_pictures=True):
    """I P B B P B B ... of 16 x 32: field pairs of either order, every fifth frame a frame picture (two slices); a GOP header at every
    I frame, a repeated sequence header at every second one"""
    rng = np.random.RandomState(seed)
    pics, letters = [], PC.ipbb_letters(frames)
    for f, c in enumerate(letters):
        first = 1 + (f // 3) % 2
        if frame_pictures and f % 5 == 4:
            new = [IC.pictures(rng, c, 1, 2, most=1)[0]]
        else:
            new = pair(rng, "IP" if c == "I" and f % 2 else c + c, first, 1, 1, anchor=f > 0)
        if c == "I" and f:
            new[0]["gop"] = True
            new[0]["seq"] = (f // 12) % 2 == 0
        pics += new
    return pics


@functools.lru_cache(maxsize=None)
def plan_streams():
    """name -> (stream, log, b).  shift_k: about 330 events in ranges of two, k user_data units behind the sequence's extensions move
    every edge through a pair - between its fields, between a field's header and its extension, between a frame picture's slices;
    long: more than 256 frames, ranges of seven events"""
    out = {}
    for k in range(7):
        s, L = FW.stream(16, 32, _plan_pictures(60, 86), seq=dict(extras_behind=PC.users(k, 3)))
        assert 256 < len(M.decoder.start_codes(s)) <= 512
        out["shift_%d" % k] = (s, L, True)
    s, L = FW.stream(16, 32, _plan_pictures(262, 87, frame_pictures=False))
    assert len(L["fields"]) == 524 and len(M.decoder.start_codes(s)) > 6 * 256
    out["long"] = (s, L, True)
    return out


@functools.lru_cache(maxsize=None)
def batch_edges():
    """32 x 32: I + P and P + P pairs in turn, then B pairs and anchors again - with "decode_batch" 1, 2 and 3 every chunk's edge has
    each kind of pair on either side of it"""
    rng = np.random.RandomState(88)
    pics = []
    for n, letters in enumerate(("IP", "PP", "PP", "IP", "PP", "IP", "BB", "BB", "PP", "IP", "PP", "BB")):
        pics += pair(rng, letters, 1 + n % 2, 2, 1, anchor=n > 0)
    return FW.stream(32, 32, pics) + (True,)


def all_streams():
    """every stream of this file that is decoded with the option on: (name, stream, b_pictures)"""
    out = [(n, v[0], v[2]) for n, v in sorted(cases().items())]
    out += [("refusal_" + n, v[0], v[1]) for n, v in sorted(refusals().items()) if v[2]]
    out += [("known_" + n, v[0], v[1]) for n, v in sorted(known().items())]
    out += [("plan_" + n, v[0], v[2]) for n, v in sorted(plan_streams().items())]
    out.append(("batch_edges", batch_edges()[0], True))
    return out + [(n, s, True) for n, s in altered()]
