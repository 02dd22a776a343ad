"""Damaged slices in the device decoder (option "decode_conceal" on top of "decode_interlaced", "decode_extended", "decode_mb_tools" and
"decode_field_pictures", "decode_b_pictures" either way, "decode_join" 0 .. 3): the streams it is tried on and what it must answer -
shared by tests/test_conceal_cases.py (CPU) and tests/test_gpu_decode_conceal.py.  The definition is the expectation:
decoder.decode(stream, quirks=False, syntax="main", ..., field_pictures=True, join=..., conceal=True) - its frames, record and report.
The known answers come from places the new code did not make:
   the twin       the damaged stream decodes to what the definition WITH THE OPTION OFF makes of a twin the writer wrote with the concealed
                  rows as forward, zero-vector, not-coded macroblocks (a field: field-based from its own parity) - the pictures behind it
                  included, so what a concealed picture hands on is held too
   the splice     a stream of I pictures alone against numpy: row r of frame n from the already spliced frame n - 1
   literals       every report is stated from how the damage was made: the rows, the slices, the picture's start code
Nothing here looks at what the device computes.

The streams are written by tests/fld_writer.py at 16 x 32 (a frame picture has two rows, a field one), 48 x 64 (3 x 4, 3 x 2 a field, the
rows cut 3, 1 + 2, 1 + 1 + 1), 48 x 48 (cropped) and 80 x 32 (skipped runs), three to eight coded pictures each; the damage is done to
the bytes, unit by unit.

host_lib(): the c_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_c_host.hpp compiled with g++."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import ext_cases as EC
import fld_cases as F
import join_cases as J

M, D, FW, IC, PC = F.M, F.D, F.FW, F.IC, F.PC
Refused = M.decoder.Refused
REPORT_FIELDS = ("first_offset", "bad_slices", "concealed_rows", "grey_rows", "damaged_pictures")


def spec(stream, b_pictures, join=0, conceal=True):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures, interlaced=True, extended=True, mb_tools=True, field_pictures=True,
                                join=join, conceal=conceal), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, b_pictures, join=0, conceal=True):
    key = (bytes(stream), bool(b_pictures), int(join), bool(conceal))
    if key not in _specs:
        _specs[key] = spec(*key)
    return _specs[key]


def report_of(d, stream):
    """the report the definition fixes: of a decoded stream, or of an option-off call"""
    return tuple(int(d.conceal[k]) for k in REPORT_FIELDS) if hasattr(d, "conceal") else (len(stream), 0, 0, 0, 0)


def no_report(stream):
    return (len(stream), 0, 0, 0, 0)


class Conceal(ctypes.Structure):
    _fields_ = [("first_offset", ctypes.c_uint64), ("bad_slices", ctypes.c_uint32), ("concealed_rows", ctypes.c_uint32), ("grey_rows", ctypes.c_uint32),
                ("damaged_pictures", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


_HARNESS = r"""
#include "dec_c_host.hpp"
extern "C" long long dec_c_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, int b_pictures, int join, unsigned lanes,
                                       dec_host::Record *rec, dec_c_host::Join *jr, dec_c_host::Conceal *cr)
{
    std::vector<uint8_t> frames;
    *rec = dec_c_host::decode(es, n, layout, cap, b_pictures != 0, join, frames, *jr, *cr, lanes);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_c_host_")
        src, so = os.path.join(d, "dec_c_host.cpp"), os.path.join(d, "libdec_c_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_c_host_decode.restype = ctypes.c_longlong
        L.dec_c_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                        ctypes.POINTER(D.Stat), ctypes.POINTER(J.Join), ctypes.POINTER(Conceal)]
        _host = L
    return _host


def host_decode(stream, b_pictures, join=0, layout="i420", lanes=256):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict, the join record, the report)"""
    stream = bytes(stream)
    room = 1 << 22
    out = np.zeros(room, np.uint8)
    rec, jr, cr = D.Stat(), J.Join(), Conceal()
    host_lib().dec_c_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, int(bool(b_pictures)), int(join), lanes, ctypes.byref(rec),
                                 ctypes.byref(jr), ctypes.byref(cr))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    j = tuple(int(getattr(jr, k)) for k in J.JOIN_FIELDS)
    c = tuple(int(getattr(cr, k)) for k in REPORT_FIELDS)
    if r["status"] != D.OK:
        return None, r, j, c
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r, j, c


record_of = F.record_of


# ---- the damage: done to the bytes, unit by unit ----
def units(stream):
    """[[code, bytes]] of every start code's unit (the stream begins with one)"""
    ev = M.decoder.start_codes(stream)
    assert ev and ev[0][0] == 0
    ends = [p for p, _ in ev[1:]] + [len(stream)]
    return [[c, stream[p:e]] for (p, c), e in zip(ev, ends)]


def pictures_of(u):
    """per coded picture: (the index of its picture header's unit, the indices of its slice units)"""
    out = []
    for i, (c, _) in enumerate(u):
        if c == 0x00:
            out.append((i, []))
        elif 1 <= c <= 0xAF and out:
            out[-1][1].append(i)
    return out


def picture_offset(stream, pic):
    u = units(stream)
    return sum(len(x[1]) for x in u[:pictures_of(u)[pic][0]])


def slice_offset(stream, pic, nth):
    u = units(stream)
    return sum(len(x[1]) for x in u[:pictures_of(u)[pic][1][nth]])


def _edit(stream, pic, fn):
    u = units(stream)
    sl = pictures_of(u)[pic][1]
    fn(u, sl)
    return b"".join(x[1] for x in u if x is not None)


def unreadable(stream, pic, nth):
    """the slice's payload overwritten with ones: quantiser_scale_code 31, intra_slice_flag 1, then extra_bit_slice 1 until the unit ends"""
    def fn(u, sl):
        c, b = u[sl[nth]]
        u[sl[nth]] = [c, b[:4] + b"\xff" * (len(b) - 4)]
    return _edit(stream, pic, fn)


def removed(stream, pic, nths):
    def fn(u, sl):
        for k in (range(len(sl)) if nths is None else nths):
            u[sl[k]] = None
    return _edit(stream, pic, fn)


def recoded(stream, pic, nth, code):
    def fn(u, sl):
        c, b = u[sl[nth]]
        u[sl[nth]] = [code, b[:3] + bytes([code]) + b[4:]]
    return _edit(stream, pic, fn)


def duplicated(stream, pic, nth):
    def fn(u, sl):
        c, b = u[sl[nth]]
        u[sl[nth]] = [c, b + b]
    return _edit(stream, pic, fn)


def exchanged(stream, pic, a, b):
    def fn(u, sl):
        u[sl[a]], u[sl[b]] = u[sl[b]], u[sl[a]]
    return _edit(stream, pic, fn)


def slice_codes(stream, pic):
    u = units(stream)
    return [u[i][0] for i in pictures_of(u)[pic][1]]


# ---- the bases: name -> (w, h, the writer's pictures, b_pictures) ----
def _frame(rng, letter, mbw, mbh, cuts=None):
    p = IC.pictures(rng, letter, mbw, mbh, most=1 if mbw == 1 else 3)[0]
    if cuts:
        p = dict(p, cuts=cuts)
    return p


def _still(ptype, ps, mbw, rows, q=5):
    """a P or B picture of zero vectors alone: it reads in any row (a slice whose code is changed to another row's)"""
    if ps == 3:
        mb = lambda: IC.frmb((0, 0)) if ptype == 2 else dict(IC.frmb((0, 0)), bwd=(0, 0))
        return dict(type=ptype, field=True, slices=[dict(q=q, mbs=[mb() for _ in range(mbw)]) for _ in range(rows)])
    mb = lambda: dict(kind="pred", motion="field", fwd=(ps - 1, (0, 0)), bwd=(ps - 1, (0, 0)) if ptype == 3 else None)
    return dict(type=ptype, ps=ps, slices=[dict(q=q, mbs=[mb() for _ in range(mbw)]) for _ in range(rows)])


@functools.lru_cache(maxsize=None)
def bases():
    out = {}
    rng = np.random.RandomState(2207)
    # 16 x 32: a frame picture has two slices, a field one
    out["f16"] = (16, 32, [_frame(rng, "I", 1, 2)] + F.pair(rng, "PP", 1, 1, 1, most=1) + [_frame(rng, "B", 1, 2)] + F.pair(rng, "BB", 2, 1, 1, most=1) + [_frame(rng, "P", 1, 2)], True)
    # 48 x 64: frame pictures of 3 x 4 and fields of 3 x 2, the rows cut 3, 1 + 2, 1 + 1 + 1
    out["c48"] = (48, 64, F.pair(rng, "IP", 1, 3, 2, anchor=False, cuts=F._cuts(2)) + [_frame(rng, "P", 3, 4, F._cuts(4))] + F.pair(rng, "BB", 2, 3, 2, cuts=F._cuts(2)[::-1] + [[1, 2]]) +
                  [_frame(rng, "B", 3, 4, [[1, 2]] * 4)] + F.pair(rng, "PP", 2, 3, 2, cuts=[[1, 2], [1, 2]]), True)
    # 48 x 48: an odd count of 32-line rows, cropped
    out["o48"] = (48, 48, [_frame(rng, "I", 3, 4)] + F.pair(rng, "PP", 2, 3, 2) + F.pair(rng, "BB", 1, 3, 2) + [_frame(rng, "P", 3, 4)], True)
    # 80 x 32: skipped runs; no B pictures
    out["s80"] = (80, 32, F.pair(rng, "II", 1, 5, 1) + F.pair(rng, "PP", 1, 5, 1) + [_frame(rng, "P", 5, 2)] + F.pair(rng, "IP", 2, 5, 1), False)
    # zero vectors alone behind an I frame: every slice reads in every row
    out["z48"] = (48, 64, [_frame(rng, "I", 3, 4)] + [_still(2, 3, 3, 4)] + [_still(3, 3, 3, 4)] + [_still(2, 1, 3, 2), _still(2, 2, 3, 2)] + [_still(3, 2, 3, 2), _still(3, 1, 3, 2)], True)
    # I pictures alone
    out["i48"] = (48, 64, [_frame(rng, "I", 3, 4)] + F.pair(rng, "II", 1, 3, 2) + [_frame(rng, "I", 3, 4, F._cuts(4))] + F.pair(rng, "II", 2, 3, 2) + [_frame(rng, "I", 3, 4)], False)
    # fields of every type with every row cut 1 + 1 + 1: an I pair in the first frame and one behind (its second field has a frame
    # in front), a P pair, a B pair
    rng3, cut3 = np.random.RandomState(2208), [[1, 2], [1, 2]]
    out["t48"] = (48, 64, F.pair(rng3, "II", 1, 3, 2, cuts=cut3) + F.pair(rng3, "PP", 2, 3, 2, cuts=cut3) + F.pair(rng3, "BB", 2, 3, 2, cuts=cut3) +
                  F.pair(rng3, "II", 2, 3, 2, cuts=cut3), True)
    return out


@functools.lru_cache(maxsize=None)
def base_stream(name):
    w, h, pics, b = bases()[name]
    s, L = FW.stream(w, h, list(pics))
    assert F.spec_cached(s, b)[0] is not None, name
    return s, L


def shape(name, pic):
    """(mbw, the rows of coded picture pic, its structure, its type)"""
    w, h, pics, b = bases()[name]
    ps = pics[pic].get("ps", 3)
    mbw, mbh = (w + 15) // 16, 2 * ((h + 31) // 32)
    return mbw, (mbh // 2 if ps != 3 else mbh), ps, pics[pic]["type"]


def twin(name, hidden, form=None):
    """the base with the rows hidden = {coded picture: rows} written as concealment macroblocks -> stream.  form: a wrong form -
    "bwd" (from the backward frame), "other_parity" (a field from the field of the other parity), "cols" = {(pic, row): columns}
    (only those columns of a row)"""
    w, h, pics, b = bases()[name]
    pics = list(pics)
    for pic, rows in hidden.items():
        mbw, nrows, ps, ptype = shape(name, pic)
        assert ptype != 1, "an I picture has no twin"
        p = dict(pics[pic])
        sls = list(p["slices"])
        cuts = [list(c) for c in p.get("cuts", [])] if p.get("cuts") else None
        for r in rows:
            if ps == 3:
                mb = IC.frmb((0, 0)) if form != "bwd" else IC.frmb((0, 0), "bwd")
            else:
                sel = ps - 1 if form != "other_parity" else 2 - ps
                mb = dict(kind="pred", motion="field", fwd=(sel, (0, 0)), bwd=None) if form != "bwd" else dict(kind="pred", motion="field", fwd=None, bwd=(sel, (0, 0)))
            if isinstance(form, dict) and (pic, r) in form:      # only some columns: the others stay what they were (a cut row without skipped macroblocks)
                mbs = [dict(mb) if c in form[(pic, r)] else dict(m, incr=1) for c, m in enumerate(sls[r]["mbs"])]
                assert len(mbs) == mbw
                sls[r] = dict(sls[r], mbs=mbs)
                continue
            sls[r] = dict(q=sls[r]["q"], mbs=[dict(mb) for _ in range(mbw)])
            if cuts and r < len(cuts):
                cuts[r] = []
        p["slices"] = sls
        if cuts is not None:
            p["cuts"] = cuts
        pics[pic] = p
    return FW.stream(w, h, pics)[0]


# ---- the cases: name -> dict(stream, b, base, pic, rows, bad, grey, twin) ----
def _case(base, pic, stream, rows, bad, **kw):
    w, h, pics, b = bases()[base]
    s0, L = base_stream(base)
    fields = L["fields"]
    grey = fields[pic]["frame"] == 0                            # the first anchor frame, both of its fields: no frame in front
    return dict(dict(stream=stream, b=b, base=base, pic=pic, rows=sorted(rows), bad=bad, grey=grey,
                     report=(picture_offset(stream, pic), bad, len(rows), len(rows) if grey else 0, 1)), **kw)


def rows_of(name, pic, nths):
    return sorted({slice_codes(base_stream(name)[0], pic)[k] - 1 for k in nths})


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for name in sorted(bases()):
        s, L = base_stream(name)
        for pic, f in enumerate(L["fields"]):
            codes = slice_codes(s, pic)
            mbw, nrows, ps, ptype = shape(name, pic)
            tag = "%s_%d%s%s" % (name, pic, " IPB"[ptype], {3: "f", 1: "t", 2: "b"}[ps])
            last = len(codes) - 1
            mid = len(codes) // 2
            out[tag + "_unreadable"] = _case(name, pic, unreadable(s, pic, mid), rows_of(name, pic, [mid]), 1)
            out[tag + "_removed"] = _case(name, pic, removed(s, pic, [0]), rows_of(name, pic, [0]), 0)
            out[tag + "_no_slices"] = _case(name, pic, removed(s, pic, None), range(nrows), 0)
            out[tag + "_code_af"] = _case(name, pic, recoded(s, pic, last, 0xAF), rows_of(name, pic, [last]), 1)
            out[tag + "_duplicated"] = _case(name, pic, duplicated(s, pic, mid), rows_of(name, pic, [mid]), 0)
            if nrows > 1:
                tail = [k for k, c in enumerate(codes) if c > nrows // 2]
                out[tag + "_last_rows"] = _case(name, pic, removed(s, pic, tail), range(nrows // 2, nrows), 0)
                if name in ("z48", "i48") or ptype == 1:        # the slice reads in any row: no vector, or the zero vector
                    other = codes[0] if codes[last] != codes[0] else codes[0] + 1
                    out[tag + "_code_other"] = _case(name, pic, recoded(s, pic, last, other), sorted({codes[last] - 1, other - 1}), 0)
            three = [c for c in set(codes) if codes.count(c) == 3]
            if three:
                k = codes.index(three[0])
                out[tag + "_one_of_three"] = _case(name, pic, unreadable(s, pic, k + 1), [three[0] - 1], 1, cut=(k, three[0] - 1))
                out[tag + "_exchanged"] = _case(name, pic, exchanged(s, pic, k, k + 2), [three[0] - 1], 0)
    for name, c in out.items():                                 # the twin: P and B pictures
        mbw, nrows, ps, ptype = shape(c["base"], c["pic"])
        c["twin"] = twin(c["base"], {c["pic"]: c["rows"]}) if ptype != 1 and not c["grey"] else None
    return out


def gpu_subset():
    """the cases the device is held to: every kind of damage, every base, every picture type and structure at least once"""
    names = sorted(cases())
    return [n for k, n in enumerate(names) if k % 3 == 0 or n.startswith("f16") or n.endswith(("_one_of_three", "_exchanged"))]


# ---- two damaged pictures in one stream, a damaged reference of a damaged picture, under the join ----
@functools.lru_cache(maxsize=None)
def chains():
    """name -> dict(stream, b, join, hidden = {pic: rows}, twin)"""
    out = {}
    s, L = base_stream("c48")
    # the P frame picture (coded 2) loses a row, the B field behind it (coded 3) the same row of its field, the last P field its own
    x = unreadable(unreadable(unreadable(s, 2, 0), 3, 0), 7, 0)
    hid = {2: rows_of("c48", 2, [0]), 3: rows_of("c48", 3, [0]), 7: rows_of("c48", 7, [0])}
    out["three_pictures"] = dict(stream=x, b=True, join=0, hidden=hid, twin=twin("c48", hid), report=(picture_offset(x, 2), 3, 3, 0, 3))
    s, L = base_stream("o48")
    x = removed(removed(s, 1, None), 2, None)                       # both P fields of a frame without a slice
    hid = {1: [0, 1], 2: [0, 1]}
    out["a_frame_of_nothing"] = dict(stream=x, b=True, join=0, hidden=hid, twin=twin("o48", hid), report=(picture_offset(x, 1), 0, 4, 0, 2))
    return out


# ---- I pictures alone: the splice ----
def splice(frames, hidden_by_frame):
    """frames (display order = coded order: no B pictures) with the lines of hidden_by_frame[n] = [(first luma line, first chroma line,
    step)] - 16 luma and 8 chroma lines each - taken from the already spliced frame n - 1 (grey where n = 0)"""
    out = []
    for n, f in enumerate(frames):
        g = [p.copy() for p in f]
        for y0, c0, step in hidden_by_frame.get(n, ()):
            for k, p in enumerate(g):
                first, count = (y0, 16) if k == 0 else (c0, 8)
                for y in range(first, first + count * step, step):
                    if y < p.shape[0]:
                        p[y] = out[n - 1][k][y] if n else 128
        out.append(tuple(g))
    return out


def lines_of(name, pic, rows):
    """the lines of the frame that the rows of coded picture pic cover: (first luma line, first chroma line, step) per row"""
    mbw, nrows, ps, ptype = shape(name, pic)
    if ps == 3:
        return [(16 * r, 8 * r, 1) for r in rows]
    return [(32 * r + (ps - 1), 16 * r + (ps - 1), 2) for r in rows]


# ---- plan streams: more than 256 events, slice-less and damaged pictures at every position of a range ----
@functools.lru_cache(maxsize=None)
def plan_streams():
    """name -> (stream, b, join).  two_k: F.plan_streams()'s shift_k (ranges of two events); three_k: about 600 events (ranges of three);
    long: more than 256 frames.  Every seventh coded picture loses all its slices, every fifth its first slice's payload"""
    def damage(s):
        n = len(pictures_of(units(s)))
        for pic in range(n - 1, 0, -1):
            if pic % 7 == 3:
                s = removed(s, pic, None)
            elif pic % 5 == 2:
                s = unreadable(s, pic, 0)
        return s
    out = {}
    for k in range(4):
        out["two_%d" % k] = (damage(F.plan_streams()["shift_%d" % k][0]), True, 0)
    for k in range(3):
        s, L = FW.stream(16, 32, F._plan_pictures(110, 91), seq=dict(extras_behind=PC.users(k, 5)))
        assert 512 < len(M.decoder.start_codes(s)) <= 768
        out["three_%d" % k] = (damage(s), True, 3 if k == 1 else 0)
    out["long"] = (damage(F.plan_streams()["long"][0]), True, 0)
    return out


def reached(stream):
    """the positions inside a range of events at which the plan meets a picture without a slice, and one whose slice is unreadable:
    from the start codes alone"""
    ev = M.decoder.start_codes(stream)
    per = -(-len(ev) // 256)
    none, first = set(), set()
    for i, (pos, code) in enumerate(ev):
        if code != 0x00:
            continue
        j = i + 2
        while j < len(ev) and ev[j][1] in (0xB2, 0xB5):
            j += 1
        if j >= len(ev) or not 1 <= ev[j][1] <= 0xAF:
            none.add(i % per)
        elif stream[ev[j][0] + 4:ev[j][0] + 6] == b"\xff\xff":
            first.add(j % per)
    return per, none, first


# ---- seeded single-bit flips confined to slice payloads ----
@functools.lru_cache(maxsize=None)
def flips(n=300, seed=1):
    s, L = F.altered_base()
    rng = np.random.RandomState(seed)
    sl = [a for k, a in L["units"] if k == "slice"]
    ends = {a: (L["units"][k + 1][1] if k + 1 < len(L["units"]) else len(s)) for k, (_, a) in enumerate(L["units"])}
    codes = M.decoder.start_codes(s)
    out = []
    while len(out) < n:
        at = sl[int(rng.randint(len(sl)))]
        bit = int(rng.randint(8 * (at + 4), 8 * ends[at]))
        x = D.flip(s, bit)
        if M.decoder.start_codes(x) == codes:
            out.append(("flip%d" % bit, x))
    return out


# ---- refusals that stay refusals: each header rule, the offsets stated from the writer's log ----
@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (stream, b, join, the offset of the unit refused) - the same with the option off, but for the last two (accepted there
    never: they are damaged as well)"""
    out = {}
    for name, v in sorted(F.refusals().items()):
        s, b, at = v[0], v[1], v[-1]
        d0, at0 = F.spec_cached(s, b)
        if d0 is not None or not v[2]:
            continue
        ev = M.decoder.start_codes(s)
        code = dict(ev).get(at0)
        if code is not None and not 1 <= code <= 0xAF:          # refused at a header, an extension, a picture: it stays one
            out["fld_" + name] = (s, b, 0, at0)
    for name, (s, b, join, want) in sorted(J.refusals().items()):
        if want is None:
            continue
        code = dict(M.decoder.start_codes(s)).get(want)
        if code is not None and not 1 <= code <= 0xAF:
            out["join_" + name] = (s, b, join, want)
    s, L = base_stream("c48")
    # a damaged stream whose later picture header is wrong: refused at that header, nothing concealed
    pic5 = picture_offset(s, 5)
    x = unreadable(s, 2, 0)
    x = x[:pic5 + 5] + bytes([x[pic5 + 5] & 0xC7]) + x[pic5 + 6:]  # picture_coding_type 0
    out["damaged_then_type_0"] = (x, True, 0, pic5)
    # the second B field (coded 4) without its coding extension: a frame picture for all the plan knows, no legal partner - at its header
    u = units(s)
    hdr = pictures_of(u)[4][0]
    y = b"".join(b for k, (c, b) in enumerate(u) if k != hdr + 1)
    out["no_coding_extension"] = (y, True, 0, sum(len(b) for c, b in u[:hdr]))
    # a second quant_matrix_extension in a kept picture, another picture of the stream damaged: refused at the second extension
    w, h, pics, b = bases()["f16"]
    pics = list(pics)
    pics[6] = dict(pics[6], extras=[EC.Q(intra=EC.A), EC.Q(non_intra=EC.A)])
    s, L = FW.stream(w, h, pics)
    out["second_quant_matrix_extension"] = (unreadable(s, 3, 0), True, 0, [a for k, a in L["units"] if k == "quant_matrix"][1])
    return out


# the header rules that stay refusals under the option -> a case of refusals() for each
RULES = {
    "a picture header that does not read": "damaged_then_type_0",
    "a sequence header that does not read": "join_marker_bit_of_the_header_at_j",
    "a repeated sequence header that says something else": "join_other_sequence_header",
    "a sequence header without its extension": "join_no_sequence_extension_at_j",
    "a coding extension: picture_structure 0": "fld_picture_structure_0",
    "a coding extension: progressive_frame 1 in a field": "fld_progressive_frame_1",
    "a picture header without a coding extension": "no_coding_extension",
    "the pairing: two fields of one parity": "fld_same_parity",
    "the pairing: a first field alone": "fld_first_field_alone",
    "the pairing: a GOP header between the fields": "fld_gop_between_the_fields",
    "P without an I frame": "join_p_in_front_of_the_first_i",
    "B without two anchor frames": "fld_b_pair_behind_one_anchor_frame",
    "a second quant_matrix_extension": "second_quant_matrix_extension",
    "the join window: its tail begins at a picture header": "join_tail_begins_at_a_picture_header",
    "the join window: a dropped B field's partner": "join_dropped_b_same_parity",
}


def all_streams():
    """every stream of this file with the settings it is decoded under: (name, stream, b_pictures, join)"""
    out = [(n, c["stream"], c["b"], 0) for n, c in sorted(cases().items())]
    out += [(n, c["stream"], c["b"], c["join"]) for n, c in sorted(chains().items())]
    out += [("plan_" + n, v[0], v[1], v[2]) for n, v in sorted(plan_streams().items()) if n != "long"]
    out += [("refusal_" + n, v[0], v[1], v[2]) for n, v in sorted(refusals().items())]
    return out + [(n, s, True, 0) for n, s in flips()[::3]]
