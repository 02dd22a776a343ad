"""Motion vectors at every f_code in the interlaced decode units (options "decode_interlaced", "decode_mb_tools", "decode_field_pictures"
and "decode_join" on the main syntax): the streams they are tried on and what they must answer - shared by tests/test_vec_cases.py (CPU)
and tests/test_gpu_decode_vectors.py.  The definition is the expectation: decoder.decode(stream, quirks=False, syntax="main", ...) with
the options a case names.  A second expectation that no decoder made: tests/vec_ref.py reads the motion codes the writer logged, follows
7.6.3 to the absolute vectors, and the references that take absolute vectors (arith_ref, mbt_ref, fld_ref) make the frames; a few
pictures are literals.  Nothing here looks at what the device computes.

Every stream comes from one description through the build() of arith_cases (frame pictures), mbt_cases (dual prime, concealment
vectors) or fld_cases (field pictures).  The vectors are chosen macroblock by macroblock by Fill.pick(): among the vectors that read inside
the picture - the ends of the legal interval, values around zero, the values that make the sum leave the f_code's range, a few random
ones - it takes the one that reaches most of what the stream has not reached yet: a wrap in either direction for every (mode, direction,
component, f_code), a residual that is not zero, a negative odd vertical frame vector in front of a field vector, a dmvector pair.  What
a stream really reaches is asserted from the writer's log by tests/test_vec_cases.py, not here.

The shapes are the smallest at which the rule can go wrong: a wrap at f_code n needs two vectors 16 << (n - 1) half samples apart, so
f_code 5 needs 160 samples, f_code 8 needs 1088, and no picture of at most 2048 samples can hold a wrap at f_code 9 (tests/test_main_cases.py);
the vertical f_codes take the same sizes turned on their side.

host_lib(): dec::il_field_vector, dec::bp_component, dec::t_dual_prime and dec::chroma_vector of csrc/m2v_decode_kernels.hpp compiled
with g++, fed through dec::Bits."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import arith_cases as AC
import dec_cases as D
import dec_writer as W
import fld_cases as FC
import fld_writer as FW
import ilace_cases as IC
import ilace_writer as IW
import main_cases as C
import mbt_cases as TC
import vec_ref as VR

M = D.M
Refused = M.decoder.Refused


# ---- the definition ----
def options(case):
    """the least capable option set that accepts the case: dict(b_pictures, interlaced, extended, mb_tools, field_pictures)"""
    need = case["needs"]
    return dict(b_pictures="b" in need, interlaced=True, extended=need in ("t", "tb", "f", "fb"), mb_tools=need in ("t", "tb", "f", "fb"), field_pictures=need in ("f", "fb"))


def ladder(case):
    """the least capable option set and every more capable one: [(name of the unit, options, join)]"""
    o = options(case)
    out = []
    if not o["extended"]:
        out.append(("dec_i", dict(o), 0))
        out.append(("dec_x", dict(o, extended=True), 0))
    if not o["field_pictures"]:
        out.append(("dec_x_tools", dict(o, extended=True, mb_tools=True), 0))
    full = dict(o, extended=True, mb_tools=True, field_pictures=True)
    out.append(("dec_f", full, 0))
    out.append(("dec_j", full, 3))
    if not o["b_pictures"]:
        out.append(("dec_f_b", dict(full, b_pictures=True), 0))
    return out


_specs = {}


def spec_cached(stream, o, join=0):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    key = (bytes(stream), tuple(sorted(o.items())), join)
    if key not in _specs:
        try:
            _specs[key] = (M.decoder.decode(bytes(stream), quirks=False, syntax="main", **dict(o, **(dict(join=join) if join else {}))), None)
        except Refused as e:
            _specs[key] = (None, e.offset)
    return _specs[key]


record_of = C.record_of


def host_decode(case):
    """the g++ build of the unit the case's options name -> (frames or None, record)"""
    o, s = options(case), case["stream"]
    if o["field_pictures"]:
        return FC.host_decode(s, o["b_pictures"], cap=1 << 24)
    if o["mb_tools"]:
        return TC.host_decode(s, o["b_pictures"], True, cap=1 << 24)
    return IC.host_decode(s, o["b_pictures"])


# ---- the g++ build of the functions ----
_HARNESS = r"""
#include <cstdint>
#include <cstring>
#include "m2v_decode_kernels.hpp"
using namespace m2v;
static dec::Bits bits_of(const uint8_t *d, uint64_t n) { dec::Bits b{}; b.d = d; b.pos = 0; b.end = 8 * n; b.err = 0; return b; }
// one component behind its predictor: -> ok | bits read << 8
extern "C" int vec_host_component(const uint8_t *d, uint64_t n, int r_size, int32_t *pmv)
{
    dec::Bits b = bits_of(d, n);
    const bool ok = dec::bp_component(b, *pmv, r_size);
    return (ok && !b.err ? 1 : 0) | (int)(b.pos << 8);
}
// a field vector of a frame picture behind its select: pmv[2] in and out, v[2] out
extern "C" int vec_host_field_vector(const uint8_t *d, uint64_t n, int r_h, int r_v, int32_t *pmv, int32_t *v)
{
    dec::Bits b = bits_of(d, n);
    int32_t p[2] = {pmv[0], pmv[1]};
    const bool ok = dec::il_field_vector(b, p, r_h, r_v, v[0], v[1]);
    pmv[0] = p[0]; pmv[1] = p[1];
    return (ok && !b.err ? 1 : 0) | (int)(b.pos << 8);
}
// out: mvx, mvy, mvx1, mvy1, bvx, bvy, bvx1, bvy1, sel[4]
extern "C" void vec_host_dual_prime(int vx, int vy, int d0, int d1, unsigned tff, int32_t *out)
{
    dec::IMb m{};
    dec::t_dual_prime(m, vx, vy, d0, d1, tff);
    const int32_t o[12] = {m.mvx, m.mvy, m.mvx1, m.mvy1, m.bvx, m.bvy, m.bvx1, m.bvy1, m.sel[0], m.sel[1], m.sel[2], m.sel[3]};
    memcpy(out, o, sizeof o);
}
// n of them: in[5 k ...] = vx, vy, d0, d1, tff; out[12 k ...]
extern "C" void vec_host_dual_prime_many(int n, const int32_t *in, int32_t *out)
{
    for (int k = 0; k < n; ++k) vec_host_dual_prime(in[5 * k], in[5 * k + 1], in[5 * k + 2], in[5 * k + 3], (unsigned)in[5 * k + 4], out + 12 * k);
}
extern "C" int vec_host_chroma(int v) { return dec::chroma_vector(v, dec::kIso); }
extern "C" int vec_host_half(int a) { return dec::t_half(a); }
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_vec_host_")
        src, so = os.path.join(d, "vec_host.cpp"), os.path.join(d, "libvec_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.vec_host_component.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
        L.vec_host_field_vector.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        L.vec_host_dual_prime.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(ctypes.c_int32)]
        L.vec_host_dual_prime_many.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _host = L
    return _host


def host_component(pmv, code, residual, f_code):
    """dec::bp_component on the bits of one component -> the predictor it leaves, which is the vector"""
    w, n = component_bits(code, residual, f_code)
    data = padded(w)
    p = ctypes.c_int32(pmv)
    r = host_lib().vec_host_component(data, len(data), f_code - 1, ctypes.byref(p))
    assert r & 1 and r >> 8 == n, "the component is accepted and as many bits are read as were written"
    return p.value


def host_field_vector(pmv, codes, f_codes):
    """dec::il_field_vector on the bits of both components: pmv (h, v), codes ((code, residual), (code, residual)), f_codes (h, v)
    -> ((vx, vy), the predictors left behind)"""
    w, n = D._Writer(), 0
    for (code, residual), f_code in zip(codes, f_codes):
        part, k = component_bits(code, residual, f_code)
        w.s += part.s
        n += k
    data = padded(w)
    p, v = (ctypes.c_int32 * 2)(*pmv), (ctypes.c_int32 * 2)()
    r = host_lib().vec_host_field_vector(data, len(data), f_codes[0] - 1, f_codes[1] - 1, p, v)
    assert r & 1 and r >> 8 == n
    return (v[0], v[1]), (p[0], p[1])


def host_dual_prime(rows):
    """dec::t_dual_prime on rows of (vx, vy, d0, d1, tff) -> [n, 12]: mvx, mvy, mvx1, mvy1, bvx, bvy, bvx1, bvy1, sel[4]"""
    a = np.ascontiguousarray(rows, np.int32)
    out = np.zeros((len(a), 12), np.int32)
    host_lib().vec_host_dual_prime_many(len(a), a.ctypes.data, out.ctypes.data)
    return out


def component_bits(code, residual, f_code):
    """motion_code (Table B-10 from dec_writer), its sign, motion_residual of f_code - 1 bits -> (bytes padded with ones, the bit count)"""
    w = D._Writer()
    w.code(W._tabs()["motion"][abs(code)])
    if code:
        w.put(code < 0, 1)
        if f_code > 1:
            w.put(residual, f_code - 1)
    n = len(w.s)
    return w, n


def padded(w):
    s = w.s + "1" * (-len(w.s) % 8 + 32)
    return bytes(int(s[k:k + 8], 2) for k in range(0, len(s), 8))


# ---- choosing vectors ----
def _frange(f_code, halved=False):
    f = 1 << (f_code - 1)
    return (-8 * f, 8 * f - 1) if halved else (-16 * f, 16 * f - 1)


def _ends(lo, hi, ok):
    """the legal interval inside [lo, hi]: ok is true on one interval"""
    p = next((c for c in (0, 4, -4, 8, -8, 16, -16) if lo <= c <= hi and ok(c)), None)
    if p is None:
        while lo <= hi and not ok(lo):
            lo += 1
        while hi >= lo and not ok(hi):
            hi -= 1
        return lo, hi
    a, b = lo, p
    while a < b:
        m = (a + b) // 2
        a, b = (a, m) if ok(m) else (m + 1, b)
    lo = a
    a, b = p, hi
    while a < b:
        m = (a + b + 1) // 2
        a, b = (m, b) if ok(m) else (a, m - 1)
    return lo, a


class Fill:
    """the chooser of one stream: what it has reached so far"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.have = set()

    def pick(self, mode, s, t, f_code, pred, halved, bound, ok, odd_negative=False, interval=True):
        """one component for (mode, direction s, component t): bound = (lo, hi) a first guess of the legal interval, ok(v) the test
        (interval: true on one interval)"""
        f = 1 << (f_code - 1)
        lo, hi = _frange(f_code, halved)
        lo, hi = max(lo, bound[0]), min(hi, bound[1])
        if interval:
            lo, hi = _ends(lo, hi, ok)
        assert lo <= hi, (mode, s, t, f_code, bound)
        cands = {lo + k for k in range(4)} | {hi - k for k in range(4)} | {0, 1, -1, 2, -2, 3, -3} | {pred, pred + 1, pred - 1}
        cands |= {pred + 16 * f + k for k in range(3)} | {pred - 16 * f - 1 - k for k in range(3)}
        cands |= {int(self.rng.randint(lo, hi + 1)) for _ in range(6)}
        best, best_score = None, None
        for v in sorted(cands):
            if not (lo <= v <= hi and ok(v)):
                continue
            delta = v - pred
            k = 1 if delta > 16 * f - 1 else -1 if delta < -16 * f else 0
            d = delta - 32 * f * k
            res = f > 1 and d != 0 and (abs(d) - 1) % f != 0
            score = 100 * ((mode, s, t, f_code, k) not in self.have) + 20 * (res and (mode, s, t, f_code, "res") not in self.have) + 10 * bool(res)
            if odd_negative and v < 0 and v & 1:
                score += 60
            for end, name in ((lo, "low"), (hi, "high")):          # a read that touches the picture's edge: the interval's end where the picture sets it
                if v == end and end != _frange(f_code, halved)[name == "high"] and (mode, s, t, f_code, name) not in self.have:
                    score += 40
            score += 8.0 * abs(v) / (16 * f) + self.rng.rand()
            if best is None or score > best_score:
                best, best_score = v, score
        assert best is not None, (mode, s, t, f_code, lo, hi)
        delta = best - pred
        k = 1 if delta > 16 * f - 1 else -1 if delta < -16 * f else 0
        d = delta - 32 * f * k
        self.have.add((mode, s, t, f_code, k))
        for end, name in ((lo, "low"), (hi, "high")):
            if best == end and end != _frange(f_code, halved)[name == "high"]:
                self.have.add((mode, s, t, f_code, name))
        if f > 1 and d != 0 and (abs(d) - 1) % f != 0:
            self.have.add((mode, s, t, f_code, "res"))
        return best


def _xbound(col, mbw):
    return (-32 * col - 2, 32 * (mbw - 1 - col) + 2)


def frame_picture(fill, ptype, mbw, mbh, f_code, kinds, res, tff=1, coded=7, dmvs=None):
    """the rows of a P or B frame picture with frame_pred_frame_dct 0: kinds(row, col) -> "frame" | "field" | "dual" | "intra" | "nomc";
    a B picture's directions go round; one macroblock in `coded` carries blocks made by res(rng)"""
    rng = fill.rng
    rows, n = [], 0
    for row in range(mbh):
        pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        mbs = []
        for col in range(mbw):
            kind = kinds(row, col)
            n += 1
            if kind == "intra":
                mbs.append(kind_intra(rng))
                pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                continue
            if kind == "nomc":
                mbs.append(dict(cbp=32, blocks=[res(rng)]))
                pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                continue
            dirs = (1, 0) if ptype == 2 else ((1, 0), (0, 1), (1, 1))[(row + col + n // 7) % 3]
            mb = dict(motion=kind, fwd=None, bwd=None)
            ybound_frame = (-32 * row - 2, 32 * (mbh - 1 - row) + 2)
            ybound_field = (-16 * row - 2, 16 * (mbh - 1 - row) + 2)
            next_field = col + 1 < mbw and kinds(row, col + 1) in ("field", "dual")
            for s in (0, 1):
                if not dirs[s]:
                    continue
                fh, fv = f_code[2 * s], f_code[2 * s + 1]
                if kind == "frame":
                    vx = fill.pick("frame", s, 0, fh, pmv[0][s][0], False, _xbound(col, mbw), lambda v: W.inside(col, row, (v, 0), mbw, mbh))
                    vy = fill.pick("frame", s, 1, fv, pmv[0][s][1], False, ybound_frame, lambda v: W.inside(col, row, (0, v), mbw, mbh), odd_negative=next_field)
                    pmv[0][s] = [vx, vy]
                    pmv[1][s] = [vx, vy]
                    mb["bwd" if s else "fwd"] = (vx, vy)
                elif kind == "field":
                    out = []
                    for r in (0, 1):
                        vx = fill.pick("field", s, 0, fh, pmv[r][s][0], False, _xbound(col, mbw), lambda v: IW.field_inside(col, row, (v, 0), mbw, mbh))
                        vy = fill.pick("field", s, 1, fv, pmv[r][s][1] >> 1, True, ybound_field, lambda v: IW.field_inside(col, row, (0, v), mbw, mbh))
                        pmv[r][s] = [vx, 2 * vy]
                        out.append((int(rng.randint(2)), (vx, vy)))
                    mb["bwd" if s else "fwd"] = tuple(out)
                else:                                               # dual prime: the vector and both derived vectors read inside their fields
                    dmv = dmvs.pop(0) if dmvs else (int(rng.randint(-1, 2)), int(rng.randint(-1, 2)))
                    inside = lambda v, t: all(IW.field_inside(col, row, (x, 0) if t == 0 else (0, x), mbw, mbh) for x in
                                              (v, VR.half(v) + dmv[t] - (t == 1), VR.half(3 * v) + dmv[t] + (t == 1), VR.half(v) + dmv[t] + (t == 1), VR.half(3 * v) + dmv[t] - (t == 1)))
                    vx = fill.pick("dual", 0, 0, fh, pmv[0][0][0], False, _xbound(col, mbw), lambda v: inside(v, 0))
                    vy = fill.pick("dual", 0, 1, fv, pmv[0][0][1] >> 1, True, ybound_field, lambda v: inside(v, 1))
                    pmv[0][0] = [vx, 2 * vy]
                    pmv[1][0] = [vx, 2 * vy]
                    mb["fwd"] = ((vx, vy), dmv)
            if n % coded == 0:
                mb.update(cbp=36, dct=int(rng.randint(2)), blocks=[res(rng), res(rng)])
            mbs.append(mb)
        rows.append(mbs)
    return dict(type=ptype, q=2, field=True, f_code=tuple(f_code), tff=tff, rows=rows)


def kind_intra(rng):
    return dict(AC.busy_i(rng, 1, 1, field=True)["rows"][0][0])


def _res_ac(rng):
    return AC.busy_block(rng, False, level=9)


def alternate(row, col):
    """frame-based and field-based macroblocks alternate along each row, either first"""
    return ("frame", "field")[(row + col) & 1]


def case(kind, needs, stream_log, **kw):
    s, log = stream_log
    return dict(dict(kind=kind, needs=needs, stream=s, log=log), **kw)


# ---- the frame-picture streams ----
@functools.lru_cache(maxsize=None)
def il_fcodes():
    """160 x 96, I P P P P P B B: horizontal f_codes 1 to 5 and vertical 1 to 4 wrap both ways; the B pictures' four f_codes differ"""
    fill = Fill(9001)
    pics = [AC.busy_i(fill.rng, 10, 6, field=True)]
    for fc in ((1, 1, 1, 1), (2, 2, 1, 1), (3, 3, 1, 1), (4, 4, 1, 1), (5, 1, 1, 1)):
        pics.append(frame_picture(fill, 2, 10, 6, fc, alternate, _res_ac))
    for fc in ((5, 4, 3, 2), (2, 3, 4, 1), (1, 2, 5, 4), (4, 1, 2, 3)):
        pics.append(frame_picture(fill, 3, 10, 6, fc, alternate, _res_ac))
    return case("frame", "b", AC.build(160, 96, pics))


@functools.lru_cache(maxsize=None)
def il_fcodes_wide():
    """1088 x 32, I P P P P B B: horizontal f_codes 6 to 8 wrap both ways in field-based vectors, forward and backward; f_code 9 has
    deltas of more than 2048 half samples and no wrap"""
    fill = Fill(9002)
    pics = [AC.busy_i(fill.rng, 68, 2, field=True)]
    for fc in ((6, 1, 1, 1), (7, 1, 1, 1), (8, 2, 1, 1), (9, 1, 1, 1)):
        pics.append(frame_picture(fill, 2, 68, 2, fc, alternate, _res_ac, coded=19))
    for fc in ((6, 1, 7, 2), (8, 2, 6, 1), (7, 1, 8, 1), (9, 1, 9, 2)):
        pics.append(frame_picture(fill, 3, 68, 2, fc, alternate, _res_ac, coded=19))
    return case("frame", "b", AC.build(1088, 32, pics))


@functools.lru_cache(maxsize=None)
def il_fcodes_tall():
    """32 x 1088, I P P P B: vertical f_codes 5 to 7, frame-based and field-based"""
    fill = Fill(9003)
    pics = [AC.busy_i(fill.rng, 2, 68, field=True)]
    for fc in ((1, 5, 1, 1), (2, 6, 1, 1), (1, 7, 1, 1)):
        pics.append(frame_picture(fill, 2, 2, 68, fc, alternate, _res_ac, coded=19))
    for fc in ((1, 5, 2, 7), (2, 6, 1, 5), (1, 7, 1, 6)):
        pics.append(frame_picture(fill, 3, 2, 68, fc, alternate, _res_ac, coded=19))
    return case("frame", "b", AC.build(32, 1088, pics))


def halved_wrap_rows(f):
    """48 x 96 (six macroblock rows), one P picture for vertical f = 1 << (f_code - 1).  Row 2: a frame vector (0, -16 f) leaves the
    vertical predictor -16 f, halved -8 f; the field vectors behind it are (0, 8 f): a delta of 16 f, one past the range, written as
    -16 f with a wrap.  Row 3: the frame vector (0, 16 f - 1), halved 8 f - 1; the field vectors (0, -8 f - 2): a delta of -16 f - 1,
    written as 16 f - 1 with a wrap.  Both field vectors lie outside the halved range of Table 7-8 ([-8 f, 8 f - 1]): no conformant
    encoder writes them, but 7.6.3.1 computes them.  The third macroblock of either row is a frame vector predicted from twice the field
    vector, which lies outside the f_code's range itself"""
    still = lambda: dict(motion="frame", fwd=(0, 0))
    rows = [[still() for _ in range(3)] for _ in range(6)]
    up, down = 8 * f, -8 * f - 2
    rows[2] = [dict(motion="frame", fwd=(0, -16 * f)), dict(motion="field", fwd=((0, (0, up)), (1, (0, up)))), dict(motion="frame", fwd=(-2, 2))]
    rows[3] = [dict(motion="frame", fwd=(0, 16 * f - 1)), dict(motion="field", fwd=((1, (0, down)), (0, (0, down)))), dict(motion="frame", fwd=(-1, -3))]
    return rows


@functools.lru_cache(maxsize=None)
def il_halved_wrap():
    """a field vector of a frame picture that needs the wrap of 7.6.3.1 on the halved scale, vertical f_codes 1 to 3, both directions
    (halved_wrap_rows): outside Table 7-8's range, so the requirement is that every decoder here gives the same answer"""
    rng = np.random.RandomState(9004)
    pics = [AC.busy_i(rng, 3, 6, field=True)]
    for f_code in (1, 2, 3):
        pics.append(dict(type=2, q=2, field=True, f_code=(1, f_code, 1, 1), rows=halved_wrap_rows(1 << (f_code - 1))))
    return case("frame", "", AC.build(48, 96, pics))


def far_columns(row, col, mbw):
    """the first and the last eight columns read from the far end of their row"""
    return col < 8 or col >= mbw - 8


@functools.lru_cache(maxsize=None)
def wide_2048():
    """2048 x 32 (the largest size), I P B with field prediction at f_code 9: the first and last eight columns read the far end of their
    row, every other macroblock reads the other parity; a few coded residuals"""
    fill = Fill(9005)
    mbw = 128
    pics = [AC.busy_i(fill.rng, mbw, 2, field=True)]

    def far(ptype):
        rows = []
        for row in range(2):
            mbs = []
            for col in range(mbw):
                if far_columns(row, col, mbw):
                    to = (mbw - 1 - col) if col < 8 else -col        # the mirror column, in macroblocks
                    vx = 32 * to + (1 if col & 1 and to < 0 else 0)
                    v = ((1 - (col & 1), (vx, (1 - 2 * (col & 1)) * (row == (col & 1)))), (col & 1, (vx, 0)))
                else:
                    vx = (7 * col) % 23 - 11
                    v = ((1, (vx, 0)), (0, (-vx, 0))) if col & 1 else ((0, (vx, 0)), (1, (vx, 0)))
                mb = dict(motion="field", fwd=v if ptype == 2 or col % 3 != 1 else None, bwd=None if ptype == 2 or col % 3 == 0 else v)
                if col % 37 == 5:
                    mb.update(cbp=36, dct=col & 1, blocks=[_res_ac(fill.rng), _res_ac(fill.rng)])
                mbs.append(mb)
            rows.append(mbs)
        return dict(type=ptype, q=2, field=True, f_code=(9, 1, 9, 1), rows=rows)
    pics += [far(2), far(3)]
    return case("frame", "b", AC.build(2048, 32, pics))


# ---- dual prime and concealment vectors ----
NINE = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]


def dual_kinds(row, col):
    """dual prime everywhere but each row's first macroblock, a frame vector (with a negative odd vertical component where the picture
    allows one)"""
    return "frame" if col == 0 else "dual"


def dual_stream(seed, w, h, f_codes, tff):
    fill = Fill(seed)
    mbw, rows = (w + 15) // 16, IW.mb_rows(h, 0)
    pics = [TC.textured_i(seed + 50, mbw, rows)]
    for fc in f_codes:
        p = frame_picture(fill, 2, mbw, rows, fc + (1, 1), dual_kinds, TC.residual, tff=tff, coded=11, dmvs=NINE + NINE[::-1])
        p.pop("field")
        pics.append(p)
    return case("tools", "t", TC.build(w, h, pics), tff=tff)


@functools.lru_cache(maxsize=None)
def dual_far():
    return dual_stream(9010, 160, 96, ((1, 1), (3, 2), (5, 4), (4, 3)), 1)


@functools.lru_cache(maxsize=None)
def dual_far_bff():
    return dual_stream(9011, 160, 96, ((2, 1), (5, 3), (4, 4)), 0)


@functools.lru_cache(maxsize=None)
def dual_far_wide():
    return dual_stream(9012, 1088, 32, ((6, 1), (8, 2), (7, 1)), 1)


@functools.lru_cache(maxsize=None)
def dual_far_bff_wide():
    return dual_stream(9013, 1088, 32, ((7, 2), (8, 1), (6, 1)), 0)


def conceal_picture(fill, ptype, mbw, mbh, f_code):
    """a frame picture with concealment vectors: an I picture of intra macroblocks, or a P picture whose rows begin with an intra
    macroblock and go on with predicted and intra macroblocks in turn: every vector is predicted from what a concealment vector left.  Every concealment vector has a residual that is not zero"""
    rng = fill.rng
    rows = []
    for row in range(mbh):
        pmv = [0, 0]
        mbs = []
        for col in range(mbw):
            intra = ptype == 1 or col % 2 == 0
            out = []
            for t in (0, 1):
                f = 1 << (f_code[t] - 1)
                if intra:                                            # any vector in the f_code's range: it is never used; the residual is not zero
                    lo, hi = _frange(f_code[t])
                    ok = lambda v, t=t, f=f: (v - pmv[t]) != 0 and (abs(_wrapd(v - pmv[t], f)) - 1) % f != 0
                    out.append(fill.pick("conceal", 0, t, f_code[t], pmv[t], False, (lo, hi), ok, interval=False))
                else:
                    bound = _xbound(col, mbw) if t == 0 else (-32 * row - 2, 32 * (mbh - 1 - row) + 2)
                    out.append(fill.pick("frame", 0, t, f_code[t], pmv[t], False, bound, lambda v, t=t: W.inside(col, row, (v, 0) if t == 0 else (0, v), mbw, mbh)))
            pmv = out
            if intra:
                m = dict(TC._textured(rng), cmv=tuple(out), dct=0)
            else:
                m = dict(fwd=tuple(out), motion="frame")
            mbs.append(m)
        rows.append(mbs)
    return dict(type=ptype, prec=0, q=3, f_code=tuple(f_code) + (1, 1), ivf=1, cmv=1, rows=rows)


def _wrapd(delta, f):
    return delta + 32 * f if delta < -16 * f else delta - 32 * f if delta > 16 * f - 1 else delta


@functools.lru_cache(maxsize=None)
def conceal_fcodes():
    """160 x 96, I P P with concealment_motion_vectors 1 and Table B-15: f_codes (4, 3) and (7, 5), a residual that is not zero in every
    concealment vector; in the P pictures every predicted macroblock stands behind an intra one and is predicted from what its
    concealment vector left"""
    fill = Fill(9020)
    pics = [conceal_picture(fill, 1, 10, 6, (4, 3)), conceal_picture(fill, 2, 10, 6, (7, 5)), conceal_picture(fill, 2, 10, 6, (4, 3))]
    return case("tools", "t", TC.build(160, 96, pics))


# ---- field pictures ----
def field_picture(fill, ptype, ps, mbw, rows, f_code, avail, res, kinds, coded=7, dmvs=None):
    """the rows of a P or B field picture: kinds(row, col) -> "field" | "16x8" | "dual" | "skip"; avail: the parities a select may name"""
    rng = fill.rng
    out, n = [], 0
    par = ps - 1
    for row in range(rows):
        pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
        mbs = []
        for col in range(mbw):
            kind = kinds(row, col)
            n += 1
            if kind == "dual" and (ptype != 2 or len(avail) < 2):
                kind = "field"
            if kind == "skip":
                if ptype == 2:
                    pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                mbs.append(dict(skip=True))
                continue
            dirs = (1, 0) if ptype == 2 else ((1, 1), (1, 0), (0, 1))[(row + col + n // 5) % 3]
            if ptype == 3 and col + 1 < mbw and kinds(row, col + 1) == "skip":
                kind = "field"                                       # (a skipped macroblock takes PMV[0][s] as a 16 x 16 field vector: it must read inside)
            mb = dict(motion=kind, fwd=None, bwd=None)
            sel = lambda: int(avail[int(rng.randint(len(avail)))]) if ptype == 2 else int(rng.randint(2))
            for s in (0, 1):
                if not dirs[s]:
                    continue
                fh, fv = f_code[2 * s], f_code[2 * s + 1]
                yb = lambda half: (-32 * row - (16 if half else 0) - 2, 32 * (rows - 1 - row) + (16 if half == 0 else 0) + 2)
                stay = ptype == 3 and col + 1 < mbw and kinds(row, col + 1) == "skip"      # the same vector must be legal one column on
                if kind == "field":
                    okx = lambda v: FW.inside(col, row, (v, 0), mbw, rows) and (not stay or FW.inside(col + 1, row, (v, 0), mbw, rows))
                    vx = fill.pick("fieldpic", s, 0, fh, pmv[0][s][0], False, _xbound(col, mbw), okx)
                    vy = fill.pick("fieldpic", s, 1, fv, pmv[0][s][1], False, yb(None), lambda v: FW.inside(col, row, (0, v), mbw, rows))
                    pmv[0][s] = [vx, vy]
                    pmv[1][s] = [vx, vy]
                    mb["bwd" if s else "fwd"] = (sel(), (vx, vy))
                elif kind == "16x8":
                    vs = []
                    for r in (0, 1):
                        vx = fill.pick("16x8_%d" % r, s, 0, fh, pmv[r][s][0], False, _xbound(col, mbw), lambda v: FW.inside(col, row, (v, 0), mbw, rows, r))
                        vy = fill.pick("16x8_%d" % r, s, 1, fv, pmv[r][s][1], False, yb(r), lambda v: FW.inside(col, row, (0, v), mbw, rows, r))
                        pmv[r][s] = [vx, vy]
                        vs.append((sel(), (vx, vy)))
                    mb["bwd" if s else "fwd"] = tuple(vs)
                else:
                    dmv = dmvs.pop(0) if dmvs else (int(rng.randint(-1, 2)), int(rng.randint(-1, 2)))
                    e = 1 if par else -1
                    inside = lambda v, t: all(FW.inside(col, row, (x, 0) if t == 0 else (0, x), mbw, rows) for x in (v, VR.half(v) + dmv[t] + (e if t else 0)))
                    vx = fill.pick("dualpic%d" % par, 0, 0, fh, pmv[0][0][0], False, _xbound(col, mbw), lambda v: inside(v, 0))
                    vy = fill.pick("dualpic%d" % par, 0, 1, fv, pmv[0][0][1], False, yb(None), lambda v: inside(v, 1))
                    pmv[0][0] = [vx, vy]
                    pmv[1][0] = [vx, vy]
                    mb["fwd"] = ((vx, vy), dmv)
            if n % coded == 0:
                mb.update(cbp=36, blocks=[res(rng), res(rng)])
            mbs.append(mb)
        out.append(mbs)
    return dict(type=ptype, ps=ps, q=2, f_code=tuple(f_code), rows=out)


def field_kinds(row, col):
    return ("field", "16x8", "dual", "16x8", "field", "16x8")[(col + row) % 6]


def field_kinds_skip(mbw):
    return lambda row, col: "skip" if col in (3, mbw - 3) and mbw > 6 else field_kinds(row, col)


def field_stream(seed, w, h, plan):
    """plan: [(letters of a pair, the first field's picture_structure, f_code)]; the first pair is I + P: its P field reads the first
    field of its own frame, the only one there"""
    fill = Fill(seed)
    mbw, rows = (w + 15) // 16, (h + 31) // 32
    pics = []
    for k, (letters, first, fc) in enumerate(plan):
        for nth, c in enumerate(letters):
            ps = first if nth == 0 else 3 - first
            ptype = " IPB".index(c)
            if ptype == 1:
                pics.append(FC.textured(seed + 10 * k + nth, ps, mbw, rows))
                continue
            avail = (0, 1)
            if ptype == 2 and k == 0:
                avail = (first - 1,)                                 # the stream's first frame: only its first field is there
            pics.append(field_picture(fill, ptype, ps, mbw, rows, fc, avail, FC._res, field_kinds_skip(mbw) if ptype == 3 or k > 1 else field_kinds,
                                      dmvs=NINE + NINE[::-1]))
    return case("field", "fb", FC.build(w, h, pics))


@functools.lru_cache(maxsize=None)
def fld_fcodes():
    """160 x 96 (a field is 160 x 48): every pairing of top / bottom and first / second, P and B fields, field-based, 16 x 8 and dual
    prime, horizontal f_codes 1 to 5 and vertical 1 to 3"""
    return field_stream(9030, 160, 96, [("IP", 1, (1, 1, 1, 1)), ("PP", 2, (2, 2, 1, 1)), ("PP", 1, (3, 3, 1, 1)), ("PP", 2, (4, 1, 1, 1)), ("PP", 1, (5, 2, 1, 1)),
                                       ("BB", 1, (5, 3, 4, 2)), ("BB", 2, (3, 1, 5, 3)), ("PP", 2, (5, 3, 1, 1)), ("BB", 2, (1, 2, 2, 1)), ("BB", 1, (2, 3, 1, 2))])


@functools.lru_cache(maxsize=None)
def fld_fcodes_tall():
    """32 x 1088 (a field is 32 x 544): vertical f_codes 4 to 7"""
    return field_stream(9031, 32, 1088, [("IP", 2, (1, 4, 1, 1)), ("PP", 1, (1, 5, 1, 1)), ("PP", 2, (2, 6, 1, 1)), ("PP", 1, (1, 7, 1, 1)),
                                        ("BB", 1, (1, 6, 2, 7)), ("BB", 2, (2, 4, 1, 5))])


@functools.lru_cache(maxsize=None)
def wide_2048_fields():
    """2048 x 64 as field pictures (a field is 2048 x 32), I I P P at f_code 9: the first and last eight columns read the far end of their
    row from the other parity, the others stay near"""
    fill = Fill(9032)
    mbw = 128
    pics = [FC.textured(9033, 1, mbw, 2), FC.textured(9034, 2, mbw, 2)]
    for ps in (1, 2):
        rows = []
        for row, sign in ((0, 1), (1, -1)):                          # vertical components point into the field
            mbs = []
            for col in range(mbw):
                if far_columns(row, col, mbw):
                    to = (mbw - 1 - col) if col < 8 else -col
                    vx = 32 * to + (1 if col & 1 and to < 0 else 0)
                    mb = dict(motion="field", fwd=((ps - 1) ^ 1 ^ (col & 1), (vx, sign * (col & 1))))
                elif col % 5 == 2:
                    mb = dict(motion="16x8", fwd=((0, ((3 * col) % 17 - 8, sign)), (1, (-((5 * col) % 13), 2 * sign))))
                else:
                    mb = dict(motion="field", fwd=(col & 1, ((7 * col) % 23 - 11, sign * (col % 3))))
                if col % 37 == 5:
                    mb.update(cbp=36, blocks=[FC._res(fill.rng), FC._res(fill.rng)])
                mbs.append(mb)
            rows.append(mbs)
        pics.append(dict(type=2, ps=ps, q=2, f_code=(9, 1, 1, 1), rows=rows))
    return case("field", "f", FC.build(2048, 64, pics))


CASES = dict(il_fcodes=il_fcodes, il_fcodes_wide=il_fcodes_wide, il_fcodes_tall=il_fcodes_tall, il_halved_wrap=il_halved_wrap, wide_2048=wide_2048,
             dual_far=dual_far, dual_far_bff=dual_far_bff, dual_far_wide=dual_far_wide, dual_far_bff_wide=dual_far_bff_wide, conceal_fcodes=conceal_fcodes,
             fld_fcodes=fld_fcodes, fld_fcodes_tall=fld_fcodes_tall, wide_2048_fields=wide_2048_fields)
NAMES = tuple(sorted(CASES))
BATCH_NAMES = ("fld_fcodes", "fld_fcodes_tall", "il_fcodes", "il_fcodes_tall", "il_fcodes_wide", "wide_2048", "wide_2048_fields")      # B pictures or field pictures


def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def ref_frames(name, wrong=()):
    """the frames of vec_ref for the case"""
    c = get(name)
    return VR.frames(c["kind"], c["log"], wrong)


@functools.lru_cache(maxsize=None)
def trace(name):
    return VR.walk(get(name)["log"])[1]


# ---- the refusals: a component inside its f_code's range whose read is not inside the picture ----
@functools.lru_cache(maxsize=None)
def refusals():
    """name -> dict(stream, needs, offset): the offset is that of the slice that holds the macroblock - the I picture in front has six
    slices (the field pictures: three a field), the P picture's row `row` is its slice number row"""
    out = {}
    still = lambda: dict(motion="frame", fwd=(0, 0))
    # 160 x 96, f_code (5, 4): the bottom-field vector of the field-based macroblock in column 2, row 3 is 225 = 2 * (160 - 16 - 32) + 1:
    # one half sample past the right edge, inside [-256, 255]
    rows = [[still() for _ in range(10)] for _ in range(6)]
    rows[3][2] = dict(motion="field", fwd=((0, (224, 3)), (1, (225, 3))))
    s, log = TC.build(160, 96, [TC.textured_i(9040, 10, 6), dict(type=2, q=2, f_code=(5, 4, 1, 1), rows=rows)])
    out["field_vector_right"] = dict(stream=s, needs="", offset=[a for k, a in log["writer"]["units"] if k == "slice"][6 + 3])
    # the dual-prime vector (100, 2) in column 5, row 2 reads 50 samples to the right, inside; with top_field_first 1 the vector derived
    # for the bottom-field lines is (150, 5): 75 samples, 80 + 75 + 16 > 160
    rows = [[still() for _ in range(10)] for _ in range(6)]
    rows[2][5] = dict(motion="dual", fwd=((100, 2), (0, 1)))
    s, log = TC.build(160, 96, [TC.textured_i(9041, 10, 6), dict(type=2, q=2, f_code=(5, 4, 1, 1), tff=1, rows=rows)])
    out["derived_vector_right"] = dict(stream=s, needs="t", offset=[a for k, a in log["writer"]["units"] if k == "slice"][6 + 2])
    # field pictures, f_code (5, 3): the lower 16 x 8 of column 7, row 1 of the second P field by (-225, 2): one half sample past the left
    # edge (2 * 16 * 7 = 224), inside [-256, 255]; the upper 16 x 8 by (-224, 2) is inside
    fstill = lambda: dict(motion="field", fwd=(0, (0, 0)))
    rows = [[fstill() for _ in range(10)] for _ in range(3)]
    bad = [list(r) for r in rows]
    bad[1][7] = dict(motion="16x8", fwd=((0, (-224, 2)), (0, (-225, 2))))
    pics = [FC.textured(9042, 1, 10, 3), FC.textured(9043, 2, 10, 3), dict(type=2, ps=1, q=2, f_code=(5, 3, 1, 1), rows=rows), dict(type=2, ps=2, q=2, f_code=(5, 3, 1, 1), rows=bad)]
    s, log = FC.build(160, 96, pics)
    out["lower_16x8_left"] = dict(stream=s, needs="f", offset=[a for k, a in log["writer"]["units"] if k == "slice"][3 + 3 + 3 + 1])
    return out


# ---- literal known answers: name -> dict(stream, needs, frames=[(Y, U, V)]) ----
BANDS = (40, 64, 88, 112, 136, 160, 184, 208)                      # the luma levels of the eight bands of eight lines (or samples)
CROWS = (50, 100, 150, 200)                                         # the chroma levels of the four macroblock rows


def _mean(a, b):
    return (a + b + 1) >> 1


@functools.lru_cache(maxsize=None)
def known():
    out = {}
    # -- the halved negative odd predictor.  48 x 48 (four macroblock rows of sixteen lines; 64 coded lines), luma line y at level
    # BANDS[y // 8], chroma line y at CROWS[y // 8].  Row 1 of the P picture: a frame vector (0, -3), then a field-based macroblock whose
    # two vectors are written with motion_code 0 in both components: they are the predictor, (0, -3 DIV 2) = (0, -2): one field line
    # up.  (-3 / 2 toward zero is -1: half a line up.)
    ref = IC.intra_levels(3, 4, lambda r, c: (BANDS[2 * r], BANDS[2 * r], BANDS[2 * r + 1], BANDS[2 * r + 1], CROWS[r], CROWS[r]))
    still = lambda: IC.fmb(0, (0, 0), 1, (0, 0))
    p = IC.pred_picture(2, 3, 4, lambda r, c: (IC.frmb((0, -3)), IC.fmb(0, (0, -2), 1, (0, -2)), still())[c] if r == 1 else still())
    s, L = IW.stream(48, 48, [ref, p])
    assert [c[1] for c in L["codes"][2:6]] == [0, 0, 0, 0], "the field vectors are their predictors"
    y0 = np.repeat(np.asarray([BANDS[y // 8] for y in range(48)], np.uint8)[:, None], 48, axis=1)
    c0 = np.repeat(np.asarray([CROWS[y // 8] for y in range(24)], np.uint8)[:, None], 24, axis=1)
    y1, c1 = y0.copy(), c0.copy()
    b1, b2, b3 = BANDS[1], BANDS[2], BANDS[3]
    # column 0, the frame vector: line y is the mean of lines y - 2 and y - 1
    y1[16:32, 0:16] = np.asarray([b1, _mean(b1, b2), b2, b2, b2, b2, b2, b2, b2, _mean(b2, b3), b3, b3, b3, b3, b3, b3], np.uint8)[:, None]
    c1[8:16, 0:8] = np.asarray([_mean(CROWS[0], CROWS[1])] + [CROWS[1]] * 7, np.uint8)[:, None]
    # column 1, the field vectors: field line k of either parity lies in band k // 4; lines 7 .. 14 in the place of 8 .. 15.  Chroma:
    # -2 / 2 = -1, half a field line: the first line of either field is the mean with the row above
    y1[16:32, 16:32] = np.asarray([b1, b1, b2, b2, b2, b2, b2, b2, b2, b2, b3, b3, b3, b3, b3, b3], np.uint8)[:, None]
    c1[8:16, 8:16] = np.asarray([_mean(CROWS[0], CROWS[1])] * 2 + [CROWS[1]] * 6, np.uint8)[:, None]
    out["halved_negative_odd"] = dict(stream=s, needs="", frames=[(y0, c0, c0.copy()), (y1, c1, c1.copy())])
    # -- the dual-prime factors with top_field_first 0.  48 x 64, luma sample x at level BANDS[x // 8], chroma sample x at CROWS[x // 8]
    # in every line.  Column 0 of rows 0 to 2: the vector (16, 0) - eight samples - with dmvector (0, 1).  The top-field lines read the
    # bottom field by (16 * 3 // 2, 0 + 1 - 1) = (24, 0): twelve samples; the bottom-field lines read the top field by (16 // 2,
    # 0 + 1 + 1) = (8, 2): four samples, one line down (the columns are constant).  With top_field_first 1 the two change places
    z = np.zeros(64, np.int64)
    flat = lambda c: dict(intra=True, dct=0, blocks=[(z, BANDS[2 * c]), (z, BANDS[2 * c + 1]), (z, BANDS[2 * c]), (z, BANDS[2 * c + 1]), (z, CROWS[c]), (z, CROWS[c])])
    ref = dict(type=1, prec=0, q=3, rows=[[flat(c) for c in range(3)] for _ in range(4)])
    rows = [[dict(motion="dual", fwd=((16, 0), (0, 1))) if (c == 0 and r < 3) else dict(motion="frame", fwd=(0, 0)) for c in range(3)] for r in range(4)]
    s, log = TC.build(48, 64, [ref, dict(type=2, q=2, tff=0, f_code=(2, 1, 1, 1), rows=rows)])
    y0 = np.repeat(np.asarray([BANDS[x // 8] for x in range(48)], np.uint8)[None, :], 64, axis=0)
    c0 = np.repeat(np.asarray([CROWS[x // 8] for x in range(24)], np.uint8)[None, :], 32, axis=0)
    y1, c1 = y0.copy(), c0.copy()
    g0, g1, g2, g3 = BANDS[:4]
    top = [g1] * 4 + [_mean(g1, g2)] * 4 + [g2] * 4 + [_mean(g2, g3)] * 4                 # (x + 8) with (x + 12)
    bottom = [_mean(g1, g0)] * 4 + [g1] * 4 + [_mean(g2, g1)] * 4 + [g2] * 4              # (x + 8) with (x + 4)
    y1[0:48:2, 0:16], y1[1:48:2, 0:16] = np.asarray(top, np.uint8), np.asarray(bottom, np.uint8)
    k0, k1 = CROWS[:2]
    ctop = [k0] * 2 + [_mean(k0, k1)] * 2 + [k1] * 4                                       # chroma: (x + 4) with (x + 6)
    cbottom = [k0] * 4 + [_mean(k1, k0)] * 2 + [k1] * 2                                    # (x + 4) with (x + 2)
    c1[0:24:2, 0:8], c1[1:24:2, 0:8] = np.asarray(ctop, np.uint8), np.asarray(cbottom, np.uint8)
    out["dual_bottom_field_first"] = dict(stream=s, needs="t", frames=[(y0, c0, c0.copy()), (y1, c1, c1.copy())])
    # -- a far read at the largest size.  2048 x 32, macroblock column c at luma level 30 + c and chroma level 60 + c.  Column 0 is
    # field-based with both vectors (4064, 0) - 127 macroblocks to the right, f_code 9 - and column 127 with (-4064, 0); the top-field
    # lines read the bottom field and the reverse.  The two columns change levels
    ref = IC.intra_levels(128, 2, lambda r, c: (30 + c,) * 4 + (60 + c,) * 2)
    far = lambda r, c: IC.fmb(1, (4064, 0), 0, (4064, 0)) if c == 0 else IC.fmb(1, (-4064, 0), 0, (-4064, 0)) if c == 127 else still()
    s, L = IW.stream(2048, 32, [ref, IC.pred_picture(2, 128, 2, far, f_code=(9, 1, 1, 1))])
    y0 = np.repeat(np.asarray([30 + x // 16 for x in range(2048)], np.uint8)[None, :], 32, axis=0)
    c0 = np.repeat(np.asarray([60 + x // 8 for x in range(1024)], np.uint8)[None, :], 16, axis=0)
    y1, c1 = y0.copy(), c0.copy()
    y1[:, 0:16], y1[:, 2032:2048], c1[:, 0:8], c1[:, 1016:1024] = 30 + 127, 30, 60 + 127, 60
    out["far_read_2048"] = dict(stream=s, needs="", frames=[(y0, c0, c0.copy()), (y1, c1, c1.copy())])
    return out


# ---- the wrong forms of vec_ref: the case that shows each ----
CATCHES = dict(half_toward_zero="dual_far_bff", wrap_on_doubled="il_halved_wrap", pmv_not_doubled="il_halved_wrap", pmv_1_not_copied_frame="il_fcodes",
               h_v_f_code_swapped="il_halved_wrap", backward_uses_forward_f_code="il_fcodes", residual_read_at_code_0="il_halved_wrap",
               residual_width_f_code="il_halved_wrap", second_16x8_from_pmv_0="wide_2048_fields", dual_from_predictor="dual_far", dual_factors_swapped="dual_far",
               dual_half_floor="dual_far", dmvector_signs_swapped="fld_fcodes", e_wrong_sign_field="fld_fcodes_tall", vector_kept_in_8_bits="il_fcodes",
               vector_kept_in_12_bits="wide_2048", chroma_shift="il_fcodes", concealment_resets_predictors="conceal_fcodes")


def changed(name, wrong):
    """what the wrong form does to the case: "=" the walk gives the same vectors (equivalent: the frames cannot change), "." other vectors
    and the same frames, "X" other frames, "O" a vector that reads outside its picture (such a decoder refuses the stream)"""
    c = get(name)
    if wrong != "chroma_shift" and VR.vectors(c["log"], wrong) == VR.vectors(c["log"]):
        return "="
    try:
        bad = ref_frames(name, wrong)
    except VR.Outside:
        return "O"
    same = all(np.array_equal(a, b) for x, y in zip(ref_frames(name), bad) for a, b in zip(x, y))
    return "." if same else "X"
