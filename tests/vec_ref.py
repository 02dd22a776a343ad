"""A second statement of ISO/IEC 13818-2 clause 7.6.3 - the motion vectors - for the decoder's tests, in plain Python integers, typed
from the standard's text.  It parses nothing and imports neither decoder.py nor anything compiled from csrc/: it takes what the
writer logged - per vector component (motion_code with its sign, motion_residual), per macroblock the mode, the directions, the
selects and the dmvector - and returns the absolute vectors of every macroblock.  The frames then come from the references that take
absolute vectors and never parse: tests/arith_ref.py (frame pictures), tests/mbt_ref.py (dual prime, concealment vectors) and
tests/fld_ref.py (field pictures).

    component(pred, code, residual, f_code)     7.6.3.1: delta from the code and the residual, the sum wrapped into [-16 f, 16 f - 1]
    vector(pmv, codes, f_codes, halved)         both components from PMV[r][s]; halved: a field vector of a frame picture - the vertical
                                                prediction is PMV DIV 2 (toward minus infinity), the predictor twice the vector afterwards
    walk(log)                                   the predictors of 7.6.3.1 to 7.6.3.4 macroblock by macroblock (below)
    half(a)                                     the "//" of 7.6.3.6: division by 2 to the nearest integer, halves away from zero
    dual_frame(v, dmv, tff), dual_field(v, dmv, parity)      7.6.3.6 with table 7-11 and 7-12 (m and e)
    chroma(a)                                   7.6.3.7: "/" 2, toward zero

The predictors (PMV[r][s][t]; r the vector, s the direction, t the component):
    a slice begins; an intra macroblock without a concealment vector; a P picture's macroblock without a vector; a P picture's skipped
    macroblock                                          every predictor 0 (7.6.3.4)
    frame pictures  frame-based                          from and into PMV[0][s], PMV[1][s] follows
                    field-based                          vector r from and into PMV[r][s], the vertical one halved in and doubled out
                    dual prime                           from and into PMV[0][0] as a field vector, PMV[1][0] follows
    field pictures  field-based                          from and into PMV[0][s], PMV[1][s] follows
                    16 x 8                               vector r from and into PMV[r][s]
                    dual prime                           from and into PMV[0][0], PMV[1][0] follows
    a concealment vector                                 from and into PMV[0][0] with the forward f_codes, PMV[1][0] follows; a frame
                                                         picture's is a frame vector
    a B picture's skipped macroblock                     the directions of the macroblock in front, PMV[0][s] as the vectors (frame
                                                         vectors in a frame picture, field vectors of the same parity in a field
                                                         picture); the predictors stay

A wrong form can be named, one at a time (WRONG): the walk then gives what a decoder with that mistake computes from the same codes.
Where a mistake is one of parsing (a residual of another width), the form here is its arithmetic: the written code and residual put
into the formula the mistaken decoder would use.
    half_toward_zero                the vertical prediction of a field vector PMV / 2 toward zero (differs for negative odd PMV)
    wrap_on_doubled                 the range test on twice the field vector
    pmv_not_doubled                 the predictor of a field vector left at the vector
    pmv_1_not_copied_frame          PMV[1][s] left alone by a frame-based vector
    h_v_f_code_swapped              f_code[s][1 - t]
    backward_uses_forward_f_code    f_code[0][t] for a backward vector
    residual_read_at_code_0         the formula with the residual at motion_code 0 (f > 1)
    residual_width_f_code           a residual of r_size + 1 bits: f doubled in the delta
    second_16x8_from_pmv_0          the second vector of a 16 x 8 macroblock from PMV[0][s]
    dual_from_predictor             the derived vectors from the (doubled) predictor, not from the vector
    dual_factors_swapped            table 7-11's 1 and 3 by the wrong top_field_first
    dual_half_floor                 >> 1 in the place of "//"
    dmvector_signs_swapped          dmvector '10' read as -1, '11' as +1
    e_wrong_sign_field              e + 1 in a top field, - 1 in a bottom field
    vector_kept_in_8_bits, vector_kept_in_12_bits      the vector and the predictor kept in that many bits
    chroma_shift                    >> 1 in the place of "/" 2
    concealment_resets_predictors   the predictors reset behind an intra macroblock that has a concealment vector"""

WRONG = ("half_toward_zero", "wrap_on_doubled", "pmv_not_doubled", "pmv_1_not_copied_frame", "h_v_f_code_swapped", "backward_uses_forward_f_code",
         "residual_read_at_code_0", "residual_width_f_code", "second_16x8_from_pmv_0", "dual_from_predictor", "dual_factors_swapped", "dual_half_floor",
         "dmvector_signs_swapped", "e_wrong_sign_field", "vector_kept_in_8_bits", "vector_kept_in_12_bits", "chroma_shift", "concealment_resets_predictors")


def _tuple(wrong):
    wrong = (wrong,) if isinstance(wrong, str) else tuple(wrong)
    assert all(m in WRONG for m in wrong), wrong
    return wrong


def _kept(v, wrong):
    for name, bits in (("vector_kept_in_8_bits", 8), ("vector_kept_in_12_bits", 12)):
        if name in wrong:
            v = ((v + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))
    return v


def delta_of(code, residual, f_code, wrong=()):
    r_size = f_code - 1
    f = 1 << r_size
    if f == 1 or (code == 0 and "residual_read_at_code_0" not in wrong):
        return code
    delta = (abs(code) - 1) * (2 * f if "residual_width_f_code" in wrong else f) + residual + 1
    return -delta if code < 0 else delta


def wrapped(v, f_code):
    """-> (v in [low, high], the multiple of the range that was added: +1, 0 or -1)"""
    f = 1 << (f_code - 1)
    high, low, rng = 16 * f - 1, -16 * f, 32 * f
    if v < low:
        return v + rng, 1
    if v > high:
        return v - rng, -1
    return v, 0


def component(pred, code, residual, f_code, wrong=()):
    """7.6.3.1: vector'[r][s][t] from its prediction"""
    assert 1 <= f_code <= 9 and -16 <= code <= 16 and 0 <= residual < 1 << (f_code - 1)
    return wrapped(pred + delta_of(code, residual, f_code, _tuple(wrong)), f_code)[0]


def field_component(pmv, code, residual, f_code, wrong=()):
    """the vertical component of a field vector of a frame picture -> (the vector, the predictor left behind, the wrap)"""
    wrong = _tuple(wrong)
    pred = (-((-pmv) // 2) if pmv < 0 else pmv // 2) if "half_toward_zero" in wrong else pmv // 2      # DIV: toward minus infinity
    raw = pred + delta_of(code, residual, f_code, wrong)
    if "wrap_on_doubled" in wrong:
        d, k = wrapped(2 * raw, f_code)
        v = d // 2
    else:
        v, k = wrapped(raw, f_code)
    v = _kept(v, wrong)
    return v, _kept(v if "pmv_not_doubled" in wrong else 2 * v, wrong), k


def half(a, wrong=()):
    return a >> 1 if "dual_half_floor" in wrong else (a + (1 if a > 0 else 0)) >> 1


def _dmv(d, wrong):
    return tuple(-x for x in d) if "dmvector_signs_swapped" in wrong else tuple(d)


def dual_frame(v, dmv, tff, wrong=()):
    """7.6.3.6, a frame picture -> (T, B): the vector that reads the bottom field for the top-field lines (e -1), and the one that reads
    the top field for the bottom-field lines (e +1).  Table 7-11's m is the distance in field periods between the field read and the
    field predicted (the vector itself spans two): with top_field_first 1 the top-field lines lie one period behind the bottom field
    in front (m 1) and the bottom-field lines three behind its top field (m 3); with top_field_first 0 the other way round"""
    wrong = _tuple(wrong)
    m_bt, m_tb = (1, 3) if bool(tff) != ("dual_factors_swapped" in wrong) else (3, 1)
    d = _dmv(dmv, wrong)
    return ((half(m_bt * v[0], wrong) + d[0], half(m_bt * v[1], wrong) + d[1] - 1),
            (half(m_tb * v[0], wrong) + d[0], half(m_tb * v[1], wrong) + d[1] + 1))


def dual_field(v, dmv, parity, wrong=()):
    """7.6.3.6, a field picture of parity 0 (top) or 1 (bottom) -> the vector that reads the field of the opposite parity: m is 1, e is
    e[opposite][parity]: -1 for a top field, +1 for a bottom field"""
    wrong = _tuple(wrong)
    e = (1 if parity else -1) * (-1 if "e_wrong_sign_field" in wrong else 1)
    d = _dmv(dmv, wrong)
    return (half(v[0], wrong) + d[0], half(v[1], wrong) + d[1] + e)


def chroma(a, wrong=()):
    """7.6.3.7, 4:2:0: both components "/" 2"""
    if "chroma_shift" in _tuple(wrong):
        return a >> 1
    return -((-a) // 2) if a < 0 else a // 2


def _zero():
    return [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]


class _Codes:
    def __init__(self, codes):
        self.codes, self.at = list(codes), 0

    def next(self):
        c = self.codes[self.at]
        self.at += 1
        return c


def walk(log, wrong=()):
    """log: dict(pictures=[dict(type, f_code, ps (1 | 2: a field picture), tff, cmv, mbs=[...])] in coded order, writer=dict(codes=[(f_code,
    motion_code, residual, ...)] in the order written)) with the macroblocks of arith_cases / mbt_cases / fld_cases.build (every row one
    slice) -> (the pictures with every vector replaced by the one read here - a dual-prime macroblock also gets derived=, the vectors of
    7.6.3.6 - and the trace: one dict per component read)"""
    wrong = _tuple(wrong)
    src = _Codes(log["writer"]["codes"])
    pictures, trace = [], []
    for index, pic in enumerate(log["pictures"]):
        ptype, fc = pic["type"], tuple(pic.get("f_code", (1, 1, 1, 1)))
        field_picture = pic.get("ps", 3) != 3
        parity = pic.get("ps", 3) - 1
        pmv, front = _zero(), None
        mbs = []

        def read(r, s, base_r, halved, mode, mb):
            """vector r of direction s from PMV[base_r][s] into PMV[r][s]"""
            out = []
            for t in (0, 1):
                ss = 0 if (s == 1 and "backward_uses_forward_f_code" in wrong) else s
                f_code = fc[2 * ss + (1 - t if "h_v_f_code_swapped" in wrong else t)]
                said, code, residual = src.next()[:3]
                assert said == fc[2 * s + t], "the writer wrote this component with the f_code the rule names"
                residual &= (1 << (f_code - 1)) - 1                 # (a wrong f_code: the bits that fit its formula)
                before = pmv[base_r][s][t]
                if halved and t == 1:
                    v, left, k = field_component(before, code, residual, f_code, wrong)
                    pred = before // 2
                else:
                    v, k = wrapped(before + delta_of(code, residual, f_code, wrong), f_code)
                    v = left = _kept(v, wrong)
                    pred = before
                pmv[r][s][t] = left
                out.append(v)
                trace.append(dict(pic=index, type=ptype, row=mb["row"], col=mb["col"], mode=mode, s=s, r=r, t=t, f_code=f_code, code=code, residual=residual,
                                  pmv=before, pred=pred, vector=v, wrap=k, field_picture=field_picture))
            return tuple(out)

        for mb in pic["mbs"]:
            mb = dict(mb)
            if mb["col"] == 0:                                      # a slice begins
                pmv, front = _zero(), None
            if mb.get("skip"):
                if ptype == 2:
                    pmv = _zero()
                    mb["fwd"], mb["bwd"] = ((parity, (0, 0)) if field_picture else (0, 0)), None
                else:
                    assert front is not None, "a B picture's skipped macroblock stands behind a predicted one"
                    mb["fwd"] = tuple(pmv[0][0]) if front[0] else None
                    mb["bwd"] = tuple(pmv[0][1]) if front[1] else None
            elif mb["intra"]:
                if pic.get("cmv"):
                    read(0, 0, 0, False, "conceal", mb)
                    pmv[1][0] = list(pmv[0][0])
                    if "concealment_resets_predictors" in wrong:
                        pmv = _zero()
                else:
                    pmv = _zero()
                front = None
            elif mb["nomc"]:                                        # a P picture's macroblock without a vector
                pmv = _zero()
                front = (1, 0)
            else:
                motion = mb.get("motion") or "frame"
                for s, name in ((0, "fwd"), (1, "bwd")):
                    told = mb.get(name)
                    if told is None:
                        continue
                    if motion == "dual":
                        v = read(0, 0, 0, not field_picture, "dual", mb)
                        pmv[1][0] = list(pmv[0][0])
                        dmv = tuple(told[1])
                        base = v
                        if "dual_from_predictor" in wrong:
                            base = tuple(pmv[0][0])
                        mb[name] = (v, dmv)
                        mb["derived"] = dual_field(base, dmv, parity, wrong) if field_picture else dual_frame(base, dmv, pic.get("tff", 1), wrong)
                    elif field_picture and motion == "field":
                        mb[name] = (told[0], read(0, s, 0, False, "field", mb))
                        pmv[1][s] = list(pmv[0][s])
                    elif field_picture:                             # 16 x 8
                        first = read(0, s, 0, False, "16x8", mb)
                        second = read(1, s, 0 if "second_16x8_from_pmv_0" in wrong else 1, False, "16x8", mb)
                        mb[name] = ((told[0][0], first), (told[1][0], second))
                    elif motion == "frame":
                        mb[name] = read(0, s, 0, False, "frame", mb)
                        if "pmv_1_not_copied_frame" not in wrong:
                            pmv[1][s] = list(pmv[0][s])
                    else:                                           # field-based in a frame picture
                        mb[name] = tuple((told[r][0], read(r, s, r, True, "field", mb)) for r in (0, 1))
                front = (1, 0) if ptype == 2 else (int(mb.get("fwd") is not None), int(mb.get("bwd") is not None))
            mbs.append(mb)
        pictures.append(dict(pic, mbs=mbs))
    assert src.at == len(src.codes), "every code the writer wrote was read"
    return pictures, trace


def vectors(log, wrong=()):
    """per picture the list of (row, col, fwd, bwd, derived) of its macroblocks"""
    return [[(m["row"], m["col"], m.get("fwd"), m.get("bwd"), m.get("derived")) for m in p["mbs"]] for p in walk(log, wrong)[0]]


class Outside(Exception):
    """a vector of the walk reads outside its picture or field: a decoder with that mistake refuses the stream"""


def frames(kind, log, wrong=()):
    """the frames of the log in display order with the vectors of walk(log, wrong): kind "frame" -> arith_ref, "tools" -> mbt_ref,
    "field" -> fld_ref.  The references halve their chroma vectors with chroma() for the call"""
    import arith_ref
    import fld_ref
    import mbt_ref
    wrong = _tuple(wrong)
    out = dict(log, pictures=walk(log, wrong)[0])
    halve = lambda a: chroma(a, wrong)
    saved = (mbt_ref.toward_zero, fld_ref.toward_zero, arith_ref._halve)
    mbt_ref.toward_zero, fld_ref.toward_zero, arith_ref._halve = halve, halve, (lambda v, floor: halve(v))
    try:
        return dict(frame=arith_ref.frames, tools=mbt_ref.frames, field=fld_ref.frames)[kind](out)
    except (AssertionError, IndexError, ValueError) as e:
        if wrong:
            raise Outside(str(e))
        raise
    finally:
        mbt_ref.toward_zero, fld_ref.toward_zero, arith_ref._halve = saved
