"""A second implementation of field pictures for the decoder's tests, in numpy, in the manner of tests/arith_ref.py (whose inverse
quantisation and inverse DCT it uses) and tests/mbt_ref.py: it never parses a stream - fld_cases.build() hands it the macroblocks it
wrote, with absolute vectors - and computes the frames.  A frame is kept as its two fields; a field picture of parity p writes field p
of its frame, and reads the most recently decoded anchor field of the parity a select names: for the second field of an anchor frame
the other parity is the first field of its own frame.

    field-based   16 x 16 (chroma 8 x 8, both components / 2 toward zero) from the field the select names
    16 x 8        the upper half by vector 0, the lower by vector 1; chroma 8 x 4 each
    dual prime    (a + b + 1) >> 1 of the same parity by (vx, vy) and the other parity by (h(vx) + d0, h(vy) + d1 + e),
                  h(a) = (a + (a > 0)) >> 1, e = -1 in a top field, + 1 in a bottom field
    no vector     a P field's macroblock without one, and its skipped macroblock: the zero vector, the field's own parity
    skipped, B    the directions of the macroblock in front, PMV[0][s] as the vectors, field-based, the field's own parity
The predictors are followed here as 7.6.3 says - field-based: from PMV[0][s], PMV[1][s] follows; 16 x 8: vector r from and into
PMV[r][s]; dual prime: PMV[1][0] follows; nothing halved - so that a wrong form of them can be followed too: what such a decoder would
read where the writer wrote the differences to the right predictors (f_code 1: the cases keep every sum in range).

frames(log, wrong) takes the classic wrong forms by name, one at a time; a case of tests/fld_cases.py shows for each that it changes
the frames:
    second_reads_previous      the second field of an anchor frame reads the frame in front instead of the first field of its own frame
    select_inverted            motion_vertical_field_select 0 read as the bottom field
    weave_swapped              the top field woven into the odd lines
    bottom_first_as_top_first  the first field of a pair woven into the even lines whatever its parity
    lower_uses_vector_0        the lower 16 x 8 predicted by vector 0 and its select
    chroma_split_at_8          the chroma of a 16 x 8 macroblock split at line 8: all of it by vector 0
    vector_1_from_pmv_0        the second vector of a 16 x 8 macroblock predicted from PMV[0][s]
    pmv_1_not_copied           PMV[1][s] left alone by a field-based vector
    vertical_halved            the vertical predictor halved going in and doubled coming out, as for field vectors of frame pictures
    e_wrong_sign               + 1 in a top field, - 1 in a bottom field
    e_left_out                 no e
    h_floor                    a >> 1 in the place of h
    skipped_p_opposite_parity  a P field's skipped macroblock reads the other parity
    skipped_b_zero_vector      a B field's skipped macroblock takes the zero vector
    two_stage_mean             the four-sample mean as two rounded two-sample means"""
import numpy as np

import arith_ref as R

WRONG = ("second_reads_previous", "select_inverted", "weave_swapped", "bottom_first_as_top_first", "lower_uses_vector_0", "chroma_split_at_8", "vector_1_from_pmv_0",
         "pmv_1_not_copied", "vertical_halved", "e_wrong_sign", "e_left_out", "h_floor", "skipped_p_opposite_parity", "skipped_b_zero_vector", "two_stage_mean")


def toward_zero(a):
    return -((-a) // 2) if a < 0 else a // 2


def block(plane, x0, y0, v, w, h, wrong=()):
    """a w x h prediction at (x0, y0) of a field plane by the vector v in half samples (7.6.4)"""
    ix, iy, hx, hy = v[0] >> 1, v[1] >> 1, v[0] & 1, v[1] & 1
    assert x0 + ix >= 0 and y0 + iy >= 0 and x0 + ix + w - 1 + hx < plane.shape[1] and y0 + iy + h - 1 + hy < plane.shape[0], "a vector reads outside its field"
    a = plane[y0 + iy:y0 + iy + h + hy, x0 + ix:x0 + ix + w + hx]
    if hx and hy:
        if "two_stage_mean" in wrong:
            return (((a[:-1, :-1] + a[:-1, 1:] + 1) >> 1) + ((a[1:, :-1] + a[1:, 1:] + 1) >> 1) + 1) >> 1
        return (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:] + 2) >> 2
    if hx:
        return (a[:, :-1] + a[:, 1:] + 1) >> 1
    if hy:
        return (a[:-1] + a[1:] + 1) >> 1
    return a


def one(field, col, row, halves, wrong=()):
    """a prediction from halves = [(field planes, vector)] * 2, the upper and the lower 16 x 8 -> [16 x 16, 8 x 8, 8 x 8]"""
    out = []
    for p, n in ((0, 16), (1, 8), (2, 8)):
        parts = []
        for r, (planes, v) in enumerate(halves):
            if p and "chroma_split_at_8" in wrong:
                planes, v = halves[0]
            assert planes is not None, "a select names a field that is not there"
            cv = v if p == 0 else (toward_zero(v[0]), toward_zero(v[1]))
            parts.append(block(planes[p], n * col, n * row + (n // 2) * r, cv, n, n // 2, wrong))
        out.append(np.vstack(parts))
    return out


def reread(mbs, ptype, wrong=()):
    """the macroblocks of one slice with the vectors a decoder reads that follows the predictors in a wrong form: the writer wrote every
    vector as its difference to the right predictor.  A skipped macroblock of a B field gets the predictors as the decoder holds them"""
    zero = lambda: [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]             # PMV[r][s]
    good, seen = zero(), zero()
    out, front = [], None

    def read(v, r, s, base_r):
        """vector v written against good[r][s], read against seen[base_r][s]; both predictors move"""
        delta = (v[0] - good[r][s][0], v[1] - good[r][s][1])
        good[r][s] = list(v)
        base = list(seen[base_r][s])
        if "vertical_halved" in wrong:
            base[1] >>= 1
        got = (base[0] + delta[0], base[1] + delta[1])
        assert got == tuple(v) or all(-16 <= c <= 15 for c in got), "the case keeps every sum in the range of f_code 1"      # (a vector read right is the writer's, at any f_code)
        seen[r][s] = [got[0], 2 * got[1]] if "vertical_halved" in wrong else list(got)
        return got

    for mb in mbs:
        mb = dict(mb)
        if mb["skip"]:
            if ptype == 2:
                good, seen = zero(), zero()
            else:
                mb["fwd"] = tuple(seen[0][0]) if front[0] else None
                mb["bwd"] = tuple(seen[0][1]) if front[1] else None
        elif mb["intra"] or mb["nomc"]:
            good, seen = zero(), zero()
            front = None if mb["intra"] else (1, 0)
        else:
            for s, name in ((0, "fwd"), (1, "bwd")):
                v = mb[name]
                if v is None:
                    continue
                if mb["motion"] == "field":
                    mb[name] = (v[0], read(v[1], 0, s, 0))
                    good[1][s] = list(good[0][s])
                    if "pmv_1_not_copied" not in wrong:
                        seen[1][s] = list(seen[0][s])
                elif mb["motion"] == "16x8":
                    first = read(v[0][1], 0, s, 0)
                    mb[name] = ((v[0][0], first), (v[1][0], read(v[1][1], 1, s, 0 if "vector_1_from_pmv_0" in wrong else 1)))
                else:
                    mb[name] = (read(v[0], 0, 0, 0), v[1])
                    good[1][0], seen[1][0] = list(good[0][0]), list(seen[0][0])
            front = (1, 0) if ptype == 2 else (int(mb["fwd"] is not None), int(mb["bwd"] is not None))
        out.append(mb)
    return out


def frames(log, wrong=()):
    """the frames of the log in display order, each (Y, U, V) of uint8, cropped to w x h"""
    wrong = (wrong,) if isinstance(wrong, str) else tuple(wrong)
    assert all(m in WRONG for m in wrong), wrong
    w, h, mbw, rows = log["w"], log["h"], log["mbw"], log["rows"]
    new_field = lambda: [np.zeros((16 * rows, 16 * mbw), np.int64), np.zeros((8 * rows, 8 * mbw), np.int64), np.zeros((8 * rows, 8 * mbw), np.int64)]
    done = []                                                       # frames: dict(type, fields=[top, bottom], first parity)
    anchors = []                                                    # the last two anchor frames
    cur = None
    half = lambda a: a >> 1 if "h_floor" in wrong else (a + (a > 0)) >> 1
    for pic in log["pictures"]:
        par, ptype = pic["ps"] - 1, pic["type"]
        second = cur is not None
        if not second:
            cur = dict(type=ptype, fields=[None, None], first=par)
        mine = new_field()
        # the field of parity q in direction s
        if ptype == 3:
            refs = [[anchors[-2]["fields"][q] for q in (0, 1)], [anchors[-1]["fields"][q] for q in (0, 1)]]
        else:
            last = anchors[-1]["fields"] if anchors else [None, None]
            refs = [list(last), [None, None]]
            if second and "second_reads_previous" not in wrong:
                refs[0][1 - par] = cur["fields"][1 - par]
        pick = lambda s, sel: refs[s][sel ^ 1 if "select_inverted" in wrong else sel]
        mbs = []
        for row in range(rows):
            mbs += reread([m for m in pic["mbs"] if m["row"] == row], ptype, wrong)
        for mb, res in zip(mbs, R.residuals(pic)):
            col, row = mb["col"], mb["row"]
            if mb["intra"]:
                pred = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
            elif mb["skip"] and ptype == 2:
                pred = one(None, col, row, [(refs[0][par ^ 1 if "skipped_p_opposite_parity" in wrong else par], (0, 0))] * 2, wrong)
            elif mb["nomc"]:
                pred = one(None, col, row, [(refs[0][par], (0, 0))] * 2, wrong)
            elif mb["skip"]:
                parts = [one(None, col, row, [(refs[s][par], (0, 0) if "skipped_b_zero_vector" in wrong else v)] * 2, wrong)
                         for s, v in ((0, mb["fwd"]), (1, mb["bwd"])) if v is not None]
                pred = parts[0] if len(parts) == 1 else [(a + c + 1) >> 1 for a, c in zip(*parts)]
            elif mb["motion"] == "dual":
                (vx, vy), (d0, d1) = mb["fwd"]
                e = 0 if "e_left_out" in wrong else (1 if par else -1) * (-1 if "e_wrong_sign" in wrong else 1)
                other = mb.get("derived") or (half(vx) + d0, half(vy) + d1 + e)      # derived: tests/vec_ref.py's, in the place of the line above
                parts = [one(None, col, row, [(refs[0][par], (vx, vy))] * 2, wrong), one(None, col, row, [(refs[0][1 - par], other)] * 2, wrong)]
                pred = [(a + c + 1) >> 1 for a, c in zip(*parts)]
            else:
                parts = []
                for s, v in ((0, mb["fwd"]), (1, mb["bwd"])):
                    if v is None:
                        continue
                    if mb["motion"] == "field":
                        halves = [(pick(s, v[0]), v[1])] * 2
                    else:
                        halves = [(pick(s, v[0][0]), v[0][1]), (pick(s, v[1][0]), v[1][1])]
                        if "lower_uses_vector_0" in wrong:
                            halves[1] = halves[0]
                    parts.append(one(None, col, row, halves, wrong))
                pred = parts[0] if len(parts) == 1 else [(a + c + 1) >> 1 for a, c in zip(*parts)]
            off = 0                                                 # (an intra block's residual carries its DC: arith_ref.residuals)
            for b in range(6):
                if b >= 4:
                    mine[b - 3][8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pred[b - 3] + off + res[b], 0, 255)
                else:
                    oy, ox = 8 * (b >> 1), 8 * (b & 1)
                    mine[0][16 * row + oy:16 * row + oy + 8, 16 * col + ox:16 * col + ox + 8] = np.clip(pred[0][oy:oy + 8, ox:ox + 8] + off + res[b], 0, 255)
        cur["fields"][par] = mine
        if second:
            done.append(cur)
            if cur["type"] != 3:
                anchors = (anchors + [cur])[-2:]
            cur = None
    assert cur is None, "the log ends with a whole frame"
    # display order: a B frame where it is decoded, an anchor frame in front of the next anchor frame, or at the end
    order, held = [], None
    for f in done:
        if f["type"] == 3:
            order.append(f)
        else:
            if held is not None:
                order.append(held)
            held = f
    if held is not None:
        order.append(held)
    out = []
    ch, cw = (h + 1) // 2, (w + 1) // 2
    for f in order:
        top, bottom = f["fields"]
        if "weave_swapped" in wrong:
            top, bottom = bottom, top
        if "bottom_first_as_top_first" in wrong and f["first"] == 1:
            top, bottom = bottom, top
        planes = []
        for p in range(3):
            woven = np.zeros((2 * top[p].shape[0], top[p].shape[1]), np.int64)
            woven[0::2], woven[1::2] = top[p], bottom[p]
            planes.append(woven)
        out.append((planes[0][:h, :w].astype(np.uint8), planes[1][:ch, :cw].astype(np.uint8), planes[2][:ch, :cw].astype(np.uint8)))
    return out
