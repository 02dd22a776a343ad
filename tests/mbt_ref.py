"""A second implementation of dual-prime prediction for the decoder's tests, in numpy, in the manner of tests/arith_ref.py (whose
inverse quantisation, inverse DCT and half-sample prediction it uses): it never parses a stream - mbt_cases.build() hands it the
macroblocks it wrote, with absolute vectors - and computes the frames.  A P picture's macroblock with motion="dual" carries
fwd=((vx, vy), (d0, d1)), the vector (vertical in half samples of the field) and the dmvector; its picture carries tff.

    h(a) = (a + (a > 0)) >> 1                       division by 2 to the nearest integer, halves away from zero
    top_field_first 1:  T = (h(vx) + d0, h(vy) + d1 - 1)      B = (h(3 vx) + d0, h(3 vy) + d1 + 1)
    top_field_first 0:  T = (h(3 vx) + d0, h(3 vy) + d1 - 1)  B = (h(vx) + d0, h(vy) + d1 + 1)
    top-field lines    = (top field by (vx, vy) + bottom field by T + 1) >> 1
    bottom-field lines = (bottom field by (vx, vy) + top field by B + 1) >> 1
each a 16 x 8 field prediction with half-sample interpolation, every vector halved toward zero on its own for chroma.

frames(log, wrong) takes the classic wrong forms by name, one at a time; a case of tests/mbt_cases.py shows for each that it changes
the frames:
    half_floor          a >> 1 in the place of h (differs for positive odd a)
    half_up             (a + 1) >> 1 in the place of h (differs for negative odd a)
    factors_swapped     the factors 1 and 3 changed places
    tff_ignored         top_field_first taken as 1
    e_swapped           + 1 with T and - 1 with B
    e_none              the - 1 and + 1 left out
    selects_swapped     the derived vectors read the field of the same parity, the vector itself the opposite one
    mean_trunc          (a + b) >> 1
    chroma_joint        one chroma halving: the chroma derived vectors are derived from the halved vector, not halved on their own
    pmv1_kept           PMV[1][0] not set by a dual-prime macroblock: the bottom-field vector of a field-based macroblock behind it is
                        read from the predictor that was there before"""
import numpy as np

import arith_ref as R

WRONG = ("half_floor", "half_up", "factors_swapped", "tff_ignored", "e_swapped", "e_none", "selects_swapped", "mean_trunc", "chroma_joint", "pmv1_kept")


def half(a, wrong=()):
    if "half_floor" in wrong:
        return a >> 1
    if "half_up" in wrong:
        return (a + 1) >> 1
    return (a + (a > 0)) >> 1


def derived(v, dmv, tff, wrong=()):
    """-> (T, B): the vectors that read the field of the opposite parity for the top-field and the bottom-field lines"""
    ft, fb = (1, 3) if tff or "tff_ignored" in wrong else (3, 1)
    if "factors_swapped" in wrong:
        ft, fb = fb, ft
    et, eb = (1, -1) if "e_swapped" in wrong else (0, 0) if "e_none" in wrong else (-1, 1)
    return ((half(ft * v[0], wrong) + dmv[0], half(ft * v[1], wrong) + dmv[1] + et),
            (half(fb * v[0], wrong) + dmv[0], half(fb * v[1], wrong) + dmv[1] + eb))


def _field_block(plane, sel, x0, y0, v, w, h):
    """a w x h prediction from field `sel` of the plane at (x0, y0) of the field by the vector v in half samples (7.6.4)"""
    f = plane[sel::2]
    ix, iy, hx, hy = v[0] >> 1, v[1] >> 1, v[0] & 1, v[1] & 1
    assert x0 + ix >= 0 and y0 + iy >= 0 and x0 + ix + w - 1 + hx < f.shape[1] and y0 + iy + h - 1 + hy < f.shape[0], "a vector reads outside its field"
    a = f[y0 + iy:y0 + iy + h + hy, x0 + ix:x0 + ix + w + hx]
    if hx and hy:
        return (a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:] + 2) >> 2
    if hx:
        return (a[:, :-1] + a[:, 1:] + 1) >> 1
    if hy:
        return (a[:-1] + a[1:] + 1) >> 1
    return a


def toward_zero(a):
    return -((-a) // 2) if a < 0 else a // 2


def dual(ref, col, row, v, dmv, tff, wrong=(), given=None):
    """the prediction of a dual-prime macroblock -> [16 x 16, 8 x 8, 8 x 8]; given: (T, B) from tests/vec_ref.py in the place of derived()"""
    t, b = given if given is not None else derived(v, dmv, tff, wrong)
    out = []
    for p, n in ((0, 16), (1, 8), (2, 8)):
        same, opp = [v, v], [t, b]
        if p:
            same = [(toward_zero(v[0]), toward_zero(v[1]))] * 2
            opp = [(toward_zero(x), toward_zero(y)) for x, y in opp]
            if "chroma_joint" in wrong:
                opp = list(derived(same[0], dmv, tff, wrong))
        blk = np.zeros((n, n), np.int64)
        for r in (0, 1):                                            # the lines of parity r
            s0, s1 = (r, 1 - r) if "selects_swapped" not in wrong else (1 - r, r)
            a = _field_block(ref[p], s0, n * col, (n // 2) * row, same[r], n, n // 2)
            c = _field_block(ref[p], s1, n * col, (n // 2) * row, opp[r], n, n // 2)
            blk[r::2] = (a + c + (0 if "mean_trunc" in wrong else 1)) >> 1
        out.append(blk)
    return out


def _pmv1_kept(mbs):
    """the macroblocks of a P picture as a decoder reads them that leaves PMV[1][0] alone in a dual-prime macroblock: the bottom-field
    vector of a field-based macroblock is off by the difference of the two predictors (f_code 1: the tests keep every sum in range)"""
    out = []
    good = wrong = (0, 0)                                           # PMV[1][0], vertical in frame units
    for mb in mbs:
        mb = dict(mb)
        if mb["col"] == 0 or mb["intra"] or mb.get("fwd") is None or mb.get("nomc"):
            good = wrong = (0, 0)
        if not mb["intra"] and mb.get("fwd") is not None and not mb.get("nomc"):
            motion = mb.get("motion", "frame")
            if motion == "dual":
                (vx, vy), _ = mb["fwd"]
                good = (vx, 2 * vy)
            elif motion == "frame":
                good = wrong = tuple(mb["fwd"])
            else:
                (s0, v0), (s1, v1) = mb["fwd"]
                seen = (v1[0] - good[0] + wrong[0], v1[1] - (good[1] >> 1) + (wrong[1] >> 1))
                assert all(-16 <= c <= 15 for c in seen)
                mb["fwd"] = ((s0, v0), (s1, seen))
                good, wrong = (v1[0], 2 * v1[1]), (seen[0], 2 * seen[1])
        out.append(mb)
    return out


def frames(log, wrong=()):
    """arith_ref.frames with dual prime: the frames of the log in display order, each (Y, U, V) of uint8, cropped to w x h"""
    wrong = (wrong,) if isinstance(wrong, str) else tuple(wrong)
    assert all(m in WRONG for m in wrong), wrong
    w, h, mbw, mbh = log["w"], log["h"], log["mbw"], log["rows"]
    anchors, coded = [], []
    for pic in log["pictures"]:
        planes = [np.zeros((16 * mbh, 16 * mbw), np.int64), np.zeros((8 * mbh, 8 * mbw), np.int64), np.zeros((8 * mbh, 8 * mbw), np.int64)]
        mbs = _pmv1_kept(pic["mbs"]) if "pmv1_kept" in wrong and pic["type"] == 2 else pic["mbs"]
        for mb, res in zip(mbs, R.residuals(pic)):
            if not mb["intra"] and mb.get("motion") == "dual":
                pred = dual(anchors[-1], mb["col"], mb["row"], mb["fwd"][0], mb["fwd"][1], pic.get("tff", 1), wrong, mb.get("derived"))
            else:
                pred = R.predict(mb, pic["type"], anchors)
            col, row = mb["col"], mb["row"]
            for b in range(6):
                if b >= 4:
                    planes[b - 3][8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pred[b - 3] + res[b], 0, 255)
                elif mb.get("dct", 0):
                    y0, x0 = 16 * row + (b >> 1), 16 * col + 8 * (b & 1)
                    planes[0][y0:y0 + 16:2, x0:x0 + 8] = np.clip(pred[0][(b >> 1)::2, 8 * (b & 1):8 * (b & 1) + 8] + res[b], 0, 255)
                else:
                    oy, ox = 8 * (b >> 1), 8 * (b & 1)
                    planes[0][16 * row + oy:16 * row + oy + 8, 16 * col + ox:16 * col + ox + 8] = np.clip(pred[0][oy:oy + 8, ox:ox + 8] + res[b], 0, 255)
        coded.append(planes)
        if pic["type"] != 3:
            anchors = (anchors + [planes])[-2:]
    assert all(p["type"] != 3 for p in log["pictures"]), "dual prime lives in P pictures: the tests' streams have no B pictures"
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return [(c[0][:h, :w].astype(np.uint8), c[1][:ch, :cw].astype(np.uint8), c[2][:ch, :cw].astype(np.uint8)) for c in coded]
