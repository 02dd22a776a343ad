"""A plain reference of the main syntax's arithmetic, written from the text of ISO/IEC 13818-2 clauses 7.4 to 7.6 and not from
decoder.py: inverse quantisation as integer formulas (7.4.1, 7.4.2), saturation (7.4.3), mismatch control (7.4.4), the Chen-Wang
inverse DCT of ISO mode restated in int64 (with the wrap of 32-bit integers where a shift can see it, or with none: idct's wrap32),
frame and field prediction with half-sample rounding (7.6.4), the mean of two predictions (7.6.7.1), chroma vectors by division
toward zero (7.6.3.7) and the final clip (7.6.8).  It never parses a stream: it takes a log of what the writer was given
(arith_cases.build makes the stream and the log from one description) -

   log      dict(w, h, mbw, rows, pictures=[...]) with the pictures in coded order
   picture  dict(type=1 | 2 | 3, prec, qst, scan=[raster index of scan position 0 .. 63], matrices=(intra, non-intra) in raster
            order, mbs=[...]) with every macroblock of the picture, row by row (no macroblock is skipped)
   mb       dict(row, col, first=starts a slice, intra, fwd, bwd, motion="frame" | "field", dct=0 | 1, cbp, qcode, blocks=[(the 64
            levels in scan order, the DC differential)] for the coded blocks in order); a frame vector is (x, y), a field-based
            direction ((select, (x, y)), (select, (x, y)))

- and returns the frames in display order, cropped to w x h.  The intra DC is the standard's: predictors reset to 2 ** (7 + precision),
F[0][0] = intra_dc_mult * QF[0][0], no prediction of 128 (decoder.py keeps the DC relative to the reset value and predicts 128).
Illegal DC predictors are out of scope.

`mut` names switches, each turning one rule into its classic wrong form (MUTANTS): tests/test_arith_cases.py proves that every case
of tests/arith_cases.py is sensitive to the rule it is named after by throwing the switch.

idct_real is the other yardstick: the float64 separable inverse DCT, rounded to nearest, clipped to -256 .. 255 (Annex A)."""
import numpy as np

MUTANTS = ("dq_floor", "sign_dropped", "sign_plus1", "prod16", "prod24", "scale_linear", "sat_symmetric", "sat_none", "mm_none", "mm_always",
           "mm_before_sat", "mm_no_dc", "dc_mult_wrong", "dc_offset_twice", "weight_by_scan", "matrices_swapped", "row18", "clip255", "no_final_clip",
           "clip_high_only", "clip_low_only", "hp_trunc", "hp_plus1", "hp_two_stage", "chroma_floor", "b_joint", "b_trunc", "b_swapped",
           "field_vert_frame_row", "field_chroma_floor", "field_dct_frame_map")

# table 7-6, q_scale_type 1
NONLINEAR = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112)


def zigzag():
    """figure 7-2 by its rule: the anti-diagonals in turn, odd ones downwards, even ones upwards -> raster index of every scan position"""
    out = []
    for s in range(15):
        us = range(max(0, s - 7), min(7, s) + 1)
        for u in (reversed(us) if s & 1 else us):
            out.append(8 * (s - u) + u)
    return out


def quantiser_scale(code, qst, mut=()):
    return NONLINEAR[code - 1] if qst and "scale_linear" not in mut else 2 * code


def _wrap(v, bits):
    return ((v + (1 << (bits - 1))) & ((1 << bits) - 1)) - (1 << (bits - 1))


def _toward_zero(num, den):
    return np.sign(num) * (np.abs(num) // den)


def dequant_ac(q, w, intra, scale, mut=()):
    """7.4.2.3: F'' = (2 QF + k) W quantiser_scale / 32 with "/" toward zero, k = 0 for intra blocks and Sign(QF) else - any shapes
    that broadcast, before saturation"""
    q, w, scale = np.asarray(q, np.int64), np.asarray(w, np.int64), np.asarray(scale, np.int64)
    k = np.where(np.asarray(intra, bool), 0, np.sign(q))
    if "sign_dropped" in mut:
        k = 0 * k
    if "sign_plus1" in mut:
        k = np.where(np.asarray(intra, bool), 0, (q != 0).astype(np.int64))
    num = (2 * q + k) * w * scale
    if "prod16" in mut:
        num = _wrap(num, 16)
    if "prod24" in mut:
        num = _wrap(num, 24)
    return num >> 5 if "dq_floor" in mut else _toward_zero(num, 32)


def saturate(F, mut=()):
    """7.4.3"""
    if "sat_none" in mut:
        return F
    return np.clip(F, -2047 if "sat_symmetric" in mut else -2048, 2047)


def dc_mult(prec, mut=()):
    return 1 << prec if "dc_mult_wrong" in mut else 8 >> prec


def mismatch(F, mut=(), before=None, intra=None):
    """7.4.4 on F[n, 64]: where the sum is even, F[7][7] moves by one: an odd one down, an even one up"""
    F = F.copy()
    if "mm_none" in mut:
        return F
    s = (before if "mm_before_sat" in mut else F).sum(axis=1)
    if "mm_no_dc" in mut:
        s = s - np.where(intra, F[:, 0], 0)
    even = (s & 1) == 0
    if "mm_always" in mut:
        even = np.ones_like(even)
    F[:, 63] += np.where(even, np.where(F[:, 63] & 1, -1, 1), 0)
    return F


def coefficients(levels, scan, intra, dc, W, scale, mult, mut=()):
    """levels[n, 64] in scan order, intra[n], dc[n] (QF[0][0] of the intra blocks), W[n, 64] in raster order, scale[n] -> F[n, 64]"""
    levels = np.asarray(levels, np.int64).reshape(-1, 64)
    n = len(levels)
    intra = np.asarray(intra, bool).reshape(n)
    scan = np.asarray(scan)
    q = np.zeros((n, 64), np.int64)
    q[:, scan] = levels                                         # 7.3: QF[v][u] = QFS[scan[v][u]]
    W = np.asarray(W, np.int64).reshape(n, 64)
    if "weight_by_scan" in mut:
        Ws = np.zeros_like(W)
        Ws[:, scan] = W[:, np.arange(64)]
        W = Ws
    F = dequant_ac(q, W, intra[:, None], np.asarray(scale, np.int64).reshape(n, 1), mut)
    F[:, 0] = np.where(intra, mult * np.asarray(dc, np.int64).reshape(n), F[:, 0])
    before = F
    F = saturate(F, mut)
    return mismatch(F, mut, before, intra)


W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565       # 2048 sqrt(2) cos(k pi / 16)


def _cw(a, row, wrap32):
    """one pass of the Chen-Wang inverse DCT over the last axis; row pass: 11 fraction bits in, 8 out; column pass: 8 in, 14 out.
    wrap32: what is shifted right is first taken modulo 2 ** 32 as a signed number - the same int64 arithmetic gives what a program
    with 32-bit integers gives (sums and products commute with the wrap; only a shift sees it)"""
    s = (lambda v: _wrap(v, 32)) if wrap32 else (lambda v: v)
    a = [a[..., k] for k in range(8)]
    if row:
        x0, x1, sh, r = (a[0] << 11) + 128, a[4] << 11, 0, 0
    else:
        x0, x1, sh, r = (a[0] << 8) + 8192, a[4] << 8, 3, 4
    x2, x3, x4, x5, x6, x7 = a[6], a[2], a[1], a[7], a[5], a[3]
    x8 = W7 * (x4 + x5) + r
    x4 = s(x8 + (W1 - W7) * x4) >> sh
    x5 = s(x8 - (W1 + W7) * x5) >> sh
    x8 = W3 * (x6 + x7) + r
    x6 = s(x8 - (W3 - W5) * x6) >> sh
    x7 = s(x8 - (W3 + W5) * x7) >> sh
    x8 = x0 + x1
    x0 = x0 - x1
    x1 = W6 * (x3 + x2) + r
    x2 = s(x1 - (W2 + W6) * x2) >> sh
    x3 = s(x1 + (W2 - W6) * x3) >> sh
    x1 = x4 + x6
    x4 = x4 - x6
    x6 = x5 + x7
    x5 = x5 - x7
    x7 = x8 + x3
    x8 = x8 - x3
    x3 = x0 + x2
    x0 = x0 - x2
    x2 = s(181 * (x4 + x5) + 128) >> 8
    x4 = s(181 * (x4 - x5) + 128) >> 8
    out = np.stack([x7 + x1, x3 + x2, x0 + x4, x8 + x6, x8 - x6, x0 - x4, x3 - x2, x7 - x1], axis=-1)
    return s(out) >> (8 if row else 14)


def idct(F, mut=(), wrap32=True):
    """F[n, 64] -> f[n, 8, 8]: rows, then columns, clipped to -256 .. 255 (7.5: the saturation of f).  wrap32=False: nothing wraps.
    The two differ only on blocks whose real inverse transform leaves the range Annex A gives a decoder figures for by far"""
    x = _cw(np.asarray(F, np.int64).reshape(-1, 8, 8), True, wrap32)
    if "row18" in mut:
        x = _wrap(x, 18)
    x = np.swapaxes(_cw(np.swapaxes(x, 1, 2), False, wrap32), 1, 2)
    return np.clip(x, -255 if "clip255" in mut else -256, 255)


def _basis():
    k = np.arange(8)
    C = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) / 2          # C[u][x]
    C[0] /= np.sqrt(2)
    return C


def idct_real(F):
    """the float64 separable inverse DCT of F[n, 64], rounded to nearest, clipped to -256 .. 255 -> int64 [n, 8, 8]"""
    C = _basis()
    f = np.einsum("ux,nuv,vy->nxy", C, np.asarray(F, np.float64).reshape(-1, 8, 8), C)       # f[y][x] = sum C[v][y] F[v][u] C[u][x]
    return np.clip(np.rint(f), -256, 255).astype(np.int64)


def fdct_real(f):
    """the float64 forward DCT of f[n, 8, 8] -> [n, 64], not rounded"""
    C = _basis()
    return np.einsum("ux,nxy,vy->nuv", C, np.asarray(f, np.float64), C).reshape(-1, 64)


# ---- prediction ----
def _halve(v, floor):
    return v >> 1 if floor else (-((-v) // 2) if v < 0 else v // 2)


def _numerator(plane, rows, cols, hx, hy, down):
    """the prediction's four-fold: 4 a, 2 (a + b), 2 (a + c) or a + b + c + d (7.6.4), with the parts for the wrong roundings"""
    assert rows[0] >= 0 and cols[0] >= 0 and rows[-1] + (down if hy else 0) < plane.shape[0] and cols[-1] + hx < plane.shape[1], "a vector reads outside"
    a = plane[np.ix_(rows, cols)]
    b = plane[np.ix_(rows, cols + 1)] if hx else a
    c = plane[np.ix_(rows + down, cols)] if hy else a
    if hx and hy:
        return a, b, c, plane[np.ix_(rows + down, cols + 1)]
    if hx:
        return a, b, a, b
    if hy:
        return a, c, a, c
    return a, a, a, a


def _rounded(parts, hx, hy, mut):
    a, b, c, d = parts
    if hx and hy:
        if "hp_two_stage" in mut:
            return (((a + b + 1) >> 1) + ((c + d + 1) >> 1) + 1) >> 1
        return (a + b + c + d + (0 if "hp_trunc" in mut else 1 if "hp_plus1" in mut else 2)) >> 2
    if hx or hy:
        return (a + b + (0 if "hp_trunc" in mut else 1)) >> 1
    return a


def _one(ref, col, row, vec, mut, field=None):
    """one direction's prediction of a macroblock -> ([16 x 16, 8 x 8, 8 x 8] rounded, the same as numerators over 4).  field: None for
    frame prediction with vec = (x, y), else vec = ((select, (x, y)), (select, (x, y)))"""
    out, num = [], []
    for p, n in ((0, 16), (1, 8), (2, 8)):
        blk, nm = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
        for r in ((0, 1) if field else (None,)):
            sel, v = vec[r] if field else (0, vec)
            if p:
                floor = ("field_chroma_floor" if field else "chroma_floor") in mut
                v = (_halve(v[0], floor), _halve(v[1], floor))
            ix, iy, hx, hy = v[0] >> 1, v[1] >> 1, v[0] & 1, v[1] & 1
            cols = n * col + ix + np.arange(n)
            if field:                                           # the field `sel` of the reference: frame rows sel, sel + 2, ...
                rows = sel + 2 * ((n // 2) * row + iy + np.arange(n // 2))
                down = 1 if "field_vert_frame_row" in mut else 2
                assert rows[-1] + (2 if hy else 0) < ref[p].shape[0]
            else:
                rows, down = n * row + iy + np.arange(n), 1
            parts = _numerator(ref[p], rows, cols, hx, hy, down)
            dst = slice(r, None, 2) if field else slice(None)
            blk[dst] = _rounded(parts, hx, hy, mut)
            nm[dst] = sum(parts)
        out.append(blk)
        num.append(nm)
    return out, num


def predict(mb, ptype, anchors, mut=()):
    if mb["intra"]:
        off = 128 if "dc_offset_twice" in mut else 0
        return [np.full((16, 16), off, np.int64), np.full((8, 8), off, np.int64), np.full((8, 8), off, np.int64)]
    refs = [anchors[-1], None] if ptype == 2 else [anchors[-2], anchors[-1]]
    if "b_swapped" in mut and ptype == 3:
        refs = refs[::-1]
    field = mb.get("motion", "frame") == "field"
    got = [_one(refs[s], mb["col"], mb["row"], v, mut, field) for s, v in enumerate((mb.get("fwd"), mb.get("bwd"))) if v is not None]
    assert got, "a predicted macroblock has a direction"
    if len(got) == 1:
        return got[0][0]
    if "b_joint" in mut:
        return [(f + b + 4) >> 3 for f, b in zip(got[0][1], got[1][1])]
    return [(f + b + (0 if "b_trunc" in mut else 1)) >> 1 for f, b in zip(got[0][0], got[1][0])]


def _final(v, mut):
    """7.6.8: saturation to 0 .. 255"""
    if "no_final_clip" in mut:
        return v & 255
    if "clip_high_only" in mut:
        return np.minimum(v, 255) & 255
    if "clip_low_only" in mut:
        return np.maximum(v, 0) & 255
    return np.clip(v, 0, 255)


def residuals(pic, mut=(), wrap32=True):
    """every coded block of the picture in one go -> per macroblock a list of six 8 x 8 arrays (zeros where the pattern has none)"""
    prec = pic["prec"]
    levels, intra, dc, W, scale, where = [], [], [], [], [], []
    pred = [0, 0, 0]
    mats = pic["matrices"][::-1] if "matrices_swapped" in mut else pic["matrices"]
    for k, mb in enumerate(pic["mbs"]):
        if mb["first"] or not mb["intra"]:
            pred = [1 << (7 + prec)] * 3                        # 7.2.1
        blocks = iter(mb["blocks"])
        for b in range(6):
            if not (mb["cbp"] >> (5 - b)) & 1:
                continue
            lv, diff = next(blocks)
            comp = 0 if b < 4 else b - 3
            if mb["intra"]:
                pred[comp] += diff
                assert 0 <= pred[comp] < 1 << (8 + prec), "an illegal DC predictor is out of scope"
            levels.append(lv)
            intra.append(mb["intra"])
            dc.append(pred[comp] if mb["intra"] else 0)
            W.append(mats[0] if mb["intra"] else mats[1])
            scale.append(quantiser_scale(mb["qcode"], pic["qst"], mut))
            where.append((k, b))
    out = [[np.zeros((8, 8), np.int64)] * 6 for _ in pic["mbs"]]
    if levels:
        f = idct(coefficients(levels, pic["scan"], intra, dc, W, scale, dc_mult(prec, mut), mut), mut, wrap32)
        for (k, b), r in zip(where, f):
            out[k] = list(out[k])
            out[k][b] = r
    return out


def frames(log, mut=(), wrap32=True):
    """the frames of the log in display order, each (Y, U, V) of uint8, cropped to w x h"""
    mut = (mut,) if isinstance(mut, str) else tuple(mut)
    assert all(m in MUTANTS for m in mut), mut
    w, h, mbw, mbh = log["w"], log["h"], log["mbw"], log["rows"]
    anchors, coded = [], []
    for pic in log["pictures"]:
        planes = [np.zeros((16 * mbh, 16 * mbw), np.int64), np.zeros((8 * mbh, 8 * mbw), np.int64), np.zeros((8 * mbh, 8 * mbw), np.int64)]
        assert len(pic["mbs"]) == mbw * mbh
        for mb, res in zip(pic["mbs"], residuals(pic, mut, wrap32)):
            pred = predict(mb, pic["type"], anchors, mut)
            col, row = mb["col"], mb["row"]
            for b in range(6):
                if b >= 4:
                    planes[b - 3][8 * row:8 * row + 8, 8 * col:8 * col + 8] = _final(pred[b - 3] + res[b], mut)
                elif mb.get("dct", 0) and "field_dct_frame_map" not in mut:      # 6.1.3 figure 6-8: blocks 0 / 1 the top-field lines, 2 / 3 the bottom-field lines
                    y0, x0 = 16 * row + (b >> 1), 16 * col + 8 * (b & 1)
                    planes[0][y0:y0 + 16:2, x0:x0 + 8] = _final(pred[0][(b >> 1)::2, 8 * (b & 1):8 * (b & 1) + 8] + res[b], mut)
                else:
                    oy, ox = 8 * (b >> 1), 8 * (b & 1)
                    planes[0][16 * row + oy:16 * row + oy + 8, 16 * col + ox:16 * col + ox + 8] = _final(pred[0][oy:oy + 8, ox:ox + 8] + res[b], mut)
        coded.append(planes)
        if pic["type"] != 3:
            anchors = (anchors + [planes])[-2:]
    # display order: a B picture goes out when decoded, an anchor when the next anchor arrives or at the end
    order, held = [], None
    for k, pic in enumerate(log["pictures"]):
        if pic["type"] == 3:
            order.append(k)
        else:
            if held is not None:
                order.append(held)
            held = k
    if held is not None:
        order.append(held)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return [(coded[k][0][:h, :w].astype(np.uint8), coded[k][1][:ch, :cw].astype(np.uint8), coded[k][2][:ch, :cw].astype(np.uint8)) for k in order]


def flat(frames_):
    """[n, frame bytes] of I420"""
    return np.stack([np.concatenate([p.reshape(-1) for p in f]) for f in frames_])
