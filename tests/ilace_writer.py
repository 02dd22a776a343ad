"""A writer of MPEG-2 streams of interlaced frame pictures (option "decode_interlaced"; decoder.decode(..., syntax="main",
interlaced=True)), field by field from ISO/IEC 13818-2.  The bit writer, the code tables and the pictures with frame_pred_frame_dct 1
are tests/dec_writer.py's, main_writer.py's and bpic_writer.py's; a picture with frame_pred_frame_dct 0 is written here, of any type:
macroblock_modes() with frame_motion_type and dct_type, field selects, field vectors from the four predictors PMV[r][s] with the
vertical one halved in and doubled out, the predictor resets.  The syntax is typed here from the standard; nothing is shared with
decoder.py.

stream(w, h, pictures, seq=...) -> (bytes, log): the pictures in CODED order.  A sequence with seq["progressive"] = 0 has
2 * ((h + 31) // 32) macroblock rows.  A picture with field=True is written here:
dict(type=1 | 2 | 3, field=True, slices=[...], f_code=(fh, fv, bh, bv), prec=, qst=, alt=, tff=, rff=, ext={...}); a macroblock of it is
dict(kind="intra" | "pred" | "nomc", motion="frame" | "field", dct=0 | 1, fwd=, bwd=, cbp=, quant=, incr=1, blocks=[...]) - a frame
vector is (x, y), a field-based direction ((select, (x, y)), (select, (x, y))) for the top-field and the bottom-field lines, the
vertical component in half samples of the field.  Any other picture goes to main_writer / bpic_writer unchanged.

The log is bpic_writer's with what the tests assert their streams really reach: ilmbs (per macroblock written: picture, type, place,
kind, motion, dct, directions, whether it carries blocks), selects (the pairs of field selects written), resets (predictor resets
that cleared a predictor that was not zero: "slice", "intra", "nomc", "p_skip")."""
import bpic_writer as BW
import dec_cases as D
import dec_writer as W
import main_writer as MW


def mb_rows(h, progressive):
    """6.3.3: the macroblock rows of a frame picture"""
    return (h + 15) // 16 if progressive else 2 * ((h + 31) // 32)


def new_log():
    return dict(BW.new_log(), ilmbs=[], selects=set(), resets=set())


def field_inside(col, row, mv, mbw, mbh):
    """a field vector reads inside its field: luma 16 x 8 at (16 col, 8 row) of 16 mbw x 8 mbh, chroma 8 x 4 with the vector halved
    toward zero"""
    def ok(x0, y0, vx, vy, w, h, W_, H_):
        ix, iy, hx, hy = vx >> 1, vy >> 1, vx & 1, vy & 1
        return x0 + ix >= 0 and y0 + iy >= 0 and x0 + ix + w - 1 + hx < W_ and y0 + iy + h - 1 + hy < H_
    return ok(16 * col, 8 * row, mv[0], mv[1], 16, 8, 16 * mbw, 8 * mbh) and \
        ok(8 * col, 4 * row, int(mv[0] / 2), int(mv[1] / 2), 8, 4, 8 * mbw, 4 * mbh)


def frame_inside(col, row, mv, mbw, mbh):
    return W.inside(col, row, tuple(mv), mbw, mbh)


def _nonzero(pmv):
    return any(c for r in pmv for s in r for c in s)


def il_picture_units(n, pic, mbw, mbh, L, strict=True):
    ptype = pic["type"]
    f_code, prec, qst, alt = pic.get("f_code", (1, 1, 1, 1)), pic.get("prec", 2), pic.get("qst", 0), pic.get("alt", 0)
    out = []
    w = D._Writer()
    for value, width in ((0x00000100, 32), (n & 1023, 10), (ptype, 3), (0xFFFF, 16)) + (((0, 1), (7, 3)) if ptype in (2, 3) else ()) + \
            (((0, 1), (7, 3)) if ptype == 3 else ()) + ((0, 1),):
        w.put(value, width)
    out.append(("picture", w.bytes()))
    w = D._Writer()
    fields = dict(picture_structure=3, frame_pred_frame_dct=0, concealment=0, intra_vlc_format=0, progressive_frame=0)
    fields.update(pic.get("ext", {}))
    said = f_code if ptype == 3 else (tuple(f_code[:2]) if ptype == 2 else (15, 15)) + (15, 15)
    for value, width in ((0x000001B5, 32), (8, 4), (said[0], 4), (said[1], 4), (said[2], 4), (said[3], 4), (prec, 2), (fields["picture_structure"], 2),
                         (pic.get("tff", 1), 1), (fields["frame_pred_frame_dct"], 1), (fields["concealment"], 1), (qst, 1), (fields["intra_vlc_format"], 1),
                         (alt, 1), (pic.get("rff", 0), 1), (pic.get("chroma_420_type", 0), 1), (fields["progressive_frame"], 1), (0, 1)):
        w.put(value, width)
    out.append(("picture_ext", w.bytes()))
    out += list(pic.get("extras", ()))
    L["pictures"].append(ptype)
    L["params"].append((tuple(f_code), prec, qst, alt))
    L["qcodes"].append([sl["q"] for sl in pic["slices"]])
    left = False                                                   # the slice in front left a predictor that is not zero
    for row, sl in enumerate(pic["slices"]):
        w = D._Writer()
        w.put(0x00000100 + sl.get("code", row + 1), 32)
        w.put(sl["q"], 5)
        w.put(0, 1)
        if left:
            L["resets"].add("slice")
        pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]                 # PMV[r][s]
        dc = [0, 0, 0]
        col, front = -1, None                                      # the directions of the macroblock in front (None: intra, or none yet)
        for mb in sl["mbs"]:
            incr = mb.get("incr", 1)
            MW.put_increment(w, incr)
            inherited = None
            if incr > 1:
                dc[:] = [0, 0, 0]
                if ptype == 2:                                     # 7.6.6: the zero vector, the predictors reset
                    if _nonzero(pmv):
                        L["resets"].add("p_skip")
                    pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                else:                                              # PMV[0][s] as frame vectors in the directions in front
                    inherited = (front, tuple(pmv[0][0]), tuple(pmv[0][1]))
                    if strict:
                        assert front is not None, "skipped behind an intra macroblock"
                        for k in range(1, incr):
                            assert all(frame_inside(col + k, row, pmv[0][s], mbw, mbh) for s in (0, 1) if front[s]), (col + k, row)
            col += incr
            quant, kind = mb.get("quant"), mb["kind"]
            intra = kind == "intra"
            fwd, bwd = (None, None) if intra or kind == "nomc" else (mb.get("fwd"), mb.get("bwd"))
            cbp = 63 if intra else (mb.get("cbp") or 0)
            if ptype == 3:
                key = (int(fwd is not None), int(bwd is not None), int(cbp != 0), int(quant is not None))
                bits = BW.TYPE_B_INTRA[key[3]] if intra else BW.TYPE_B[key]
            elif ptype == 2:
                name = "intra" if intra else "nomc" if kind == "nomc" else "coded" if cbp else "not_coded"
                bits = MW.TYPE_P[(name, quant is not None)]
            else:
                bits = MW.TYPE_I[("intra", quant is not None)]
            MW.put_bits(w, mb.get("type_bits") or bits)
            # macroblock_modes(): frame_motion_type behind macroblock_type where there is a vector, then dct_type where there are blocks
            motion = mb.get("motion", "frame")
            if fwd is not None or bwd is not None:
                w.put(mb.get("motion_bits", 1 if motion == "field" else 2), 2)
            if intra or cbp:
                w.put(mb.get("dct", 0), 1)
            if quant is not None:
                w.put(quant, 5)
                L["quants"].append((quant, qst))
            for s, v in ((0, fwd), (1, bwd)):
                if v is None:
                    continue
                fc = f_code[2 * s:2 * s + 2]
                if motion == "frame":                              # from PMV[0][s]; PMV[1][s] follows (7.6.3.3)
                    MW.put_vector(w, tuple(v), pmv[0][s], fc, L)
                    pmv[1][s] = list(pmv[0][s])
                    if strict:
                        assert frame_inside(col, row, v, mbw, mbh), (col, row, v)
                else:
                    L["selects"].add((v[0][0], v[1][0]))
                    for r in (0, 1):                               # select, then the vector from PMV[r][s]: vertical DIV 2 in, times 2 out
                        sel, mv = v[r]
                        w.put(sel, 1)
                        tmp = [pmv[r][s][0], pmv[r][s][1] >> 1]
                        MW.put_vector(w, tuple(mv), tmp, fc, L)
                        pmv[r][s] = [mv[0], 2 * mv[1]]
                        if strict:
                            assert field_inside(col, row, mv, mbw, mbh), (col, row, r, mv)
            if intra or (ptype == 2 and fwd is None):              # 7.6.3.4
                if _nonzero(pmv):
                    L["resets"].add("intra" if intra else "nomc")
                pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            if not intra:
                dc[:] = [0, 0, 0]
                if cbp:
                    w.code(W._tabs()["cbp"][cbp])
            front = None if intra else (1, 0) if ptype == 2 else (int(fwd is not None), int(bwd is not None))
            L["ilmbs"].append(dict(pic=len(L["pictures"]) - 1, type=ptype, row=row, col=col, kind=kind, motion=motion if (fwd or bwd) is not None else None,
                                   dct=mb.get("dct", 0) if (intra or cbp) else None, fwd=fwd, bwd=bwd, cbp=cbp, incr=incr, inherited=inherited, quant=quant))
            L["incrs"].append(incr)
            blocks = iter(mb.get("blocks", ()))
            for b in range(6):
                if (cbp >> (5 - b)) & 1:
                    MW.put_block(w, next(blocks), intra, 0 if b < 4 else b - 3, dc, L, alt)
        if strict:
            assert col == mbw - 1, "the row's last macroblock is coded"
        left = _nonzero(pmv)
        MW.put_bits(w, sl.get("tail", ""))
        out.append(("slice", w.bytes()))
    return out


def stream(w, h, pictures, seq=None, end=True, stuff=None, tail=0, strict=True, rows=None):
    """bpic_writer.stream with pictures of frame_pred_frame_dct 0 (field=True) among `pictures`; seq["progressive"] defaults to 0
    here.  rows: the macroblock rows the pictures are written with (default: the rule of 6.3.3)"""
    seq = dict(seq or {})
    seq.setdefault("progressive", 0)
    mbw, mbh = (w + 15) // 16, rows or mb_rows(h, seq["progressive"])
    L = new_log()
    units = []
    in_gop = 0
    for k, pic in enumerate(pictures):
        if pic.get("seq", k == 0):
            units += MW.sequence_units(w, h, seq)
        if pic.get("gop", k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x00 if pic.get("open_gop") else 0x40])))
            in_gop = 0
        if pic.get("field"):
            units += il_picture_units(in_gop, pic, mbw, mbh, L, strict)
        else:
            units += (BW.b_picture_units if pic["type"] == 3 else MW.picture_units)(in_gop, pic, mbw, mbh, L, strict)
        in_gop += 1
    if end:
        units.append(("end", b"\x00\x00\x01\xb7"))
    out = bytearray()
    for k, (kind, data) in enumerate(units):
        z = stuff(k, kind, len(out)) if callable(stuff) else (stuff or {}).get(k, 0)
        out += bytes(z)
        L["units"].append((kind, len(out)))
        out += data
    return bytes(out) + bytes(tail), L
