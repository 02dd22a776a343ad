"""A writer of MPEG-2 streams with field pictures (decoder.decode(..., syntax="main", interlaced=True, extended=True, mb_tools=True,
field_pictures=True)), field by field from ISO/IEC 13818-2 6.2.3.1, 6.2.5.1 and 6.3.17: picture_structure 1 / 2, two field pictures a
frame, field_motion_type, motion_vertical_field_select, 16 x 8 motion compensation, dual prime and concealment vectors in a field.  The
bit writer, the code tables, the cuts of a row, the slice headers' extras and Table B-15 are tests/dec_writer.py's, main_writer.py's,
bpic_writer.py's, ext_writer.py's and mbt_writer.py's; a frame picture is written by mbt_writer.picture_units; the macroblock layer of
a field picture is written here from ABSOLUTE vectors - the deltas are derived from the predictors this file keeps.  Nothing is shared
with decoder.py.

stream(w, h, pictures, seq=...) -> (bytes, log).  A picture is mbt_writer's, with
   ps=3 | 1 | 2    picture_structure: a frame picture (the default), a top field, a bottom field.  A field no first field waits for is
                   a first field, the next picture its partner: both carry the frame's temporal_reference ("tref" overrides it)
   ext=dict(...)   overrides of the coding extension's fields (picture_structure, top_field_first, frame_pred_frame_dct,
                   repeat_first_field, progressive_frame)
A field's slices hold macroblocks dict(kind="intra" | "pred" | "nomc", motion="field" | "16x8" | "dual", fwd=, bwd=, cbp=, quant=, incr=,
blocks=, cmv=(select, (vx, vy)), marker=):
   motion="field"  fwd / bwd = (select, (vx, vy)): one vector a direction from PMV[0][s]; PMV[1][s] follows
   motion="16x8"   fwd / bwd = ((select, (vx, vy)), (select, (vx, vy))): vector r from and into PMV[r][s]
   motion="dual"   fwd = ((vx, vy), (d0, d1)): no select, a dmvector behind each component; PMV[1][0] follows
No vertical component is halved: a field picture's vectors are field vectors as they stand.

The log is mbt_writer's with: fields (per coded picture: type, structure, whether it is its frame's second field, the frame's index),
fmbs (every macroblock of a field picture, skipped ones included: pic, frame, type, ps, second, row, col, kind, motion, fwd, bwd, cbp,
skipped, cmv), pairs (the kinds of pair written: (first structure, first type, second type))."""
import dec_cases as D
import ext_writer as XW
import ilace_writer as IW
import main_writer as MW
import bpic_writer as BW
import dec_writer as W
import mbt_writer as TW

MOTION_BITS = {"field": 1, "16x8": 2, "dual": 3}


def new_log():
    return dict(TW.new_log(), fields=[], fmbs=[], pairs=set())


def inside(col, row, mv, mbw, rows, half=None):
    """whether the vector reads inside a field of 16 mbw x 16 rows: the 16 x 16 of macroblock (col, row), or its upper / lower 16 x 8;
    luma and chroma (both components halved toward zero)"""
    y0, h = (16 * row, 16) if half is None else (16 * row + 8 * half, 8)
    for x, y, bw, bh, (vx, vy), pw, ph in ((16 * col, y0, 16, h, mv, 16 * mbw, 16 * rows),
                                           (8 * col, y0 // 2, 8, h // 2, (int(mv[0] / 2), int(mv[1] / 2)), 8 * mbw, 8 * rows)):
        ix, iy, hx, hy = vx >> 1, vy >> 1, vx & 1, vy & 1
        if not (x + ix >= 0 and y + iy >= 0 and x + ix + bw - 1 + hx < pw and y + iy + bh - 1 + hy < ph):
            return False
    return True


def field_units(tref, pic, mbw, rows, L, second, frame):
    """the units of one field picture"""
    ptype, ps, ivf, cmv = pic["type"], pic["ps"], pic.get("ivf", 0), pic.get("cmv", 0)
    f_code = (tuple(pic.get("f_code", (1, 1, 1, 1))) + (1, 1))[:4]
    prec, qst, alt = pic.get("prec", 2), pic.get("qst", 0), pic.get("alt", 0)
    index = len(L["pictures"])
    pic = XW.cut_picture(pic, mbw, L, index)
    out = []
    w = D._Writer()
    for value, width in ((0x00000100, 32), (tref & 1023, 10), (ptype, 3), (0xFFFF, 16)) + (((0, 1), (7, 3)) if ptype in (2, 3) else ()) + \
            (((0, 1), (7, 3)) if ptype == 3 else ()) + ((0, 1),):
        w.put(value, width)
    out.append(("picture", w.bytes()))
    w = D._Writer()
    fields = dict(picture_structure=ps, top_field_first=0, frame_pred_frame_dct=0, concealment=cmv, intra_vlc_format=ivf, repeat_first_field=0,
                  progressive_frame=0)
    fields.update(pic.get("ext", {}))
    said = f_code if ptype == 3 else (f_code[:2] if ptype == 2 or cmv else (15, 15)) + (15, 15)
    said = pic.get("ext_f_code", said)
    for value, width in ((0x000001B5, 32), (8, 4), (said[0], 4), (said[1], 4), (said[2], 4), (said[3], 4), (prec, 2), (fields["picture_structure"], 2),
                         (fields["top_field_first"], 1), (fields["frame_pred_frame_dct"], 1), (fields["concealment"], 1), (qst, 1),
                         (fields["intra_vlc_format"], 1), (alt, 1), (fields["repeat_first_field"], 1), (0, 1), (fields["progressive_frame"], 1), (0, 1)):
        w.put(value, width)
    out.append(("picture_ext", w.bytes()))
    out += list(pic.get("extras", ()))
    L["pictures"].append(ptype)
    L["params"].append((f_code, prec, qst, alt))
    L["qcodes"].append([sl["q"] for sl in pic["slices"]])
    L["fields"].append(dict(type=ptype, ps=ps, second=second, frame=frame))
    par = ps - 1
    for nth, sl in enumerate(pic["slices"]):
        row = sl.get("code", nth + 1) - 1
        w = D._Writer()
        w.put(0x00000100 + sl.get("code", nth + 1), 32)
        w.put(sl["q"], 5)
        w.put(0, 1)
        pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]                 # PMV[r][s]
        dc = [0, 0, 0]
        col = -1
        front = None                                               # the directions of the macroblock in front
        for mb in sl["mbs"]:
            incr = mb.get("incr", 1)
            MW.put_increment(w, incr)
            common = dict(pic=index, frame=frame, type=ptype, ps=ps, second=second, row=row)
            if incr > 1 and col >= 0:                              # skipped macroblocks (the slice's first increment only places it)
                dc[:] = [0, 0, 0]
                if ptype == 2:
                    pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                    skipped = dict(kind="pred", motion="field", fwd=(par, (0, 0)), bwd=None)
                else:
                    skipped = dict(kind="pred", motion="field", fwd=(par, tuple(pmv[0][0])) if front[0] else None, bwd=(par, tuple(pmv[0][1])) if front[1] else None)
                for k in range(1, incr):
                    L["fmbs"].append(dict(common, col=col + k, cbp=0, skipped=True, cmv=None, blocks=[], **skipped))
            col = col + incr if col >= 0 else incr - 1
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
            motion = mb.get("motion", "field")
            if fwd is not None or bwd is not None:                 # macroblock_modes(): field_motion_type; a field picture has no dct_type
                w.put(mb.get("motion_bits", MOTION_BITS[motion]), 2)
            if quant is not None:
                w.put(quant, 5)
                L["quants"].append((quant, qst))
            for s, v in ((0, fwd), (1, bwd)):
                if v is None:
                    continue
                fc = f_code[2 * s:2 * s + 2]
                if motion == "field":
                    sel, mv = v
                    w.put(sel, 1)
                    MW.put_vector(w, tuple(mv), pmv[0][s], fc, L)
                    pmv[1][s] = list(pmv[0][s])
                elif motion == "16x8":
                    for r in (0, 1):
                        sel, mv = v[r]
                        w.put(sel, 1)
                        MW.put_vector(w, tuple(mv), pmv[r][s], fc, L)
                else:                                              # component, dmvector, component, dmvector
                    (vx, vy), dmv = v
                    for t, target in enumerate((vx, vy)):
                        TW._component(w, target, pmv[0][0][t], fc[t], L)
                        MW.put_bits(w, {0: "0", 1: "10", -1: "11"}[dmv[t]])
                    pmv[0][0] = [vx, vy]
                    pmv[1][0] = [vx, vy]
            conceal = None
            if intra and fields["concealment"]:
                sel, v = mb.get("cmv", (0, (0, 0)))
                w.put(sel, 1)
                if IW._nonzero(pmv):
                    L["kept"] += 1
                MW.put_vector(w, tuple(v), pmv[0][0], f_code[:2], L)
                pmv[1][0] = list(pmv[0][0])
                w.put(mb.get("marker", 1), 1)
                conceal = (sel, tuple(v))
            elif intra or (ptype == 2 and fwd is None):            # 7.6.3.4
                pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            if not intra:
                dc[:] = [0, 0, 0]
                if cbp:
                    w.code(W._tabs()["cbp"][cbp])
            front = None if intra else (1, 0) if ptype == 2 else (int(fwd is not None), int(bwd is not None))
            L["mbs"].append(dict(pic=index, row=row, col=col, kind=kind, mv=(0, 0), cbp=cbp, incr=incr))
            L["fmbs"].append(dict(common, col=col, kind=kind, motion=motion if (fwd is not None or bwd is not None) else None, fwd=fwd, bwd=bwd, cbp=cbp,
                                  skipped=False, cmv=conceal, blocks=list(mb.get("blocks", ()))))
            L["incrs"].append(incr)
            blocks = iter(mb.get("blocks", ()))
            for b in range(6):
                if (cbp >> (5 - b)) & 1:
                    TW.put_block(w, next(blocks), intra, 0 if b < 4 else b - 3, dc, L, fields["intra_vlc_format"])
        MW.put_bits(w, sl.get("tail", ""))
        unit = w.bytes()
        if sl.get("header") is not None:
            unit = XW._with_extras(unit, sl["header"], L)
        out.append(("slice", unit))
    return out


def stream(w, h, pictures, seq=None, end=True, tail=0):
    """mbt_writer.stream with field pictures; pic["between"]: units written in front of the picture (a header between two fields)"""
    seq = dict(seq or {})
    seq.setdefault("progressive", 0)
    mbw, mbh = (w + 15) // 16, IW.mb_rows(h, seq["progressive"])
    L = new_log()
    units = []
    in_gop, frame, waiting = 0, -1, None
    for k, pic in enumerate(pictures):
        ps = pic.get("ps", 3)
        second = waiting is not None
        if pic.get("seq", k == 0):
            units += MW.sequence_units(w, h, seq)
        if pic.get("gop", k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x40])))
            in_gop = 0
        units += list(pic.get("between", ()))
        if not second:
            frame += 1
        tref = pic.get("tref", in_gop)
        if ps == 3:
            L["fields"].append(dict(type=pic["type"], ps=3, second=second, frame=frame))
            units += TW.picture_units(tref, pic, mbw, mbh, L)
        else:
            units += field_units(tref, pic, mbw, mbh // 2, L, second, frame)
        if second:
            L["pairs"].add((waiting["ps"], waiting["type"], pic["type"]))
            waiting = None
        elif ps != 3:
            waiting = pic
        if waiting is None:
            in_gop += 1
    if end:
        units.append(("end", b"\x00\x00\x01\xb7"))
    out = bytearray()
    for kind, data in units:
        L["units"].append((kind, len(out)))
        out += data
    return bytes(out) + bytes(tail), L
