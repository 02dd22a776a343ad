"""A writer of MPEG-2 streams with what option "decode_mb_tools" adds (decoder.decode(..., syntax="main", extended=True,
mb_tools=True)), field by field from ISO/IEC 13818-2: Table B-15 for the intra blocks of a picture with intra_vlc_format 1,
concealment motion vectors, dual prime.  The bit writer, the code tables of the other layers, the cuts of a row and the slice
headers' extras are tests/dec_writer.py's, main_writer.py's, bpic_writer.py's and ext_writer.py's; the macroblock layer is written
here, one function for every picture kind, so that the SAME macroblocks can be written with intra_vlc_format 0 or 1, with or without
concealment vectors, with or without dual prime.  Nothing is shared with decoder.py's macroblock layer.

stream(w, h, pictures, seq=...) -> (bytes, log): ext_writer.stream's pictures with
   ivf=0 | 1      intra_vlc_format: the AC coefficients of intra blocks by Table B-15 (typed here as code strings: the 41 codes that
                  differ from B-14, the end of block; the 70 long codes the two tables share are B-14's, by the rule that names them)
   cmv=0 | 1      concealment_motion_vectors: every intra macroblock carries its "cmv" (an ABSOLUTE frame vector, default (0, 0)) and a
                  marker bit ("marker", default 1) behind its quantiser; it moves PMV[0][0] and PMV[1][0] and the macroblock does not
                  reset the predictors.  An I picture then says f_code[0][*] as a P picture does
   tff=0 | 1      top_field_first
   field=True     frame_pred_frame_dct 0: macroblock_modes() is written
A macroblock is ilace_writer's - dict(kind="intra" | "pred" | "nomc", motion="frame" | "field" | "dual", dct=, fwd=, bwd=, cbp=, quant=,
incr=, blocks=) - or main_writer's ("coded" / "not_coded" with mv=).  motion="dual": fwd=((vx, vy), (d0, d1)), the vector (vertical in
half samples of the field) and the dmvector.  Every vector is absolute: the deltas are derived here from the predictors, so a
concealment vector that moves a predictor changes the delta of the vector behind it, not the vector.

The log is ext_writer's with: b15 (every (run, level, sign) written with a B-15 code, (None, 0, 0) for an end of block directly behind
the DC), b15_escapes, cmvs (picture, row, col, vector, whether a predicted macroblock with a forward vector follows in the slice),
duals (picture, row, col, vector, dmvector, top_field_first), kept (predictors that were not zero kept across an intra macroblock)."""
import bpic_writer as BW
import dec_cases as D
import dec_writer as W
import ext_writer as XW
import ilace_writer as IW
import main_writer as MW

# Table B-15: the 41 codes that differ from Table B-14, (run, level) -> code without the sign bit
B15 = {(0, 1): "10", (0, 2): "110", (0, 3): "0111", (0, 4): "11100", (0, 5): "11101", (0, 6): "000101", (0, 7): "000100",
       (0, 8): "1111011", (0, 9): "1111100", (0, 10): "00100011", (0, 11): "00100010", (0, 12): "11111010", (0, 13): "11111011",
       (0, 14): "11111110", (0, 15): "11111111",
       (1, 1): "010", (1, 2): "00110", (1, 3): "1111001", (1, 4): "00100111", (1, 5): "00100000",
       (2, 1): "00101", (2, 2): "0000111", (2, 3): "11111100", (2, 4): "0000001100",
       (3, 1): "00111", (3, 2): "00100110", (4, 1): "000110", (4, 2): "11111101", (5, 1): "000111", (5, 2): "000000100",
       (6, 1): "0000110", (7, 1): "0000100", (8, 1): "0000101", (9, 1): "1111000", (10, 1): "1111010", (11, 1): "00100001",
       (12, 1): "00100101", (13, 1): "00100100", (14, 1): "000000101", (15, 1): "000000111", (16, 1): "0000001101"}
B15_EOB, ESCAPE = "0110", "000001"
B15_MOVED = tuple((0, l) for l in range(8, 16)) + ((1, 5), (2, 4))     # pairs of B-14's long codes that have a short code in B-15


def b15_codes():
    """all of Table B-15: (run, level) -> code string; the shared codes are B-14's that begin with seven zero bits, but for B15_MOVED"""
    out = dict(B15)
    for pair, (code, length) in W._tabs()["ac"].items():
        bits = format(code, "0%db" % length)
        if bits.startswith("0000000") and pair not in B15_MOVED:
            assert pair not in out
            out[pair] = bits
    return out


def new_log():
    return dict(XW.new_log(), b15=set(), b15_escapes=[], cmvs=[], duals=[], kept=0, tmbs=[])


def put_block(w, blk, intra, comp, pred, L, ivf):
    """dec_writer's block; an intra block of a picture with intra_vlc_format 1 by Table B-15"""
    if not (intra and ivf):
        return W._put_block(w, blk, intra, comp, pred, L, True)
    T = W._tabs()
    codes = b15_codes()
    diff = int(blk.get("dc", 0))
    size = abs(diff).bit_length()
    assert size <= 11
    w.code(T["dcc" if comp else "dcy"][size])
    if size:
        w.put(diff if diff > 0 else diff + (1 << size) - 1, size)
    pred[comp] += diff
    L["dc"].append((comp, size, (diff > 0) - (diff < 0), pred[comp], pred[comp] - diff, len(L["mbs"]) - 1))
    k, levels = 1, []
    for run, lvl, esc in blk.get("coefs", ()):
        k += run
        assert k < 64 and lvl != 0 and -2047 <= lvl <= 2047
        if (run, abs(lvl)) in codes and not esc:
            MW.put_bits(w, blk.get("codes", {}).get((run, abs(lvl)), codes[(run, abs(lvl))]))
            w.put(lvl < 0, 1)
            L["b15"].add((run, abs(lvl), lvl < 0))
        else:
            MW.put_bits(w, ESCAPE)
            w.put(run, 6)
            w.put(lvl & 0xFFF, 12)
            L["b15_escapes"].append((run, lvl))
        levels.append((k, lvl))
        k += 1
    if not levels:
        L["b15"].add((None, 0, 0))
    MW.put_bits(w, B15_EOB)
    L["blocks"].append((True, comp, levels))


def _normal(mb):
    """main_writer's macroblock as ilace_writer's"""
    if mb["kind"] in ("coded", "not_coded"):
        return dict(mb, kind="pred", fwd=tuple(mb["mv"]), bwd=None, cbp=mb.get("cbp", 0) if mb["kind"] == "coded" else 0)
    return mb


def _component(w, v, p, f_code, L=None):
    """one vector component v behind its predictor p (7.6.3.1 backwards): motion_code, sign, motion_residual; L: the log that gets it"""
    tmp = D._Writer()
    pmv = [p, 0]
    own = dict(vectors=[])
    MW.put_vector(tmp, (v, 0), pmv, (f_code, 1), own)
    if L is not None:
        L.setdefault("dual_vectors", []).append(own["vectors"][0])
        L.setdefault("codes", []).append(own["codes"][0])
    w.s += tmp.s[:-1]                                              # (the second component, 0 behind 0, is motion_code '1')
    assert tmp.s[-1] == "1"


def picture_units(n, pic, mbw, mbh, L):
    ptype, field, ivf, cmv = pic["type"], bool(pic.get("field")), pic.get("ivf", 0), pic.get("cmv", 0)
    f_code = tuple(pic.get("f_code", (1, 1, 1, 1))) + (1, 1)
    f_code = f_code[:4]
    prec, qst, alt = pic.get("prec", 2), pic.get("qst", 0), pic.get("alt", 0)
    tff = pic.get("tff", 1 if field else 0)
    index = len(L["pictures"])
    pic = XW.cut_picture(dict(pic, slices=[dict(sl, mbs=[_normal(m) for m in sl["mbs"]]) for sl in pic["slices"]]), mbw, L, index)
    out = []
    w = D._Writer()
    for value, width in ((0x00000100, 32), (n & 1023, 10), (ptype, 3), (0xFFFF, 16)) + (((0, 1), (7, 3)) if ptype in (2, 3) else ()) + \
            (((0, 1), (7, 3)) if ptype == 3 else ()) + ((0, 1),):
        w.put(value, width)
    out.append(("picture", w.bytes()))
    w = D._Writer()
    fields = dict(picture_structure=3, frame_pred_frame_dct=0 if field else 1, concealment=cmv, intra_vlc_format=ivf, progressive_frame=0 if field else 1)
    fields.update(pic.get("ext", {}))
    said = f_code if ptype == 3 else (f_code[:2] if ptype == 2 or cmv else (15, 15)) + (15, 15)
    said = pic.get("ext_f_code", said)
    for value, width in ((0x000001B5, 32), (8, 4), (said[0], 4), (said[1], 4), (said[2], 4), (said[3], 4), (prec, 2), (fields["picture_structure"], 2),
                         (tff, 1), (fields["frame_pred_frame_dct"], 1), (fields["concealment"], 1), (qst, 1), (fields["intra_vlc_format"], 1),
                         (alt, 1), (0, 1), (fields["progressive_frame"], 1), (fields["progressive_frame"], 1), (0, 1)):
        w.put(value, width)
    out.append(("picture_ext", w.bytes()))
    out += list(pic.get("extras", ()))
    L["pictures"].append(ptype)
    L["params"].append((f_code, prec, qst, alt))
    L["qcodes"].append([sl["q"] for sl in pic["slices"]])
    for nth, sl in enumerate(pic["slices"]):
        row = sl.get("code", nth + 1) - 1
        w = D._Writer()
        w.put(0x00000100 + sl.get("code", nth + 1), 32)
        w.put(sl["q"], 5)
        w.put(0, 1)
        pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]                 # PMV[r][s]
        dc = [0, 0, 0]
        col = -1
        for at, mb in enumerate(sl["mbs"]):
            incr = mb.get("incr", 1)
            MW.put_increment(w, incr)
            if incr > 1 and col >= 0:                              # skipped macroblocks (the slice's first increment only places it)
                dc[:] = [0, 0, 0]
                if ptype == 2:
                    pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
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
            motion = mb.get("motion", "frame")
            if field or pic.get("force_modes"):                    # macroblock_modes()
                if fwd is not None or bwd is not None:
                    w.put(mb.get("motion_bits", dict(field=1, frame=2, dual=3)[motion]), 2)
                if intra or cbp:
                    w.put(mb.get("dct", 0), 1)
            if quant is not None:
                w.put(quant, 5)
                L["quants"].append((quant, qst))
            for s, v in ((0, fwd), (1, bwd)):
                if v is None:
                    continue
                fc = f_code[2 * s:2 * s + 2]
                if motion == "frame":                              # from PMV[0][s]; PMV[1][s] follows
                    MW.put_vector(w, tuple(v), pmv[0][s], fc, L)
                    pmv[1][s] = list(pmv[0][s])
                elif motion == "dual":                             # component, dmvector, component, dmvector; the vertical one a field vector
                    (vx, vy), dmv = v
                    for t, (target, p) in enumerate(((vx, pmv[0][0][0]), (vy, pmv[0][0][1] >> 1))):
                        _component(w, target, p, fc[t], L)
                        MW.put_bits(w, {0: "0", 1: "10", -1: "11"}[dmv[t]])
                    pmv[0][0] = [vx, 2 * vy]
                    pmv[1][0] = [vx, 2 * vy]
                    L["duals"].append((index, row, col, (vx, vy), tuple(dmv), tff))
                else:
                    L["selects"].add((v[0][0], v[1][0]))
                    for r in (0, 1):                               # select, then the vector from PMV[r][s]: vertical DIV 2 in, times 2 out
                        sel, mv = v[r]
                        w.put(sel, 1)
                        tmp = [pmv[r][s][0], pmv[r][s][1] >> 1]
                        MW.put_vector(w, tuple(mv), tmp, fc, L)
                        pmv[r][s] = [mv[0], 2 * mv[1]]
            if intra and fields["concealment"]:
                v = tuple(mb.get("cmv", (0, 0)))
                if IW._nonzero(pmv):
                    L["kept"] += 1
                MW.put_vector(w, v, pmv[0][0], f_code[:2], L)
                pmv[1][0] = list(pmv[0][0])
                w.put(mb.get("marker", 1), 1)
                behind = [m for m in sl["mbs"][at + 1:at + 2] if m["kind"] == "pred" and m.get("fwd") is not None and m.get("incr", 1) == 1]
                L["cmvs"].append((index, row, col, v, bool(behind)))
            elif intra or (ptype == 2 and fwd is None):            # 7.6.3.4
                pmv = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
            if not intra:
                dc[:] = [0, 0, 0]
                if cbp:
                    w.code(W._tabs()["cbp"][cbp])
            L["mbs"].append(dict(pic=index, row=row, col=col, kind=kind, mv=(0, 0), cbp=cbp, incr=incr))
            L["tmbs"].append(dict(pic=index, type=ptype, row=row, col=col, kind=kind, motion=motion if (fwd or bwd) is not None else None, fwd=fwd, bwd=bwd,
                                  cbp=cbp, incr=incr, cmv=tuple(mb.get("cmv", (0, 0))) if intra and fields["concealment"] else None))
            L["incrs"].append(incr)
            blocks = iter(mb.get("blocks", ()))
            for b in range(6):
                if (cbp >> (5 - b)) & 1:
                    put_block(w, next(blocks), intra, 0 if b < 4 else b - 3, dc, L, fields["intra_vlc_format"])
        MW.put_bits(w, sl.get("tail", ""))
        unit = w.bytes()
        if sl.get("header") is not None:
            unit = XW._with_extras(unit, sl["header"], L)
        out.append(("slice", unit))
    return out


def stream(w, h, pictures, seq=None, end=True, tail=0):
    """ext_writer.stream over picture_units above"""
    seq = dict(seq or {})
    seq.setdefault("progressive", 0 if any(p.get("field") for p in pictures) else 1)
    mbw, mbh = (w + 15) // 16, IW.mb_rows(h, seq["progressive"])
    L = new_log()
    units = []
    in_gop = 0
    for k, pic in enumerate(pictures):
        if pic.get("seq", k == 0):
            units += MW.sequence_units(w, h, seq)
        if pic.get("gop", k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x40])))
            in_gop = 0
        units += picture_units(in_gop, pic, mbw, mbh, L)
        in_gop += 1
    if end:
        units.append(("end", b"\x00\x00\x01\xb7"))
    out = bytearray()
    for kind, data in units:
        L["units"].append((kind, len(out)))
        out += data
    return bytes(out) + bytes(tail), L
