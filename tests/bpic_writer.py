"""A writer of MPEG-2 streams with B pictures (option "decode_b_pictures"; decoder.decode(..., syntax="main", b_pictures=True)), field
by field from ISO/IEC 13818-2.  I and P pictures are tests/main_writer.py's; a B picture is written here: the picture header with the
backward pair, all four f_codes in the coding extension, Table B-4 by (directions, pattern, quant), vectors of both directions from
their own predictors with their own f_codes, skipped macroblocks.  Table B-4 is typed here a second time from the standard: nothing
is shared with decoder.py's copy, and tests/test_bpic_cases.py compares the two (and the kernels header's).

stream(w, h, pictures, ...) -> (bytes, log): the pictures in CODED order, as the caller gives them.  A B picture is
dict(type=3, slices=[...], f_code=(fh, fv, bh, bv), prec=, qst=, alt=, gop=, seq=, ext={...}, ext_f_code=, full_pel_backward=0); a macroblock of it
is dict(kind="pred" | "intra", fwd=(x, y) or None, bwd=(x, y) or None, cbp=None or 1 .. 63, quant=code or None, incr=1, blocks=[...]).
The log is main_writer's with, per B macroblock written, what the tests assert their streams really hold: btypes (the lines of Table
B-4 used), bmbs (place, directions, vectors, increment, and for the skipped ones in front the directions and vectors they inherit),
bvectors (direction, f_code, wrap, component, delta, predictor before)."""
import dec_cases as D
import dec_writer as W
import main_writer as MW

# Table B-4: (forward, backward, pattern, quant) -> macroblock_type; intra by quant
TYPE_B = {(1, 1, 0, 0): "10", (1, 1, 1, 0): "11", (0, 1, 0, 0): "010", (0, 1, 1, 0): "011", (1, 0, 0, 0): "0010", (1, 0, 1, 0): "0011",
          (1, 1, 1, 1): "00010", (1, 0, 1, 1): "000011", (0, 1, 1, 1): "000010"}
TYPE_B_INTRA = {0: "00011", 1: "000001"}


def new_log():
    return dict(MW.new_log(), btypes=set(), bmbs=[], bvectors=[])


def b_picture_units(n, pic, mbw, mbh, L, strict=True):
    f_code, prec, qst, alt = pic.get("f_code", (1, 1, 1, 1)), pic.get("prec", 2), pic.get("qst", 0), pic.get("alt", 0)
    ptype = pic.get("header_type", 3)
    out = []
    w = D._Writer()
    for value, width in ((0x00000100, 32), (n & 1023, 10), (ptype, 3), (0xFFFF, 16), (0, 1), (pic.get("forward_f_code", 7), 3),
                         (pic.get("full_pel_backward", 0), 1), (pic.get("backward_f_code", 7), 3), (0, 1)):
        w.put(value, width)
    out.append(("picture", w.bytes()))
    w = D._Writer()
    fields = dict(picture_structure=3, frame_pred_frame_dct=1, concealment=0, intra_vlc_format=0, progressive_frame=1)
    fields.update(pic.get("ext", {}))
    said = pic.get("ext_f_code", f_code)                          # what the extension says (a refusal: something the vectors are not written with)
    for value, width in ((0x000001B5, 32), (8, 4), (said[0], 4), (said[1], 4), (said[2], 4), (said[3], 4), (prec, 2), (fields["picture_structure"], 2),
                         (0, 1), (fields["frame_pred_frame_dct"], 1), (fields["concealment"], 1), (qst, 1), (fields["intra_vlc_format"], 1), (alt, 1), (0, 1), (1, 1),
                         (fields["progressive_frame"], 1), (0, 1)):
        w.put(value, width)
    out.append(("picture_ext", w.bytes()))
    out += list(pic.get("extras", ()))
    L["pictures"].append(3)
    L["params"].append((tuple(f_code), prec, qst, alt))
    L["qcodes"].append([sl["q"] for sl in pic["slices"]])
    for row, sl in enumerate(pic["slices"]):
        w = D._Writer()
        w.put(0x00000100 + sl.get("code", row + 1), 32)
        w.put(sl["q"], 5)
        w.put(0, 1)
        pmv = [[0, 0], [0, 0]]                                     # PMV[0][0] forward, PMV[0][1] backward
        dc = [0, 0, 0]
        col, front = -1, None                                      # the directions of the macroblock in front (None: intra, or none yet)
        for mb in sl["mbs"]:
            incr = mb.get("incr", 1)
            MW.put_increment(w, incr)
            inherited = None
            if incr > 1:                                           # skipped: the directions in front, the predictors as vectors
                inherited = (front, tuple(pmv[0]), tuple(pmv[1]))
                dc[:] = [0, 0, 0]
                if strict:
                    assert front is not None, "skipped behind an intra macroblock"
                    for k in range(1, incr):
                        assert all(W.inside(col + k, row, tuple(pmv[d]), mbw, mbh) for d in (0, 1) if front[d]), (col + k, row)
            col += incr
            quant = mb.get("quant")
            intra = mb["kind"] == "intra"
            fwd, bwd = (None, None) if intra else (mb.get("fwd"), mb.get("bwd"))
            cbp = 63 if intra else (mb.get("cbp") or 0)
            key = (int(fwd is not None), int(bwd is not None), int(cbp != 0), int(quant is not None))
            MW.put_bits(w, mb.get("type_bits") or (TYPE_B_INTRA[key[3]] if intra else TYPE_B[key]))
            L["btypes"].add(("intra", key[3]) if intra else key)
            if quant is not None:
                w.put(quant, 5)
                L["quants"].append((quant, qst))
            before = (tuple(pmv[0]), tuple(pmv[1]))
            for d, mv in ((0, fwd), (1, bwd)):
                if mv is None:
                    continue
                tmp = dict(vectors=[])
                MW.put_vector(w, tuple(mv), pmv[d], f_code[2 * d:2 * d + 2], tmp)
                L["bvectors"] += [(d, f, wrap, c, delta, before[d][t]) for t, (f, wrap, c, delta) in enumerate(tmp["vectors"])]
                if strict:
                    assert W.inside(col, row, tuple(mv), mbw, mbh), (col, row, mv)
            if intra:
                pmv = [[0, 0], [0, 0]]
            else:
                dc[:] = [0, 0, 0]
            if not intra and cbp:
                w.code(W._tabs()["cbp"][cbp])
            front = None if intra else (key[0], key[1])
            L["bmbs"].append(dict(pic=len(L["pictures"]) - 1, row=row, col=col, intra=intra, fwd=None if fwd is None else tuple(fwd),
                                  bwd=None if bwd is None else tuple(bwd), cbp=cbp, incr=incr, inherited=inherited, quant=quant))
            L["incrs"].append(incr)
            blocks = iter(mb.get("blocks", ()))
            for b in range(6):
                if (cbp >> (5 - b)) & 1:
                    MW.put_block(w, next(blocks), intra, 0 if b < 4 else b - 3, dc, L, alt)
        if strict:
            assert col == mbw - 1, "the row's last macroblock is coded"
        MW.put_bits(w, sl.get("tail", ""))
        out.append(("slice", w.bytes()))
    return out


def stream(w, h, pictures, seq=None, end=True, stuff=None, tail=0, strict=True):
    """main_writer.stream with B pictures among `pictures` (coded order)"""
    seq = seq or {}
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    L = new_log()
    units = []
    in_gop = 0
    for k, pic in enumerate(pictures):
        if pic.get("seq", k == 0):
            units += MW.sequence_units(w, h, seq)
        if pic.get("gop", k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x00 if pic.get("open_gop") else 0x40])))
            units += list(pic.get("gop_extras", ()))
            in_gop = 0
        units += (b_picture_units if pic["type"] == 3 else MW.picture_units)(in_gop, pic, mbw, mbh, L, strict)
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
