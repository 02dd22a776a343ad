"""A writer of main-syntax MPEG-2 streams (option "decode_syntax" = main; decoder.decode(..., syntax="main")), field by field from
ISO/IEC 13818-2: what an ordinary encoder writes and this project's never does - f_codes 1 .. 9 with motion residuals, every
intra_dc_precision, both quantiser scale tables, both scans, matrices in the sequence header, every macroblock type of tables B-2 / B-3,
macroblock quantisers, address increments with escapes (skipped macroblocks), optional and transparent units.

The bit writer and the run / level, DC, pattern and motion codes are tests/dec_writer.py's.  Table B-1, table 7-6 and figure 7-3 are
typed here a second time from the standard: nothing is shared with decoder.py's copies, and tests/test_main_cases.py compares the two.

stream(w, h, pictures, ...) -> (bytes, log).  A picture is dict(type=1 | 2, slices=[...], f_code=(h, v), prec=0 .. 3, qst=0 | 1, alt=0 | 1,
gop=bool, seq=bool, extras=[units behind the picture coding extension], gop_extras=[units behind the GOP header]); a slice is
dict(q=code, mbs=[...]); a macroblock is dict(kind="intra" | "coded" | "not_coded" | "nomc", quant=code or None, incr=address increment
(default 1: incr - 1 macroblocks in front of it are skipped), mv=(x, y), cbp=, blocks=[...]) with dec_writer's blocks."""
import dec_cases as D
import dec_writer as W

# Table B-1: macroblock_address_increment 1 .. 33, and macroblock_escape
B1 = ("1", "011", "010", "0011", "0010", "00011", "00010", "0000111", "0000110", "00001011", "00001010", "00001001", "00001000", "00000111",
      "00000110", "0000010111", "0000010110", "0000010101", "0000010100", "0000010011", "0000010010", "00000100011", "00000100010",
      "00000100001", "00000100000", "00000011111", "00000011110", "00000011101", "00000011100", "00000011011", "00000011010", "00000011001",
      "00000011000")
B1_ESCAPE = "00000001000"
# table 7-6: quantiser_scale for quantiser_scale_code 1 .. 31 with q_scale_type 1
NONLINEAR = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112)
# figure 7-3: alternate scan, the scan position of raster [v][u], row by row
ALTERNATE = ((0, 4, 6, 20, 22, 36, 38, 52), (1, 5, 7, 21, 23, 37, 39, 53), (2, 8, 19, 24, 34, 40, 50, 54), (3, 9, 18, 25, 35, 41, 51, 55),
             (10, 17, 26, 30, 42, 46, 56, 60), (11, 16, 27, 31, 43, 47, 57, 61), (12, 15, 28, 32, 44, 48, 58, 62), (13, 14, 29, 33, 45, 49, 59, 63))
# tables B-2 and B-3: kind, quant -> macroblock_type
TYPE_I = {("intra", False): "1", ("intra", True): "01"}
TYPE_P = {("coded", False): "1", ("nomc", False): "01", ("not_coded", False): "001", ("intra", False): "00011", ("coded", True): "00010",
          ("nomc", True): "00001", ("intra", True): "000001"}


def scale(code, qst):
    return (NONLINEAR[code - 1] if code else 0) if qst else 2 * code


def scan_position(raster, alt):
    """where coefficient `raster` lies in the picture's scan"""
    return ALTERNATE[raster >> 3][raster & 7] if alt else W._tabs()["raster"].index(raster)


def new_log():
    return dict(W.new_log(), types=set(), incrs=[], vectors=[], params=[], quants=[])


def put_bits(w, bits):
    for b in bits:
        w.put(int(b), 1)


def put_increment(w, incr):
    while incr > 33:
        put_bits(w, B1_ESCAPE)
        incr -= 33
    put_bits(w, B1[incr - 1])


def put_vector(w, mv, pmv, f_code, L):
    """7.6.3.1 backwards: the delta nearest zero that reaches mv from pmv modulo the range -> motion_code, motion_residual"""
    T = W._tabs()
    for c in range(2):
        r_size = f_code[c] - 1
        f = 1 << r_size
        delta = mv[c] - pmv[c]
        wrap = 0
        if delta < -16 * f:
            delta, wrap = delta + 32 * f, 1
        elif delta > 16 * f - 1:
            delta, wrap = delta - 32 * f, -1
        assert -16 * f <= mv[c] <= 16 * f - 1 and -16 * f <= delta <= 16 * f - 1
        if f == 1 or delta == 0:
            code, residual = abs(delta), None
        else:
            code, residual = (abs(delta) - 1) // f + 1, (abs(delta) - 1) % f
        w.code(T["motion"][code])
        if code:
            w.put(delta < 0, 1)
        if residual is not None:
            w.put(residual, r_size)
        L["vectors"].append((f_code[c], wrap, mv[c], delta))
        L.setdefault("codes", []).append((f_code[c], -code if delta < 0 else code, residual or 0, pmv[c]))      # what a decoder reads, and the predictor it was written against
        pmv[c] = mv[c]


def put_block(w, blk, intra, comp, pred, L, alt):
    """dec_writer's block; with alternate_scan the (run, level) list is the caller's, already in the picture's scan order"""
    W._put_block(w, blk, intra, comp, pred, L, True)


def picture_units(n, pic, mbw, mbh, L, strict=True):
    ptype = pic["type"]
    f_code, prec, qst, alt = pic.get("f_code", (1, 1)), pic.get("prec", 2), pic.get("qst", 0), pic.get("alt", 0)
    out = []
    w = D._Writer()
    for value, width in ((0x00000100, 32), (n & 1023, 10), (ptype, 3), (0xFFFF, 16)) + (((0, 1), (7, 3)) if ptype in (2, 3) else ()) + (((0, 1), (7, 3)) if ptype == 3 else ()) + ((0, 1),):
        w.put(value, width)
    out.append(("picture", w.bytes()))
    w = D._Writer()
    fields = dict(picture_structure=3, frame_pred_frame_dct=1, concealment=0, intra_vlc_format=0, progressive_frame=1, composite_display_flag=0)
    fields.update(pic.get("ext", {}))
    for value, width in ((0x000001B5, 32), (8, 4), (f_code[0], 4), (f_code[1], 4), (15, 4), (15, 4), (prec, 2), (fields["picture_structure"], 2), (0, 1),
                         (fields["frame_pred_frame_dct"], 1), (fields["concealment"], 1), (qst, 1), (fields["intra_vlc_format"], 1), (alt, 1), (0, 1), (1, 1),
                         (fields["progressive_frame"], 1), (fields["composite_display_flag"], 1)) + \
            (((1, 1), (3, 3), (0, 1), (5, 7), (9, 8)) if fields["composite_display_flag"] else ()):      # v_axis, field_sequence, sub_carrier, burst_amplitude, sub_carrier_phase
        w.put(value, width)
    out.append(("picture_ext", w.bytes()))
    out += list(pic.get("extras", ()))
    L["pictures"].append(ptype)
    L["params"].append((tuple(f_code), prec, qst, alt))
    L["qcodes"].append([sl["q"] for sl in pic["slices"]])
    for row, sl in enumerate(pic["slices"]):
        w = D._Writer()
        w.put(0x00000100 + sl.get("code", row + 1), 32)
        w.put(sl["q"], 5)
        if sl.get("intra_slice_flag"):                              # intra_slice_flag, intra_slice, reserved_bits, then extra_bit_slice
            for value, width in ((1, 1), (0, 1), (0, 7)):
                w.put(value, width)
        w.put(0, 1)
        st = dict(pmv=[0, 0], dc=[0, 0, 0])
        col = -1
        for mb in sl["mbs"]:
            incr = mb.get("incr", 1)
            put_increment(w, incr)
            if incr > 1:
                st["pmv"][:] = [0, 0]
                st["dc"][:] = [0, 0, 0]
            col += incr
            kind, quant = mb["kind"], mb.get("quant")
            put_bits(w, mb.get("type_bits") or (TYPE_I if ptype == 1 else TYPE_P)[(kind, quant is not None)])
            if quant is not None:
                w.put(quant, 5)
                L["quants"].append((quant, qst))
            L["types"].add((ptype, kind, quant is not None))
            L["incrs"].append(incr)
            mv = (0, 0)
            if kind in ("coded", "not_coded"):
                mv = tuple(mb["mv"])
                put_vector(w, mv, st["pmv"], f_code, L)
                if strict:
                    assert W.inside(col, row, mv, mbw, mbh), (col, row, mv)
            else:
                st["pmv"][:] = [0, 0]
            if kind != "intra":
                st["dc"][:] = [0, 0, 0]
            cbp = 63 if kind == "intra" else mb["cbp"] if kind in ("coded", "nomc") else 0
            if kind in ("coded", "nomc"):
                w.code(W._tabs()["cbp"][cbp])
            L["mbs"].append(dict(pic=len(L["pictures"]) - 1, row=row, col=col, kind=kind, mv=mv, cbp=cbp, incr=incr))
            blocks = iter(mb.get("blocks", ()))
            for b in range(6):
                if (cbp >> (5 - b)) & 1:
                    put_block(w, next(blocks), kind == "intra", 0 if b < 4 else b - 3, st["dc"], L, alt)
        if strict:
            assert col == mbw - 1, "the row's last macroblock is coded"
        put_bits(w, sl.get("tail", ""))
        out.append(("slice", w.bytes()))
    return out


def matrix_bytes(raster):
    """64 weights in raster order -> the 64 bytes of the header, zig-zag order"""
    order = W._tabs()["raster"]
    return [raster[order[k]] for k in range(64)]


def sequence_units(w, h, seq):
    """sequence_header (with the matrices of seq), sequence_extension, [user_data], [sequence_display_extension]"""
    b = D._Writer()
    for value, width in ((0x000001B3, 32), (w, 12), (h, 12), (seq.get("aspect", 1), 4), (seq.get("frame_rate_code", 3), 4), (10000, 18), (1, 1), (5, 10), (0, 1)):
        b.put(value, width)
    for name in ("intra_matrix", "non_intra_matrix"):
        m = seq.get(name)
        b.put(m is not None, 1)
        for v in matrix_bytes(m) if m is not None else ():
            b.put(v, 8)
    units = [("sequence", b.bytes())]
    b = D._Writer()
    for value, width in ((0x000001B5, 32), (1, 4), (0x44, 8), (seq.get("progressive", 1), 1), (seq.get("chroma_format", 1), 2), (seq.get("size_ext", 0), 4), (0, 12), (1, 1), (0, 8),
                         (seq.get("low_delay", 0), 1), (0, 7)):
        b.put(value, width)
    units.append(("sequence_ext", b.bytes()))
    units += list(seq.get("extras", ()))
    if seq.get("display", True):
        b = D._Writer()
        for value, width in ((0x000001B5, 32), (2, 4), (5, 3), (0, 1), (w, 14), (1, 1), (h, 14)):
            b.put(value, width)
        units.append(("display_ext", b.bytes()))
    units += list(seq.get("extras_behind", ()))
    return units


USER = ("user", b"\x00\x00\x01\xb2" + b"made by main_writer \xff\x00\x00\x02")
COPYRIGHT = ("copyright", b"\x00\x00\x01\xb5" + bytes([0x48, 0x12, 0x81, 0x11, 0x18, 0x11, 0x11, 0x91, 0x11, 0x15, 0x20]))      # id 4, copyright_flag, ..., marker bits
PICTURE_DISPLAY = ("picture_display", b"\x00\x00\x01\xb5" + bytes([0x70, 0x08, 0x80, 0x04, 0x40]))                                  # id 7, one frame centre offset


def stream(w, h, pictures, seq=None, end=True, stuff=None, tail=0, strict=True):
    """-> (stream, log).  seq: dict(intra_matrix=, non_intra_matrix= (raster lists), display=bool, extras=[units behind sequence_extension],
    extras_behind=[units behind the display extension]); end: sequence_end_code; tail: zero bytes behind the last unit;
    stuff: dec_writer.assemble's"""
    seq = seq or {}
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    L = new_log()
    units = []
    in_gop = 0
    for k, pic in enumerate(pictures):
        if pic.get("seq", k == 0):
            units += sequence_units(w, h, seq)
        if pic.get("gop", k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x40])))
            units += list(pic.get("gop_extras", ()))
            in_gop = 0
        units += picture_units(in_gop, pic, mbw, mbh, L, strict)
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
