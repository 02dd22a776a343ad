"""A writer of MPEG-2 streams with what option "decode_extended" adds (decoder.decode(..., syntax="main", extended=True)), field by
field from ISO/IEC 13818-2: several slices in a macroblock row, slice headers with intra_slice_flag 1 and extra_information_slice
bytes, quant_matrix_extension, composite_display_flag 1.  The bit writer, the code tables and the macroblock layer are
tests/dec_writer.py's, main_writer.py's, bpic_writer.py's and ilace_writer.py's; the slice layer is written here.  Nothing is shared
with decoder.py.

stream(w, h, pictures, seq=...) -> (bytes, log): ilace_writer.stream's pictures (of any of the three kinds), each with two more keys:
   cuts     per macroblock row the columns at which a new slice begins, e.g. [[], [1], [2], [1, 2]]: the row's macroblocks are the
            same ones, but every slice after a cut starts with all predictors reset (6.3.16, 7.2.1, 7.6.3.4), so the writer re-derives
            what is carried: the slice's quantiser_scale_code is the one in force at the cut, the first macroblock's address increment
            is its column + 1, an intra macroblock's first DC
            differentials of each component are its absolute values, and the vectors' deltas come from zero predictors (the
            macroblock writers take vectors as absolute values).  A cut is only possible at a macroblock that is written (a skipped
            one has no place to start a slice from)
   a slice's header=dict(intra_slice=0 | 1, info=[bytes]): intra_slice_flag 1, intra_slice, reserved_bits, then one
            extra_bit_slice 1 + extra_information_slice per byte of info, then the closing 0 (6.2.4); closing=False leaves that 0 out
quant_ext(intra=, non_intra=, chroma=(0, 0)) is a quant_matrix_extension unit for a picture's extras (6.2.3.2).

The log is ilace_writer's with: cuts (per slice written: picture, row, first and last column, whether a skipped run follows its first
macroblock, whether one ends in front of its last), extras (the number of information bytes of every slice with intra_slice_flag 1,
and its intra_slice), dc_rederived and vectors_rederived (cuts at which a DC predictor / a vector predictor that was not zero was
reset)."""
import copy

import bpic_writer as BW
import dec_cases as D
import ilace_writer as IW
import main_writer as MW


def new_log():
    return dict(IW.new_log(), cuts=[], extras=[], dc_rederived=0, vectors_rederived=0, loads=[])


def quant_ext(intra=None, non_intra=None, chroma=(0, 0), cut=None):
    """quant_matrix_extension: identifier 3, load_intra_quantiser_matrix [64 bytes, zig-zag], load_non_intra_quantiser_matrix [64 bytes],
    load_chroma_intra_quantiser_matrix, load_chroma_non_intra_quantiser_matrix (both 0 in 4:2:0; a 1 is written without a matrix).  cut: the unit's first `cut` bytes only"""
    w = D._Writer()
    w.put(0x000001B5, 32)
    w.put(3, 4)
    for m in (intra, non_intra):
        w.put(m is not None, 1)
        for v in MW.matrix_bytes(m) if m is not None else ():
            w.put(v, 8)
    w.put(chroma[0], 1)
    w.put(chroma[1], 1)
    data = w.bytes()
    return ("quant_matrix", data if cut is None else data[:cut])


def _absolute_dc(mbs):
    """the DC predictors in front of every macroblock of an uncut row, relative to the reset value"""
    pred, out = [0, 0, 0], []
    for mb in mbs:
        if mb.get("incr", 1) > 1 or mb["kind"] != "intra":
            pred = [0, 0, 0]
        out.append(list(pred))
        if mb["kind"] == "intra":
            for b, blk in enumerate(mb["blocks"]):
                pred[0 if b < 4 else b - 3] += int(blk.get("dc", 0))
    return out


def _has_vector(mb):
    return any(mb.get(k) is not None for k in ("fwd", "bwd")) or (mb["kind"] in ("coded", "not_coded") and tuple(mb.get("mv", (0, 0))) != (0, 0))


def cut_picture(pic, mbw, L, index):
    """the picture with its rows cut at pic["cuts"]: more slices, each with its code, its first increment and its re-derived DC"""
    cuts = pic.get("cuts")
    out = dict(pic)
    out["slices"] = []
    for row, sl in enumerate(pic["slices"]):
        code = sl.get("code", row + 1)
        at = sorted(cuts[row]) if cuts and row < len(cuts) else []
        cols, col = [], -1
        for mb in sl["mbs"]:
            col += mb.get("incr", 1)
            cols.append(col)
        front = _absolute_dc(sl["mbs"])
        scale, q = [], sl["q"]                                  # the quantiser_scale_code in force in front of every macroblock
        for mb in sl["mbs"]:
            scale.append(q)
            q = mb["quant"] if mb.get("quant") is not None else q
        if pic.get("strict_cuts", True):                        # a skipped macroblock neither starts a slice nor ends one
            assert all(c in cols and c - 1 in cols for c in at), (row, at, cols)
        starts = [0] + [cols.index(c) for c in at]
        for k, first in enumerate(starts):
            last = starts[k + 1] if k + 1 < len(starts) else len(sl["mbs"])
            mbs = [copy.deepcopy(m) for m in sl["mbs"][first:last]]
            if k:
                head = mbs[0]
                head["incr"] = cols[first] + 1
                if head["kind"] == "intra" and any(front[first]):
                    L["dc_rederived"] += 1
                    seen = set()
                    for b, blk in enumerate(head["blocks"]):
                        comp = 0 if b < 4 else b - 3
                        if comp not in seen:
                            blk["dc"] = int(blk.get("dc", 0)) + front[first][comp]
                            seen.add(comp)
                if any(_has_vector(m) for m in sl["mbs"][:first]) and _has_vector(head):
                    L["vectors_rederived"] += 1
            piece = dict(sl, code=code, mbs=mbs, q=scale[first] if mbs else sl["q"])
            if k and "tail" in piece and last != len(sl["mbs"]):
                del piece["tail"]
            L["cuts"].append(dict(pic=index, row=row, first=cols[first] if mbs else None, last=cols[last - 1] if mbs else None, slices=len(starts),
                                  skip_behind_first=len(mbs) > 1 and mbs[1].get("incr", 1) > 1, skip_before_last=len(mbs) > 1 and mbs[-1].get("incr", 1) > 1))
            out["slices"].append(piece)
    return out


def _with_extras(unit, extras, L):
    """a slice unit with intra_slice_flag 1 and what follows it in place of the extra_bit_slice 0 behind quantiser_scale_code; every
    bit behind keeps its place in the order, and the unit is stuffed to a whole byte again"""
    bits = "".join(format(b, "08b") for b in unit)
    assert bits[37] == "0"
    info = list(extras.get("info", ()))
    head = "1" + str(int(extras.get("intra_slice", 0))) + format(extras.get("reserved", 0), "07b") + "".join("1" + format(v, "08b") for v in info)
    if extras.get("closing", True):
        head += "0"
    L["extras"].append((len(info), int(extras.get("intra_slice", 0))))
    rest = bits[38:]
    if not extras.get("closing", True) and "1" not in rest:     # nothing behind: not even stuffing, which would read as the closing 0
        rest = ""
    bits = bits[:37] + head + rest
    bits += "0" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big")


def picture_units(n, pic, mbw, mbh, L):
    """the units of one picture: its kind's writer on the cut picture, then the slice headers' extras"""
    index = len(L["pictures"])
    cut = cut_picture(pic, mbw, L, index)
    write = IW.il_picture_units if pic.get("field") else BW.b_picture_units if pic["type"] == 3 else MW.picture_units
    units = write(n, cut, mbw, mbh, L, False)
    slices = [k for k, (kind, _) in enumerate(units) if kind == "slice"]
    assert len(slices) == len(cut["slices"])
    for k, sl in zip(slices, cut["slices"]):
        if sl.get("header") is None:
            continue
        units[k] = ("slice", _with_extras(units[k][1], sl["header"], L))
    for kind, data in pic.get("extras", ()):
        if kind == "quant_matrix" and len(data) > 4:
            load_intra = (data[4] >> 3) & 1
            load_non = (data[4 + 64] >> 2) & 1 if load_intra and len(data) > 68 else (data[4] >> 2) & 1
            L["loads"].append((load_intra, load_non))
    return units


def stream(w, h, pictures, seq=None, end=True, stuff=None, tail=0, rows=None):
    """ilace_writer.stream over picture_units above; seq["progressive"] defaults to 1 here (a picture with field=True needs 0)"""
    seq = dict(seq or {})
    seq.setdefault("progressive", 0 if any(p.get("field") for p in pictures) else 1)
    mbw, mbh = (w + 15) // 16, rows or IW.mb_rows(h, seq["progressive"])
    L = new_log()
    units = []
    in_gop = 0
    for k, pic in enumerate(pictures):
        if pic.get("seq", k == 0):
            units += MW.sequence_units(w, h, seq)
        if pic.get("gop", k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x00 if pic.get("open_gop") else 0x40])))
            in_gop = 0
        units += picture_units(in_gop, pic, mbw, mbh, L)
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
