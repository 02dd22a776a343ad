"""A writer of MPEG-2 I / P streams for the device decoder's tests, and the streams written with it - the ones the oracle encoder never
writes: any header size, any quantiser code, DC differentials of every size, escapes of every run, saturating blocks, vector wraps,
hundreds of tiny pictures, one chunk of 37 MB, and zero stuffing that puts every kind of unit where the scan's tiles meet.

stream() generalises dec_cases.small(): the bits come from decoder.iso_tables() and desc_cases.seq_headers, nothing from the oracle
and nothing from what the device (or its host build) computes.  It returns the stream and a log of what it wrote; the CPU file
(tests/test_dec_cases.py) asserts from that log, not from a decoder, that each case holds what its name says.  valid() is the
assertion every stream meant as valid gets at construction: dec_cases.spec returns frames in both modes.  The two streams that
decoder.py needs minutes for (big_chunk, stuffed_2mib) are not asserted here but in the CPU file, which says how.

A picture is dict(type=1 | 2, slices=[...], gop=bool, seq=bool): gop - a GOP header in front (default: the first picture only),
seq - a repeated sequence header in front of that (2: the header twice).  A slice is dict(q=code, mbs=[...]) (code=, tail= for the refusals).  A macroblock
is dict(kind="intra" | "coded" | "not_coded", mv=(x, y) or delta=(mx, my), cbp=, blocks=[...]), a block dict(dc=differential,
coefs=[(run, level, force_escape)]); blocks lists the coded blocks in order."""
import functools

import numpy as np

import dec_cases as D
import desc_cases as DC

M = D.M
KINDS = D.UNIT_KINDS


@functools.lru_cache(maxsize=None)
def _tabs():
    t = M.decoder.iso_tables()
    out = {name: {sym: (code, length) for code, length, sym in t[name]} for name in ("motion", "cbp", "dcy", "dcc", "ac")}
    raster = [0] * 64                                          # scan position -> raster index
    for r, pos in enumerate(t["zigzag"]):
        raster[pos] = r
    out["raster"], out["intra_w"] = raster, list(t["intra_w"])
    return out


def inside(col, row, mv, mbw, mbh):
    """decoder._predict's assertion for a macroblock's luma block and - with the chroma vector of either mode - its chroma blocks"""
    def ok(x0, y0, vx, vy, n, W, H):
        ix, iy, hx, hy = vx >> 1, vy >> 1, vx & 1, vy & 1
        return x0 + ix >= 0 and y0 + iy >= 0 and y0 + iy + n - 1 + hy < H and x0 + ix + n - 1 + hx < W
    if not ok(16 * col, 16 * row, mv[0], mv[1], 16, 16 * mbw, 16 * mbh):
        return False
    return all(ok(8 * col, 8 * row, cx, cy, 8, 8 * mbw, 8 * mbh) for cx, cy in ((mv[0] >> 1, mv[1] >> 1), (int(mv[0] / 2), int(mv[1] / 2))))


def new_log():
    return dict(units=[], pictures=[], qcodes=[], mbs=[], dc=[], esc=[], blocks=[], stuffing=0)


def _put_block(w, blk, intra, comp, pred, L, strict):
    T = _tabs()
    k = 0
    if intra:
        diff = int(blk.get("dc", 0))
        size = abs(diff).bit_length()
        assert size <= 11
        w.code(T["dcc" if comp else "dcy"][size])
        if size:
            w.put(diff if diff > 0 else diff + (1 << size) - 1, size)
        pred[comp] += diff
        # (component, size, sign, the predictor behind and in front of it, the macroblock's place in the log)
        L["dc"].append((comp, size, (diff > 0) - (diff < 0), pred[comp], pred[comp] - diff, len(L["mbs"]) - 1))
        k = 1
    first = not intra
    levels = []
    for run, lvl, esc in blk.get("coefs", ()):
        k += run
        if strict:
            assert k < 64 and lvl != 0 and -2047 <= lvl <= 2047
        coded = (run, abs(lvl)) in T["ac"]
        if first and run == 0 and abs(lvl) == 1 and not esc:
            w.put(1, 1)
            w.put(lvl < 0, 1)
        elif coded and not esc:
            w.code(T["ac"][(run, abs(lvl))])
            w.put(lvl < 0, 1)
        else:
            w.put(1, 6)
            w.put(run, 6)
            w.put(lvl & 0xFFF, 12)
            L["esc"].append((run, lvl, intra, first, k, coded))
        levels.append((k, lvl))
        first = False
        k += 1
    if strict:
        assert not first, "a coded non-intra block needs a coefficient"
    w.put(2, 2)
    L["blocks"].append((intra, comp, levels))


def _put_mb(w, mb, ptype, col, row, mbw, mbh, st, L, strict):
    T = _tabs()
    kind = mb["kind"]
    for bit in mb.get("incr", "1") + mb.get("type_bits", ("1" if ptype == 1 else {"coded": "1", "not_coded": "001", "intra": "00011"}[kind])):
        w.put(int(bit), 1)
    if strict:
        assert kind == "intra" or ptype == 2
    mv, deltas, wraps, before = [0, 0], [0, 0], [0, 0], list(st["pmv"])
    if kind != "intra":
        for c in range(2):
            if "delta" in mb:
                m = mb["delta"][c]
            else:
                m = mb["mv"][c] - st["pmv"][c]
                m = m - 32 if m > 16 else m + 32 if m < -16 else m
            v = st["pmv"][c] + m
            if v < -16:
                v, wraps[c] = v + 32, -1
            elif v > 15:
                v, wraps[c] = v - 32, 1
            w.code(T["motion"][abs(m)])
            if m:
                w.put(m < 0, 1)
            st["pmv"][c] = mv[c] = v
            deltas[c] = m
        assert "mv" not in mb or tuple(mb["mv"]) == tuple(mv)
        if strict:
            assert inside(col, row, mv, mbw, mbh), (col, row, mv)
        st["dc"][:] = [0, 0, 0]
    else:
        st["pmv"][:] = [0, 0]
    cbp = 63 if kind == "intra" else mb["cbp"] if kind == "coded" else 0
    if kind == "coded":
        w.code(T["cbp"][cbp])
    blocks = iter(mb.get("blocks", ()))
    L["mbs"].append(dict(pic=len(L["pictures"]) - 1, row=row, col=col, kind=kind, mv=tuple(mv), delta=tuple(deltas), wrap=tuple(wraps), pmv=tuple(before), cbp=cbp))
    for b in range(6):
        if (cbp >> (5 - b)) & 1:
            _put_block(w, next(blocks), kind == "intra", 0 if b < 4 else b - 3, st["dc"], L, strict)


def picture_units(n, pic, mbw, mbh, L, strict):
    """[(kind, bytes)] of picture header, picture coding extension and slices (small()'s headers)"""
    ptype = pic["type"]
    out = []
    w = D._Writer()
    for value, width in ((0x00000100, 32), (n & 1023, 10), (ptype, 3), (0xFFFF, 16)) + (((0, 1), (7, 3)) if ptype == 2 else ()) + ((0, 1),):
        w.put(value, width)
    out.append(("picture", w.bytes()))
    w = D._Writer()
    for value, width in ((0x000001B5, 32), (8, 4), (1, 4), (1, 4), (15, 4), (15, 4), (2, 2), (3, 2), (0, 1), (1, 1), (0, 1), (0, 1), (0, 1), (0, 1),
                         (0, 1), (1, 1), (1, 1), (0, 1)):
        w.put(value, width)
    out.append(("picture_ext", w.bytes()))
    L["pictures"].append(ptype)
    L["qcodes"].append([sl["q"] for sl in pic["slices"]])
    if strict:
        assert len(pic["slices"]) == mbh
    for row, sl in enumerate(pic["slices"]):
        w = D._Writer()
        w.put(0x00000100 + sl.get("code", row + 1), 32)
        w.put(sl["q"], 5)
        w.put(0, 1)
        st = dict(pmv=[0, 0], dc=[0, 0, 0])
        if strict:
            assert len(sl["mbs"]) == mbw
        for col, mb in enumerate(sl["mbs"]):
            _put_mb(w, mb, ptype, col, min(row, mbh - 1), mbw, mbh, st, L, strict)
        for bit in sl.get("tail", ""):
            w.put(int(bit), 1)
        out.append(("slice", w.bytes()))
    return out


def assemble(units, stuff, L):
    out = bytearray()
    for k, (kind, data) in enumerate(units):
        z = stuff(k, kind, len(out)) if callable(stuff) else (stuff or {}).get(k, 0)
        out += bytes(z)
        L["stuffing"] += z
        L["units"].append((kind, len(out)))
        out += data
    out += bytes(-len(out) % 32)
    return bytes(out)


def stream(w, h, pictures, stuff=None, strict=True, d=DC.MODULE):
    """-> (stream, log).  stuff: {ordinal of a unit: zero bytes in front of it}, or a function (ordinal, kind, offset so far) -> count.
    strict=False writes what it is told (the refusals)."""
    if strict:
        assert 1 <= w <= 2048 and 1 <= h <= 2048
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    L = new_log()
    hdr = DC.seq_headers(w, h, d)
    assert hdr[12:16] == hdr[22:26] == b"\x00\x00\x01\xb5" and len(hdr) == 34
    seq = [("sequence", hdr[:12]), ("sequence_ext", hdr[12:22]), ("display_ext", hdr[22:])]
    units = []
    in_gop = frame = 0
    for k, pic in enumerate(pictures):
        units += seq * int(pic.get("seq", k == 0))
        if pic.get("gop", pic.get("seq", False) or k == 0):
            units.append(("gop", b"\x00\x00\x01\xb8" + DC.time_code(frame, d["frame_rate_code"])))
            in_gop = 0
        units += picture_units(in_gop, pic, mbw, mbh, L, strict)
        in_gop, frame = in_gop + 1, frame + 1
    units.append(("end", b"\x00\x00\x01\xb7"))
    return assemble(units, stuff, L), L


_decoded = {}


def valid(s):
    """the assertion at construction: the definition returns frames in both modes (kept for expected())"""
    for quirks in (True, False):
        d, why = D.spec(s, quirks)
        assert d is not None, why
        _decoded[(s, quirks)] = d
    return s


def expected(s, mode, layout="i420"):
    """decoder.decode's frames of a stream in the layout, as m2v_decode_device must write them"""
    quirks = mode == "module"
    if (s, quirks) not in _decoded:
        _decoded[(s, quirks)] = M.decoder.decode(s, quirks=quirks)
    return D.frames_of(_decoded[(s, quirks)], layout)


# ---- content ----
def random_block(rng, intra, dc=60, most=5):
    """small()'s kind of block: a few run / level pairs - table codes and, one time in eight, a level nine times as large (an escape)"""
    coefs, k = [], 1 if intra else 0
    for _ in range(int(rng.randint(1, most))):
        run, lvl = int(rng.randint(0, 6)), int(rng.randint(1, 9)) * (1 if rng.randint(2) else -1)
        if k + run > 63:
            break
        if rng.randint(8) == 0:
            lvl *= 9
        coefs.append((run, lvl, False))
        k += run + 1
    if not intra and not coefs:
        coefs = [(0, 1, False)]
    return dict(dc=int(rng.randint(-dc, dc + 1)), coefs=coefs)


def legal_vector(rng, col, row, mbw, mbh, most=16):
    for _ in range(8):
        mv = (int(rng.randint(-most, most)), int(rng.randint(-most, most)))
        if inside(col, row, mv, mbw, mbh):
            return mv
    mv = (int(rng.randint(0, 4)) * (1 if col == 0 else -1), int(rng.randint(0, 4)) * (1 if row == 0 else -1))
    return mv if inside(col, row, mv, mbw, mbh) else (0, 0)


def random_picture(rng, ptype, mbw, mbh, q=4, gop=None, seq=None):
    slices = []
    for row in range(mbh):
        mbs = []
        for col in range(mbw):
            kind = "intra" if ptype == 1 else ("coded", "coded", "not_coded", "intra")[int(rng.randint(4))]
            mb = dict(kind=kind)
            if kind != "intra":
                mb["mv"] = legal_vector(rng, col, row, mbw, mbh)
            if kind == "coded":
                mb["cbp"] = int(rng.randint(1, 64))
            n = 6 if kind == "intra" else bin(mb.get("cbp", 0)).count("1")
            mb["blocks"] = [random_block(rng, kind == "intra") for _ in range(n)]
            mbs.append(mb)
        slices.append(dict(q=q(row) if callable(q) else q, mbs=mbs))
    pic = dict(type=ptype, slices=slices)
    if gop is not None:
        pic["gop"] = gop
    if seq is not None:
        pic["seq"] = seq
    return pic


def moved_picture(mbw, mbh, vector, gop=None, seq=None):
    """a P picture of not-coded macroblocks; vector(col, row) -> (x, y)"""
    pic = dict(type=2, slices=[dict(q=1, mbs=[dict(kind="not_coded", mv=vector(col, row)) for col in range(mbw)]) for row in range(mbh)])
    if gop is not None:
        pic["gop"] = gop
    if seq is not None:
        pic["seq"] = seq
    return pic


def inward(mbw, mbh, k, most=5):
    """vectors of picture k that point into the picture from every macroblock, up to most - 1 half samples, both phases"""
    def vector(col, row):
        x = (k + col) % most * (1 if 2 * col < mbw else -1)
        y = (k + 2 * row) % most * (1 if 2 * row < mbh else -1)
        return (x if mbw > 1 else 0, y if mbh > 1 else 0)
    return vector


# ---- the directed valid cases ----
@functools.lru_cache(maxsize=None)
def qcodes():
    """16 x 512, one I and one P picture of 32 slices: slice k carries quantiser code k.  Levels of +-61 on intra coefficients of
    weight 16 give 2 * 61 * code = 1952 at code 16 and 2074 at 17; +-60 in non-intra blocks give 121 * code = 1936 and 2057"""
    def intra(row):
        return dict(dc=(row % 5 - 2) * 20, coefs=[(0, 61, False), (0, -61, False), (1, 7, False), (2, -300, False), (0, 300, False)])

    def inter(row):
        return dict(coefs=[(0, 60, False), (0, -60, False), (3, 1, False), (0, -2, False), (1, 70, False), (0, -70, False)])
    i = dict(type=1, slices=[dict(q=k, mbs=[dict(kind="intra", blocks=[intra(k)] * 6)]) for k in range(32)])
    p = dict(type=2, slices=[dict(q=k, mbs=[dict(kind="coded", mv=(0, (k % 7) - 3 if 0 < k < 31 else 0), cbp=63, blocks=[inter(k)] * 6)]) for k in range(32)])
    s, L = stream(16, 512, [i, p])
    return valid(s), L


DC_BIG = [2047] * 6 + [-2047] * 12 + [2047] * 4 + [1024, -1024, 1023, -1023, 512, -512, 511, -511, 256, -256]      # 32: the luma of picture 0
DC_MID = [300, -300, 600, -600, -300, 300, -600, 600] * 2                  # sizes 9 and 10: the chroma of picture 2
DC_SMALL_C = [0, 1, -1, 3, -3, 7, -7, 15, -15, 31, -31, 63, -63, 127, -127, 255, -255]      # 17: the chroma of pictures 1 and 3
DC_SMALL = [0, 1, -1, 2, -2, 3, -3, 4, -4, 7, -7, 8, -8, 15, -15, 16, -16, 31, -31, 32, -32, 63, -63, 64, -64, 127, -127, 128, -128, 255, -255, 0]


@functools.lru_cache(maxsize=None)
def dc_range():
    """64 x 32.  Picture 0 (I): differentials of +-2047 one after another - the luma predictor runs to +12 282, down to -12 282 and
    back, the chroma ones past +-6 000 - then the size boundaries down to 255.  Picture 1 (P): intra, MC coded, intra in one slice
    (the predictor is reset in between) with differentials small enough that nothing saturates.  Picture 2 (I): every size 0 .. 8 with
    both signs in luma, 9 and 10 in chroma, the second slice starting from the reset predictor.  Picture 3 (I): the small chroma sizes.
    Picture 0's blocks hold two large AC levels as well: a DC beyond the saturation alone drives every sample to 0 or 255 whether
    M2V_DEC_ISO clips F[0] or not; with them some samples come back into range"""
    big_y, small, mid, small_c = iter(DC_BIG), iter(DC_SMALL * 8), iter(DC_MID), iter(DC_SMALL_C * 2)
    big_c = iter([2047, 2047, 2047, -2047, 2047, -2047, 1024, -1024] + [-2047, -2047, -2047, 2047, -2047, 2047, -1024, 1024])

    def intra(y, c, ac=()):
        return dict(kind="intra", blocks=[dict(dc=next(y), coefs=list(ac)) for _ in range(4)] + [dict(dc=next(c), coefs=list(ac)) for _ in range(2)])
    ac = ((0, 3, False), (2, -2, False))
    p0 = dict(type=1, slices=[dict(q=2, mbs=[intra(big_y, big_c, ((0, 300, False), (0, -280, False))) for _ in range(4)]) for _ in range(2)])
    inter = dict(kind="coded", mv=(0, 0), cbp=0b100110, blocks=[dict(coefs=[(0, 5, False)])] * 3)
    p1 = dict(type=2, slices=[dict(q=2, mbs=[intra(small, small_c, ac), inter, intra(small, small_c, ac), dict(kind="not_coded", mv=(0, 0))]),
                              dict(q=3, mbs=[intra(small, small_c), intra(small, small_c, ac), dict(kind="not_coded", mv=(-2, -1)), intra(small, small_c)])])
    p2 = dict(type=1, slices=[dict(q=2, mbs=[intra(small, mid, ac) for _ in range(4)]) for _ in range(2)])
    p3 = dict(type=1, slices=[dict(q=4, mbs=[intra(small, small_c, ac) for _ in range(4)]) for _ in range(2)])
    s, L = stream(64, 32, [p0, p1, p2, p3])
    return valid(s), L


@functools.lru_cache(maxsize=None)
def escapes():
    """64 x 64, one I and two P pictures of coded macroblocks: every run 0 .. 63 as an escape at levels +1, -1, +2047, -2047 (runs up to
    31 at +-1 have a table code too) - 96 of them alone in an intra block, the others first in a non-intra block, run 63 and the
    intra run 62 landing on index 63; the blocks left over hold '1s', table codes and escapes behind one another"""
    combos = [(run, lvl) for lvl in (1, -2047, -1, 2047) for run in range(64)]
    intra = [c for c in combos if c[0] <= 62][:96]
    inter = [c for c in combos if c not in intra]
    assert len(inter) == 160
    rng = np.random.RandomState(11)
    extra = [dict(coefs=[(0, 1 if k % 2 else -1, False), (k % 7, 3 + k, True), (0, -2047, True), (62 - k % 7 - 2, 2, True)]) for k in range(32)]
    blocks_i = iter(dict(dc=int(rng.randint(-40, 41)), coefs=[(run, lvl, True)]) for run, lvl in intra)
    blocks_p = iter([dict(coefs=[(run, lvl, True)]) for run, lvl in inter] + extra)
    pics = [dict(type=1, slices=[dict(q=1 + row, mbs=[dict(kind="intra", blocks=[next(blocks_i) for _ in range(6)]) for _ in range(4)]) for row in range(4)])]
    for n in range(2):
        pics.append(dict(type=2, slices=[dict(q=1 + 4 * n + row, mbs=[dict(kind="coded", mv=(0, 0), cbp=63, blocks=[next(blocks_p) for _ in range(6)])
                                                                   for _ in range(4)]) for row in range(4)]))
    s, L = stream(64, 64, pics)
    return valid(s), L


SIGNS = {"plus": lambda x, y: 1, "minus": lambda x, y: -1, "alternating": lambda x, y: 1 - 2 * ((x + y) & 1), "alternating_minus": lambda x, y: 2 * ((x + y) & 1) - 1,
         "by_row": lambda x, y: 1 - 2 * (y & 1), "by_column": lambda x, y: 1 - 2 * (x & 1)}


@functools.lru_cache(maxsize=None)
def saturate():
    """16 x 48, one I and one P picture, quantiser codes 1, 16 and 31 down the slices: every block holds 64 coefficients of +-2047 (an
    intra block: a DC differential of +-2047 and 63 escapes), the six blocks of a macroblock in the six sign patterns of SIGNS"""
    raster = _tabs()["raster"]

    def block(name, intra):
        sign = [SIGNS[name](raster[k] & 7, raster[k] >> 3) for k in range(64)]
        return dict(dc=2047 * sign[0], coefs=[(0, 2047 * sign[k], True) for k in range(1 if intra else 0, 64)])
    pics = []
    for ptype in (1, 2):
        mb = dict(kind="intra") if ptype == 1 else dict(kind="coded", mv=(0, 0), cbp=63)
        pics.append(dict(type=ptype, slices=[dict(q=q, mbs=[dict(mb, blocks=[block(name, ptype == 1) for name in SIGNS])]) for q in (1, 16, 31)]))
    s, L = stream(16, 48, pics)
    return valid(s), L


@functools.lru_cache(maxsize=None)
def pmv_chain():
    """48 x 48, an I picture and two P pictures written as motion codes (delta=), so that the log says where a component wrapped.
    Picture 1: row 0 carries (4, 2) across two not-coded macroblocks and ends at (-2, 2); row 1 starts from the reset prediction with
    (15, 15), adds (+1, +1) -> (-16, -16), adds (-16, -16) -> (0, 0); row 2 has an intra macroblock between two coded ones.
    Picture 2, row 1: (0, -16), then (-16, -1) -> (-16, 15), then (-16, +1) -> (0, -16)"""
    rng = np.random.RandomState(5)

    def mc(kind, delta):
        mb = dict(kind=kind, delta=delta)
        if kind == "coded":
            mb.update(cbp=0b101001, blocks=[random_block(rng, False) for _ in range(3)])
        return mb
    intra = lambda: dict(kind="intra", blocks=[random_block(rng, True) for _ in range(6)])
    p1 = dict(type=2, slices=[dict(q=3, mbs=[mc("not_coded", (4, 2)), mc("not_coded", (0, 0)), mc("coded", (-6, 0))]),
                              dict(q=3, mbs=[mc("coded", (15, 15)), mc("not_coded", (1, 1)), mc("coded", (-16, -16))]),
                              dict(q=3, mbs=[mc("coded", (6, -4)), intra(), mc("coded", (-3, -2))])])
    p2 = dict(type=2, slices=[dict(q=2, mbs=[mc("coded", (3, 5)), mc("not_coded", (-3, -5)), mc("not_coded", (-7, 1))]),
                              dict(q=2, mbs=[mc("not_coded", (0, -16)), mc("coded", (-16, -1)), mc("not_coded", (-16, 1))]),
                              dict(q=2, mbs=[mc("not_coded", (2, -2)), mc("not_coded", (0, 0)), mc("not_coded", (-4, -4))])])
    s, L = stream(48, 48, [random_picture(rng, 1, 3, 3), p1, p2])
    return valid(s), L


SIZES = ((1, 1), (2, 2), (15, 17), (16, 16), (17, 33), (2047, 1), (1, 2047), (2048, 16), (16, 2048))
SMALL_SIZES = SIZES[:5]


@functools.lru_cache(maxsize=None)
def sized(w, h):
    """seeded small()-like content at header size w x h: an I and a P picture; 1 x 1 has 13 pictures, I at 0, 5 and 6, in two GOPs"""
    rng = np.random.RandomState(1000 * w + h)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    types = (1, 2, 2, 2, 2, 1, 1, 2, 2, 2, 2, 2, 2) if (w, h) == (1, 1) else (1, 2)
    pics = [random_picture(rng, t, mbw, mbh, q=lambda row: 1 + row % 9, gop=(k in (0, 6))) for k, t in enumerate(types)]
    s, L = stream(w, h, pics)
    return valid(s), L


def bad_size(w, h):
    """small() with another size in its sequence header (0 and 2049 are outside what the device decodes: m2v_mi355x.h)"""
    s = D.small()
    return DC.seq_headers(w, h, DC.MODULE) + s[34:]


MANY_I = (0, 37, 38, 120, 255, 256, 257, 333)


@functools.lru_cache(maxsize=None)
def many_pictures():
    """32 x 16, 400 pictures: I at MANY_I, each behind a GOP header (37 and 257 behind a repeated sequence header too), the rest P
    pictures of two not-coded macroblocks with vectors (1 .. 3, 0) and (-1 .. -4, 0)"""
    rng = np.random.RandomState(21)
    pics = []
    for k in range(400):
        if k in MANY_I:
            pics.append(random_picture(rng, 1, 2, 1, gop=True, seq=k in (0, 37, 257)))
        else:
            pics.append(moved_picture(2, 1, lambda col, row: (k % 3 + 1, 0) if col == 0 else (-(k % 4) - 1, 0), gop=False))
    s, L = stream(32, 16, pics)
    return valid(s), L


BIG = dict(w=320, h=304, n=256)


@functools.lru_cache(maxsize=None)
def big_chunk(n=None):
    """320 x 304, 256 pictures: an I picture, then not-coded P pictures whose vectors point inward, 0 .. 4 half samples, different in
    every picture - 37 355 520 bytes of I420 in one default chunk.  n: only the first n pictures (the CPU file's prefix).
    Not asserted at construction: decoder.py needs about 200 s a mode"""
    mbw, mbh = BIG["w"] // 16, BIG["h"] // 16
    rng = np.random.RandomState(31)
    pics = [random_picture(rng, 1, mbw, mbh)] + [moved_picture(mbw, mbh, inward(mbw, mbh, k), gop=False) for k in range(1, n or BIG["n"])]
    return stream(BIG["w"], BIG["h"], pics)


# ---- stuffing ----
def _stuffed_pictures(seed):
    """small()'s shape - 32 x 32, an I and a P picture - and behind them a repeated sequence header, a GOP header and a third picture (P)"""
    rng = np.random.RandomState(seed)
    return [random_picture(rng, 1, 2, 2), random_picture(rng, 2, 2, 2), random_picture(rng, 2, 2, 2, seq=True)]


def _place(T, shift, inner):
    """a stuffing function: the last unit of every kind begins `shift` bytes from the next multiple of T (inner: of 16, and away from
    the multiples of T)"""
    units = [k for k, _ in stream(32, 32, _stuffed_pictures(0))[1]["units"]]
    last = {kind: max(j for j, k in enumerate(units) if k == kind) for kind in KINDS}

    def stuff(k, kind, at):
        if last[kind] != k:
            return 0
        step = 16 if inner else T
        want = -(-(at - shift) // step) * step + shift
        while inner and not 16 <= (want + 3) % T < T - 16:
            want += 16
        return want - at
    return stuff


@functools.lru_cache(maxsize=None)
def stuffed(T=4096):
    """eight streams: in stream j = 0 .. 3 the last unit of every kind begins at j - 3 from a multiple of the scan's tile T, in stream
    4 + j at j - 3 from a multiple of 16 inside a tile.  -> ((stream, log), ...)"""
    out = []
    for j in range(8):
        s, L = stream(32, 32, _stuffed_pictures(40 + j), stuff=_place(T, j % 4 - 3, j >= 4))
        out.append((valid(s), L))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stuffed_2mib(T=4096, stuffing=True):
    """over 512 tiles: the I picture's header three bytes in front of tile 512 (its slices are in tile 512), the P picture in tile 513,
    the repeated sequence header, the GOP header and the third picture in tile 514.  stuffing=False: the same units with none.
    Not asserted at construction (decoder.py reads the zeros for 20 s a mode): the CPU file does"""
    pics = _stuffed_pictures(77)
    units = [k for k, _ in stream(32, 32, pics)[1]["units"]]
    first_picture, second_picture, repeat = units.index("picture"), [j for j, k in enumerate(units) if k == "picture"][1], [j for j, k in enumerate(units) if k == "sequence"][1]
    where = {first_picture: 512 * T - 3, second_picture: 513 * T + 100, repeat: 514 * T + 7}
    return stream(32, 32, pics, stuff=(lambda k, kind, at: where[k] - at if k in where else 0) if stuffing else None)


# ---- the refusals ----
def _p_only(n, seq=1):
    """n P pictures of 32 x 16 and no I picture; seq: how many sequence headers stand in front"""
    return [moved_picture(2, 1, lambda col, row: (0, 0), gop=(k == 0), seq=(seq if k == 0 else None)) for k in range(n)]


# name -> (picture, macroblock row) of the slice the fault is written into
REFUSED_IN = {"index_64_intra": (0, 1), "index_64_inter": (1, 1), "escape_level_0": (0, 1), "escape_level_-2048": (1, 1), "eob_first_inter": (1, 1),
              "mb_type_01": (1, 0), "increment_2": (0, 1), "increment_2_p": (1, 1), "vector_left": (1, 0), "vector_right": (1, 0), "vector_top": (1, 0),
              "vector_bottom": (1, 1), "slice_stuffing_bit": (0, 0), "slice_stuffing_byte": (0, 0)}


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> stream, each refused by decoder.py in both modes (the CPU file asserts it).  32 x 32, small()'s shape"""
    rng = np.random.RandomState(3)
    out = {}

    def base():                                                  # an I and a P picture, the same for every case
        r = np.random.RandomState(9)
        return [random_picture(r, 1, 2, 2), random_picture(r, 2, 2, 2)]

    def with_block(blk, intra):
        pics = base()
        mb = pics[0 if intra else 1]["slices"][1]["mbs"][0]
        if not intra:
            mb.update(kind="coded", mv=(0, 0), cbp=0b100000)
            mb.pop("delta", None)
        mb["blocks"] = [blk] + ([random_block(rng, True) for _ in range(5)] if intra else [])
        return stream(32, 32, pics, strict=False)[0]
    out["index_64_intra"] = with_block(dict(dc=3, coefs=[(62, 2, False), (0, 1, False)]), True)
    out["index_64_inter"] = with_block(dict(coefs=[(31, 1, False), (31, 1, False), (0, 1, False)]), False)
    out["escape_level_0"] = with_block(dict(dc=3, coefs=[(2, 0, True)]), True)
    out["escape_level_-2048"] = with_block(dict(coefs=[(2, -2048, True)]), False)
    out["eob_first_inter"] = with_block(dict(coefs=[]), False)

    def with_mb(picture, row, col, **change):
        pics = base()
        pics[picture]["slices"][row]["mbs"][col].update(change)
        return stream(32, 32, pics, strict=False)[0]
    out["mb_type_01"] = with_mb(1, 0, 1, kind="coded", mv=(0, 0), cbp=0b010000, blocks=[dict(coefs=[(0, 2, False)])], type_bits="01")
    out["increment_2"] = with_mb(0, 1, 1, incr="011")
    out["increment_2_p"] = with_mb(1, 1, 0, incr="011")
    moved = dict(kind="not_coded", blocks=[])
    out["vector_left"] = with_mb(1, 0, 0, mv=(-1, 0), **moved)
    out["vector_right"] = with_mb(1, 0, 1, mv=(1, 0), **moved)
    out["vector_top"] = with_mb(1, 0, 1, mv=(0, -1), **moved)
    out["vector_bottom"] = with_mb(1, 1, 0, mv=(0, 1), **moved)
    pics = base()
    pics[1]["slices"].append(dict(q=2, code=3, mbs=pics[1]["slices"][1]["mbs"]))
    out["slice_code_mbh_plus_1"] = stream(32, 32, pics, strict=False)[0]
    pics = base()
    pics[0]["slices"][0]["tail"] = "1"
    a = stream(32, 32, pics, strict=False)[0]
    pics[0]["slices"][0]["tail"] = "10000000"                   # (whichever leaves a whole byte 0x80 or a bit in the last byte)
    out["slice_stuffing_bit"], out["slice_stuffing_byte"] = a, stream(32, 32, pics, strict=False)[0]
    # no reference: a P picture behind the sequence header and a repeated one; and 150 P pictures, 455 start codes - every P picture
    # lacks its reference, every lane of the plan reports its own, and the offset is the first picture's
    out["p_behind_repeated_header"] = stream(32, 16, _p_only(1, seq=2), strict=False)[0]
    out["p_pictures_only"] = stream(32, 16, _p_only(150), strict=False)[0]
    return out
