"""A small MPEG-2 video elementary-stream decoder written from the ISO/IEC 13818-2 syntax (clause 6.2) and
decoding process (clause 7), for the subset this encoder emits: frame pictures, I and P, 4:2:0, frame prediction
with one forward vector, f_code 1, intra_vlc_format 0, zig-zag scan, q_scale_type 0, default matrices.

It is an INDEPENDENT check of the stream layer (every header field, macroblock types, vector and DC prediction, the
run/level coding, end-of-slice padding) and, with `quirks=True`, of the encoder's reconstruction loop: the RTL
deviates from ISO in a few places and a conformant decoder would drift from the encoder's own
reference frames, so the quirks can be switched on to reproduce the encoder's reconstruction exactly:
   * half-pel 4-sample average rounds with +1 instead of +2                      (RTL:764)
   * chroma vector = floor(mv / 2) instead of mv / 2 truncated toward zero       (RTL:1854-1916)
   * intra AC dequantisation floors negatives; no mismatch control               (RTL:2132-2148)
   * IDCT = Chen-Wang with an 18-bit row store and a +-255 output clip           (RTL:844-972)
Everything here, the VLC tables of Annex B included, is written from the standard: nothing is shared with the
encoder, the oracle or the RTL.  It is an analysis tool (tools/m2v_stats.py: PSNR of a stream against its source) and
the independent checker of the parity tests; it runs on the CPU and is not on the encode path.
"""
import numpy as np


class BitReader:
    def __init__(self, data):
        self.d = data
        self.pos = 0                 # bit position

    def bits(self, n):
        v = 0
        for _ in range(n):
            byte = self.d[self.pos >> 3]
            v = (v << 1) | ((byte >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def peek(self, n):
        p = self.pos
        v = self.bits(n)
        self.pos = p
        return v

    def aligned(self):
        return (self.pos & 7) == 0

    def align(self):
        pad = (-self.pos) & 7
        assert self.bits(pad) == 0, "non-zero stuffing before a start code"

    def next_start_code(self):
        """next_start_code(): zero stuffing to the byte boundary, then zero bytes, then 0x000001"""
        self.align()
        while self.peek(24) != 1:
            assert self.bits(8) == 0, "garbage before a start code"
        return self.peek(32) & 0xFF


def _vlc_decoder(entries):
    """entries: list of (code, length, symbol) -> function(BitReader) -> symbol"""
    table = {}
    for code, length, sym in entries:
        assert (length, code) not in table, "duplicate code"
        table[(length, code)] = sym
    maxlen = max(l for _, l, _ in entries)
    for (l1, c1) in table:                                # a VLC table must be prefix free
        for l2 in range(1, l1):
            assert (l2, c1 >> (l1 - l2)) not in table, "code %s/%d has a prefix in the table" % (bin(c1), l1)

    def dec(br):
        v = 0
        for l in range(1, maxlen + 1):
            v = (v << 1) | br.bits(1)
            if (l, v) in table:
                return table[(l, v)]
        raise ValueError("invalid VLC at bit %d" % br.pos)
    return dec


# ---------------------------------------------------------------------------------------------------------------
# ISO/IEC 13818-2 Annex B, typed in from the standard's tables (NOT taken from the encoder, the oracle or the RTL:
# tests/test_decoder_tables.py checks that the three agree entry by entry)
# ---------------------------------------------------------------------------------------------------------------
_B10_MOTION = """0:1 1:01 2:001 3:0001 4:000011 5:0000101 6:0000100 7:0000011 8:000001011 9:000001010 10:000001001
11:0000010001 12:0000010000 13:0000001111 14:0000001110 15:0000001101 16:0000001100"""

_B12_DC_LUMA = "0:100 1:00 2:01 3:101 4:110 5:1110 6:11110 7:111110 8:1111110 9:11111110 10:111111110 11:111111111"
_B13_DC_CHROMA = "0:00 1:01 2:10 3:110 4:1110 5:11110 6:111110 7:1111110 8:11111110 9:111111110 10:1111111110 11:1111111111"

_B9_CBP = """60:111 4:1101 8:1100 16:1011 32:1010 12:10011 48:10010 20:10001 40:10000 28:01111 44:01110 52:01101 56:01100
1:01011 61:01010 2:01001 62:01000 24:001111 36:001110 3:001101 63:001100 5:0010111 9:0010110 17:0010101 33:0010100
6:0010011 10:0010010 18:0010001 34:0010000 7:00011111 11:00011110 19:00011101 35:00011100 13:00011011 49:00011010
21:00011001 41:00011000 14:00010111 50:00010110 22:00010101 42:00010100 15:00010011 51:00010010 23:00010001 43:00010000
25:00001111 37:00001110 26:00001101 38:00001100 29:00001011 45:00001010 53:00001001 57:00001000 30:00000111 46:00000110
54:00000101 58:00000100 31:000000111 47:000000110 55:000000101 59:000000100 27:000000011 39:000000010"""

# Table B-14 (DCT coefficients table zero), "run,level:code" without the sign bit; (0,1) is listed in its
# "not first coefficient" form '11' - the first-coefficient form '1s' is handled in the block loop
_B14_AC = """0,1:11 1,1:011 0,2:0100 2,1:0101 0,3:00101 3,1:00111 4,1:00110 1,2:000110 5,1:000111 6,1:000101 7,1:000100
0,4:0000110 2,2:0000100 8,1:0000111 9,1:0000101
0,5:00100110 0,6:00100001 1,3:00100101 3,2:00100100 10,1:00100111 11,1:00100011 12,1:00100010 13,1:00100000
0,7:0000001010 1,4:0000001100 2,3:0000001011 4,2:0000001111 5,2:0000001001 14,1:0000001110 15,1:0000001101 16,1:0000001000
0,8:000000011101 0,9:000000011000 0,10:000000010011 0,11:000000010000 1,5:000000011011 2,4:000000010100 3,3:000000011100
4,3:000000010010 6,2:000000011110 7,2:000000010101 8,2:000000010001 17,1:000000011111 18,1:000000011010 19,1:000000011001
20,1:000000010111 21,1:000000010110
0,12:0000000011010 0,13:0000000011001 0,14:0000000011000 0,15:0000000010111 1,6:0000000010110 1,7:0000000010101
2,5:0000000010100 3,4:0000000010011 5,3:0000000010010 9,2:0000000010001 10,2:0000000010000 22,1:0000000011111
23,1:0000000011110 24,1:0000000011101 25,1:0000000011100 26,1:0000000011011
0,16:00000000011111 0,17:00000000011110 0,18:00000000011101 0,19:00000000011100 0,20:00000000011011 0,21:00000000011010
0,22:00000000011001 0,23:00000000011000 0,24:00000000010111 0,25:00000000010110 0,26:00000000010101 0,27:00000000010100
0,28:00000000010011 0,29:00000000010010 0,30:00000000010001 0,31:00000000010000
0,32:000000000011000 0,33:000000000010111 0,34:000000000010110 0,35:000000000010101 0,36:000000000010100
0,37:000000000010011 0,38:000000000010010 0,39:000000000010001 0,40:000000000010000 1,8:000000000011111
1,9:000000000011110 1,10:000000000011101 1,11:000000000011100 1,12:000000000011011 1,13:000000000011010 1,14:000000000011001
1,15:0000000000010011 1,16:0000000000010010 1,17:0000000000010001 1,18:0000000000010000 6,3:0000000000010100
11,2:0000000000011010 12,2:0000000000011001 13,2:0000000000011000 14,2:0000000000010111 15,2:0000000000010110
16,2:0000000000010101 27,1:0000000000011111 28,1:0000000000011110 29,1:0000000000011101 30,1:0000000000011100
31,1:0000000000011011"""
_B14_EOB, _B14_ESCAPE = "10", "000001"

# Table B-15 (DCT coefficients table one, intra blocks of a picture with intra_vlc_format 1): the 41 codes that differ from B-14's;
# every B-14 code that begins with seven zero bits is B-15's too, except those of _B15_MOVED, whose B-14 codewords begin no code here
_B15_AC = """0,1:10 0,2:110 0,3:0111 0,4:11100 0,5:11101 0,6:000101 0,7:000100 0,8:1111011 0,9:1111100 0,10:00100011 0,11:00100010
0,12:11111010 0,13:11111011 0,14:11111110 0,15:11111111 1,1:010 1,2:00110 1,3:1111001 1,4:00100111 1,5:00100000
2,1:00101 2,2:0000111 2,3:11111100 2,4:0000001100 3,1:00111 3,2:00100110 4,1:000110 4,2:11111101 5,1:000111 5,2:000000100
6,1:0000110 7,1:0000100 8,1:0000101 9,1:1111000 10,1:1111010 11,1:00100001 12,1:00100101 13,1:00100100
14,1:000000101 15,1:000000111 16,1:0000001101"""
_B15_EOB = "0110"
_B15_MOVED = [(0, l) for l in range(8, 16)] + [(1, 5), (2, 4)]

# 7.3 figure 7-2: zig-zag scan (alternate_scan = 0), scan position of raster [v][u]
_ZIGZAG = [0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
           10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63]
# 6.3.11: default intra quantiser matrix, raster [v][u]
_INTRA_W = [8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
            22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83]


def _parse(text, key=int):
    """'sym:bits sym:bits ...' -> [(code, length, sym)]"""
    out = []
    for item in text.split():
        sym, bits = item.split(":")
        out.append((int(bits, 2), len(bits), key(sym)))
    return out


def iso_tables():
    """The raw Annex B tables as lists of (code, length, symbol); used by tests/test_decoder_tables.py"""
    ac = _parse(_B14_AC, key=lambda t: tuple(int(x) for x in t.split(",")))
    return dict(motion=_parse(_B10_MOTION), cbp=_parse(_B9_CBP), dcy=_parse(_B12_DC_LUMA), dcc=_parse(_B13_DC_CHROMA), ac=ac,
                zigzag=list(_ZIGZAG), intra_w=list(_INTRA_W))


def b15_table():
    """Table B-15 as [(code, length, (run, level))], without end of block and escape"""
    pair = lambda t: tuple(int(x) for x in t.split(","))
    own = _parse(_B15_AC, key=pair)
    shared = [e for e in _parse(_B14_AC, key=pair) if e[1] > 7 and e[0] >> (e[1] - 7) == 0 and e[2] not in _B15_MOVED]
    return own + shared


def _tables():
    t = iso_tables()
    ac = [e for e in t["ac"] if e[2] != (0, 1)]          # '11' is matched before the table look-up (see the block loop)
    ac.append((int(_B14_EOB, 2), len(_B14_EOB), "EOB"))
    ac.append((int(_B14_ESCAPE, 2), len(_B14_ESCAPE), "ESC"))
    zz = np.zeros(64, np.int64)                          # scan position -> raster index
    for raster, pos in enumerate(_ZIGZAG):
        zz[pos] = raster
    ac15 = b15_table() + [(int(_B15_EOB, 2), len(_B15_EOB), "EOB"), (int(_B14_ESCAPE, 2), len(_B14_ESCAPE), "ESC")]
    return dict(motion=_vlc_decoder(t["motion"]), cbp=_vlc_decoder(t["cbp"]), dcy=_vlc_decoder(t["dcy"]),
                dcc=_vlc_decoder(t["dcc"]), ac=_vlc_decoder(ac), ac15=_vlc_decoder(ac15), zz=zz, W=np.array(_INTRA_W, np.int64))


_T = None


def tables():
    global _T
    if _T is None:
        _T = _tables()
    return _T


# ---------------------------------------------------------------------------------------------------------------
# inverse DCT
# ---------------------------------------------------------------------------------------------------------------
def _s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def _sext(x, bits):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565


def _idct_1d(a, row, quirks):
    """mpeg2decode's idctrow / idctcol (Chen-Wang), 32-bit arithmetic"""
    if row:
        x0, x1 = _s32((a[0] << 11) + 128), _s32(a[4] << 11)
    else:
        x0, x1 = _s32((a[0] << 8) + 8192), _s32(a[4] << 8)
    x2, x3, x4, x5, x6, x7 = a[6], a[2], a[1], a[7], a[5], a[3]
    r = 0 if row else 4
    sh = 0 if row else 3
    x8 = _s32(W7 * (x4 + x5) + r)
    x4 = _s32(x8 + (W1 - W7) * x4) >> sh
    x5 = _s32(x8 - (W1 + W7) * x5) >> sh
    x8 = _s32(W3 * (x6 + x7) + r)
    x6 = _s32(x8 - (W3 - W5) * x6) >> sh
    x7 = _s32(x8 - (W3 + W5) * x7) >> sh
    x8 = _s32(x0 + x1)
    x0 = _s32(x0 - x1)
    x1 = _s32(W6 * (x3 + x2) + r)
    x2 = _s32(x1 - (W2 + W6) * x2) >> sh
    x3 = _s32(x1 + (W2 - W6) * x3) >> sh
    x1 = _s32(x4 + x6)
    x4 = _s32(x4 - x6)
    x6 = _s32(x5 + x7)
    x5 = _s32(x5 - x7)
    x7 = _s32(x8 + x3)
    x8 = _s32(x8 - x3)
    x3 = _s32(x0 + x2)
    x0 = _s32(x0 - x2)
    x2 = _s32(181 * (x4 + x5) + 128) >> 8
    x4 = _s32(181 * (x4 - x5) + 128) >> 8
    out = [x7 + x1, x3 + x2, x0 + x4, x8 + x6, x8 - x6, x0 - x4, x3 - x2, x7 - x1]
    out = [_s32(v) >> (8 if row else 14) for v in out]
    if row:
        return [_sext(v, 18) for v in out] if quirks else out
    lo = -255 if quirks else -256
    return [max(lo, min(255, v)) for v in out]


def idct(F, quirks):
    rows = [_idct_1d([int(v) for v in F[i * 8:i * 8 + 8]], True, quirks) for i in range(8)]
    out = np.zeros(64, np.int64)
    for j in range(8):
        col = _idct_1d([rows[i][j] for i in range(8)], False, quirks)
        for i in range(8):
            out[i * 8 + j] = col[i]
    return out


# ---------------------------------------------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------------------------------------------
class Decoded:
    def __init__(self):
        self.frames = []            # (Y, U, V) uint8 arrays
        self.pictures = []          # dicts of header fields
        self.mbs = []               # per picture: list of dict(type, mv, cbp)
        self.width = self.height = 0
        self.gops = []
        self.slice_qcodes = []      # per picture: the quantiser_scale_code of every slice, top to bottom (1 << level: a level per GOP)
        self.sequence = {}          # fields of sequence_header, sequence_extension and sequence_display_extension
        self.repeated_headers = 0   # sequence headers met again in front of a GOP header (each equal to the first)


def _sequence_headers(br):
    """sequence_header + sequence_extension + sequence_display_extension at the reader's position -> (width, height, fields).
    bit_rate is the 30-bit value (units of 400 bit/s: 18 bits of the header, 12 of the extension), vbv the 18-bit one (units of 16384
    bits: 10 + 8)."""
    # ---- sequence_header ----
    assert br.next_start_code() == 0xB3
    br.bits(32)
    width, height = br.bits(12), br.bits(12)
    hdr = dict(aspect=br.bits(4), frame_rate_code=br.bits(4), bit_rate=br.bits(18))
    assert br.bits(1) == 1
    hdr.update(vbv=br.bits(10), constrained=br.bits(1))
    assert br.bits(1) == 0 and br.bits(1) == 0, "quantiser matrices are not loaded by this encoder"
    # ---- sequence_extension ----
    assert br.next_start_code() == 0xB5
    br.bits(32)
    assert br.bits(4) == 1
    hdr.update(profile_level=br.bits(8), progressive_sequence=br.bits(1), chroma_format=br.bits(2))
    assert br.bits(2) == 0 and br.bits(2) == 0                  # horizontal / vertical size extension
    hdr["bit_rate"] |= br.bits(12) << 18
    assert br.bits(1) == 1
    hdr["vbv"] |= br.bits(8) << 10
    hdr.update(low_delay=br.bits(1))
    br.bits(7)
    assert hdr["chroma_format"] == 1
    assert 1 <= hdr["aspect"] <= 4 and 1 <= hdr["frame_rate_code"] <= 8 and hdr["bit_rate"] != 0, "forbidden or reserved value"
    # ---- sequence_display_extension ----
    assert br.next_start_code() == 0xB5
    br.bits(32)
    assert br.bits(4) == 2
    hdr.update(video_format=br.bits(3), colour_primaries=None, transfer_characteristics=None, matrix_coefficients=None)
    if br.bits(1):
        hdr.update(colour_primaries=br.bits(8), transfer_characteristics=br.bits(8), matrix_coefficients=br.bits(8))
        assert hdr["colour_primaries"] and hdr["transfer_characteristics"] and hdr["matrix_coefficients"], "0 is forbidden"
    dw = br.bits(14)
    assert br.bits(1) == 1
    hdr["display_size"] = (dw, br.bits(14))
    return width, height, hdr


def sequence_headers(data):
    """(width, height, fields) of the sequence headers at the start of a stream, without decoding a picture"""
    return _sequence_headers(BitReader(data))


def decode(data, quirks=True, syntax="module", b_pictures=False, interlaced=False, extended=False, mb_tools=False, field_pictures=False, join=0, conceal=False):
    """syntax="module" (the default): the subset this encoder emits, as the head of this file says.  syntax="main": Main-Profile
    streams of progressive frame pictures, I and P, 4:2:0, from any encoder (decode_main below); it needs quirks=False, and a
    refusal is a Refused exception that names the unit.  b_pictures=True (syntax="main" only): B pictures too, and the frames in
    display order (the section "B pictures" below); with False the function is what it was for every input.  interlaced=True
    (syntax="main" only, with b_pictures either way): frame pictures with frame_pred_frame_dct 0 too (the section "Interlaced frame
    pictures" below); with False the function is what it was for every input.  extended=True (syntax="main" only, with the other two
    either way): several slices in a macroblock row, slice headers with intra_slice_flag 1, quant_matrix_extension and
    composite_display_flag 1 too (the section "Several slices a row" below); with False the function is what it was for every input.
    mb_tools=True (with extended=True only, the other two either way): Table B-15 for the intra blocks of a picture with
    intra_vlc_format 1, concealment motion vectors, and dual prime in a P picture with frame_pred_frame_dct 0 (the section "The
    macroblock tools" below); with False the function is what it was for every input.  field_pictures=True (with interlaced, extended
    and mb_tools all True, b_pictures either way): pictures with picture_structure 1 / 2 too, two of them woven into one frame (the
    section "Field pictures" below); with False the function is what it was for every input.  join=1 .. 3 (JOIN_HEAD | JOIN_TAIL, with
    the four keywords in front of it all True, b_pictures either way): a stream cut from a running broadcast (the section "Streams
    cut from a broadcast" below); with 0 the function is what it was for every input.  conceal=True (with the same four keywords all
    True, b_pictures either way, join 0 .. 3): damaged slices are dropped and their macroblock rows patched from the picture in front
    (the section "Damaged slices" below); with False the function is what it was for every input."""
    if conceal and not (syntax == "main" and interlaced and extended and mb_tools and field_pictures):
        raise ValueError("conceal goes with syntax=\"main\", interlaced=True, extended=True, mb_tools=True and field_pictures=True")
    if join not in (0, 1, 2, 3):
        raise ValueError("join is 0 or a mask of JOIN_HEAD (1) and JOIN_TAIL (2)")
    if join and not (syntax == "main" and interlaced and extended and mb_tools and field_pictures):
        raise ValueError("join goes with syntax=\"main\", interlaced=True, extended=True, mb_tools=True and field_pictures=True")
    if field_pictures and not (syntax == "main" and interlaced and extended and mb_tools):
        raise ValueError("field_pictures goes with syntax=\"main\", interlaced=True, extended=True and mb_tools=True")
    if mb_tools and not extended:
        raise ValueError("mb_tools goes with extended=True")
    if extended and syntax != "main":
        raise ValueError("extended goes with syntax=\"main\"")
    if b_pictures and syntax != "main":
        raise ValueError("b_pictures goes with syntax=\"main\"")
    if interlaced and syntax != "main":
        raise ValueError("interlaced goes with syntax=\"main\"")
    if syntax == "main":
        assert not quirks, "the module's quirks have no meaning outside its own syntax"
        if join:
            return decode_join(data, b_pictures, join, bool(conceal))
        return decode_main(data, b_pictures, interlaced, extended, mb_tools, field_pictures, conceal=bool(conceal))
    assert syntax == "module", syntax
    T = tables()
    br = BitReader(data)
    out = Decoded()
    out.width, out.height, hdr = _sequence_headers(br)
    out.sequence = hdr
    # the header sizes are the displayable ones (6.3.3): the macroblock count rounds them up, the pictures are coded at whole
    # macroblocks and handed out cropped to width x height (chroma to the halves, rounded up)
    mbw, mbh = (out.width + 15) // 16, (out.height + 15) // 16
    W, H = 16 * mbw, 16 * mbh
    cw, ch = (out.width + 1) // 2, (out.height + 1) // 2
    ref = None
    ended = False
    while True:
        code = br.next_start_code()
        if code == 0xB7:
            br.bits(32)
            ended = True
            break
        if code == 0xB3:
            # a repeated sequence header (6.1.1.6): only in front of a GOP, and it says what the first one said
            again = _sequence_headers(br)
            assert again == (out.width, out.height, out.sequence), "a repeated sequence header differs from the first"
            out.repeated_headers += 1
            code = br.next_start_code()
            assert code == 0xB8, "a repeated sequence header must be followed by a GOP header"
        if code == 0xB8:                                        # group_of_pictures_header
            br.bits(32)
            tc = dict(drop=br.bits(1), hours=br.bits(5), minutes=br.bits(6))
            assert br.bits(1) == 1
            tc.update(seconds=br.bits(6), pictures=br.bits(6), closed_gop=br.bits(1), broken_link=br.bits(1))
            out.gops.append(tc)
            code = br.next_start_code()
        assert code == 0x00, hex(code)
        # ---- picture_header ----
        br.bits(32)
        pic = dict(temporal_reference=br.bits(10), type=br.bits(3), vbv_delay=br.bits(16))
        assert pic["type"] in (1, 2)
        if pic["type"] == 2:
            assert br.bits(1) == 0
            pic["forward_f_code"] = br.bits(3)
        assert br.bits(1) == 0                                  # extra_bit_picture
        # ---- picture_coding_extension ----
        assert br.next_start_code() == 0xB5
        br.bits(32)
        assert br.bits(4) == 8
        pic["f_code"] = [br.bits(4) for _ in range(4)]
        pic.update(intra_dc_precision=br.bits(2), picture_structure=br.bits(2), top_field_first=br.bits(1),
                   frame_pred_frame_dct=br.bits(1), concealment_motion_vectors=br.bits(1), q_scale_type=br.bits(1),
                   intra_vlc_format=br.bits(1), alternate_scan=br.bits(1), repeat_first_field=br.bits(1),
                   chroma_420_type=br.bits(1), progressive_frame=br.bits(1), composite_display_flag=br.bits(1))
        assert pic["picture_structure"] == 3 and pic["frame_pred_frame_dct"] == 1
        assert pic["q_scale_type"] == 0 and pic["intra_vlc_format"] == 0 and pic["alternate_scan"] == 0
        assert pic["concealment_motion_vectors"] == 0 and pic["intra_dc_precision"] == 2
        assert pic["f_code"][0] == 1 and pic["f_code"][1] == 1
        out.pictures.append(pic)
        if pic["type"] == 2:
            assert ref is not None, "P picture without a reference"
        Y = np.zeros((H, W), np.int64)
        U = np.zeros((H // 2, W // 2), np.int64)
        V = np.zeros((H // 2, W // 2), np.int64)
        mbs = []
        qcodes = []
        for row in range(mbh):
            assert br.next_start_code() == row + 1, "slices must come one per macroblock row, in order"
            br.bits(32)
            qcodes.append(br.bits(5))
            qscale = 2 * qcodes[-1]                             # q_scale_type 0
            assert br.bits(1) == 0                              # extra_bit_slice
            dc_pred = [0, 0, 0]                                 # relative to the reset value 1 << (7 + precision)
            pmv = [0, 0]
            for col in range(mbw):
                assert br.bits(1) == 1, "macroblock_address_increment must be 1 (no skipped macroblocks)"
                # macroblock_type, tables B-2 / B-3 (without the quant variants, which this encoder never emits)
                if pic["type"] == 1:
                    assert br.bits(1) == 1
                    intra, mc, pattern = True, False, False
                else:
                    if br.bits(1):
                        intra, mc, pattern = False, True, True          # '1'   MC, coded
                    elif br.bits(1):
                        raise AssertionError("'01' No-MC coded is never emitted by this encoder")
                    elif br.bits(1):
                        intra, mc, pattern = False, True, False         # '001' MC, not coded
                    else:
                        assert br.bits(2) == 0b11                       # '00011' intra
                        intra, mc, pattern = True, False, False
                mv = [0, 0]
                if mc:
                    for t in range(2):                          # motion_code, no residual for f_code 1 (7.6.3.1)
                        m = T["motion"](br)
                        if m and br.bits(1):
                            m = -m
                        v = pmv[t] + m
                        if v < -16:
                            v += 32
                        elif v > 15:
                            v -= 32
                        pmv[t] = mv[t] = v
                else:
                    pmv = [0, 0]                                # 7.6.3.4: reset by an intra macroblock
                cbp = 63 if intra else (T["cbp"](br) if pattern else 0)
                # prediction
                if intra:
                    py = np.full((16, 16), 128, np.int64)
                    pu = np.full((8, 8), 128, np.int64)
                    pv = np.full((8, 8), 128, np.int64)
                else:
                    dc_pred = [0, 0, 0]                         # 7.2.1: reset by a non-intra macroblock
                    py = _predict(ref[0], 16 * col, 16 * row, mv[0], mv[1], 16, quirks)
                    if quirks:
                        cmv = [mv[0] >> 1, mv[1] >> 1]          # floor
                    else:
                        cmv = [int(mv[0] / 2), int(mv[1] / 2)]  # toward zero (7.6.3.7)
                    pu = _predict(ref[1], 8 * col, 8 * row, cmv[0], cmv[1], 8, quirks)
                    pv = _predict(ref[2], 8 * col, 8 * row, cmv[0], cmv[1], 8, quirks)
                for b in range(6):
                    res = np.zeros(64, np.int64)
                    if (cbp >> (5 - b)) & 1:
                        QF = np.zeros(64, np.int64)
                        k = 0
                        comp = 0 if b < 4 else b - 3
                        if intra:
                            size = (T["dcy"] if b < 4 else T["dcc"])(br)
                            diff = 0
                            if size:
                                d = br.bits(size)
                                diff = d if d >> (size - 1) else d - (1 << size) + 1
                            dc_pred[comp] += diff
                            QF[0] = dc_pred[comp]
                            k = 1
                        first = not intra
                        while True:
                            if first and br.peek(1) == 1:       # '1s': run 0 level +-1 as first coefficient
                                br.bits(1)
                                run, lvl = 0, 1
                                lvl = -lvl if br.bits(1) else lvl
                            else:
                                sym = T["ac"](br) if not (br.peek(2) == 0b11) else (br.bits(2), (0, 1))[1]
                                if sym == "EOB":
                                    assert not first, "a coded non-intra block cannot start with EOB"
                                    break
                                if sym == "ESC":
                                    run = br.bits(6)
                                    lvl = br.bits(12)
                                    lvl = lvl - 4096 if lvl & 0x800 else lvl
                                    assert lvl not in (0, -2048)
                                else:
                                    run, lvl = sym
                                    lvl = -lvl if br.bits(1) else lvl
                            first = False
                            k += run
                            assert k < 64, "coefficient index beyond 63"
                            QF[T["zz"][k]] = lvl
                            k += 1
                        F = _dequant(QF, intra, qscale, T["W"], quirks)
                        res = idct(F, quirks)
                    res = res.reshape(8, 8)
                    if b < 4:
                        oy, ox = 8 * (b >> 1), 8 * (b & 1)
                        Y[16 * row + oy:16 * row + oy + 8, 16 * col + ox:16 * col + ox + 8] = np.clip(
                            py[oy:oy + 8, ox:ox + 8] + res, 0, 255)
                    elif b == 4:
                        U[8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pu + res, 0, 255)
                    else:
                        V[8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pv + res, 0, 255)
                mbs.append(dict(intra=intra, mv=tuple(mv), cbp=cbp))
            # the slice must end here: only zero stuffing up to the next start code
            pad = (-br.pos) & 7
            assert br.peek(pad) == 0 if pad else True
        ref = (Y, U, V)
        out.frames.append(tuple(np.ascontiguousarray(p[:r, :c]).astype(np.uint8)
                                for p, r, c in zip(ref, (out.height, ch, ch), (out.width, cw, cw))))
        out.mbs.append(mbs)
        out.slice_qcodes.append(qcodes)
    assert ended
    rest = data[(br.pos + 7) >> 3:]
    assert not any(rest) and len(data) % 32 == 0, "only zero padding may follow sequence_end_code"
    return out


def _dequant(QF, intra, qscale, W, quirks):
    F = np.zeros(64, np.int64)
    if intra:
        F[0] = 2 * QF[0]                                        # intra_dc_mult for 10-bit precision, minus the 1024 offset
        for i in range(1, 64):
            v = 2 * int(QF[i]) * int(W[i]) * qscale
            F[i] = (v >> 5) if quirks else int(v / 32)          # RTL floors (>>>), ISO truncates toward zero
    else:
        for i in range(64):
            q = int(QF[i])
            v = (2 * q + (1 if q > 0 else -1 if q < 0 else 0)) * 16 * qscale
            F[i] = int(v / 32)
    if quirks:
        F = np.clip(F, -2047, 2047)
        F[0] = 2 * QF[0] if intra else F[0]
    else:
        F = np.clip(F, -2048, 2047)
        if (int(F.sum()) & 1) == 0:                             # mismatch control (7.4.4)
            F[63] += -1 if F[63] & 1 else 1
    return F


def _predict(plane, x0, y0, mvx, mvy, n, quirks):
    """half-pel prediction of an n x n block (7.6.4); mv in half-sample units of this plane"""
    ix, iy, hx, hy = mvx >> 1, mvy >> 1, mvx & 1, mvy & 1
    H, W = plane.shape
    ys = np.arange(y0 + iy, y0 + iy + n + 1)
    xs = np.arange(x0 + ix, x0 + ix + n + 1)
    assert ys[0] >= 0 and xs[0] >= 0 and ys[n - 1 + hy] < H and xs[n - 1 + hx] < W, "vector points outside the picture"
    ys, xs = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    p = plane[np.ix_(ys, xs)].astype(np.int64)
    a, b, c, d = p[:n, :n], p[:n, 1:n + 1], p[1:n + 1, :n], p[1:n + 1, 1:n + 1]
    if hx and hy:
        return (a + b + c + d + (1 if quirks else 2)) >> 2
    if hx:
        return (a + b + 1) >> 1
    if hy:
        return (a + c + 1) >> 1
    return a


def _predict_rect(plane, x0, y0, mvx, mvy, w, h):
    """_predict(quirks=False) for a w x h block: a field prediction's 16 x 8 or 8 x 4 in one field of the reference"""
    ix, iy, hx, hy = mvx >> 1, mvy >> 1, mvx & 1, mvy & 1
    H, W = plane.shape
    ys = np.arange(y0 + iy, y0 + iy + h + 1)
    xs = np.arange(x0 + ix, x0 + ix + w + 1)
    assert ys[0] >= 0 and xs[0] >= 0 and ys[h - 1 + hy] < H and xs[w - 1 + hx] < W, "vector points outside the field"
    ys, xs = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
    p = plane[np.ix_(ys, xs)].astype(np.int64)
    a, b, c, d = p[:h, :w], p[:h, 1:w + 1], p[1:h + 1, :w], p[1:h + 1, 1:w + 1]
    if hx and hy:
        return (a + b + c + d + 2) >> 2
    if hx:
        return (a + b + 1) >> 1
    if hy:
        return (a + c + 1) >> 1
    return a


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


# ---------------------------------------------------------------------------------------------------------------
# syntax="main": ordinary Main-Profile streams of progressive frame pictures, I and P, 4:2:0 - what another encoder writes.
# Beyond the module's syntax: f_code 1 .. 9, intra_dc_precision 0 .. 3, both quantiser scale tables, both scans, matrices loaded in the
# sequence header, every macroblock type of tables B-2 / B-3, macroblock quantisers, address increments with skipped macroblocks;
# optional sequence_display_extension, GOP header and sequence_end_code; user_data, copyright_extension and
# picture_display_extension skipped where 6.2.2.2 allows them; trailing zero bytes.  Still refused: leading B and D pictures, field
# pictures, dual prime, concealment vectors, intra_vlc_format 1, scalable and size extensions, sizes over 2048, other chroma formats,
# skipped macroblocks in an I picture, an increment past the row's end, vectors that read outside the picture.  Refused unless their
# keyword is on (the sections below): B pictures (b_pictures); frame_pred_frame_dct 0 (interlaced); several slices in a row, a first
# increment other than 1, a row that ends short, a slice with intra_slice_flag 1 (the bit behind quantiser_scale_code),
# quant_matrix_extension, composite_display_flag 1 - without the keyword its 20 bits are not read and fail the zero-stuffing check
# (extended).
#
# The stream is cut at its start codes first (a start code prefix is unique in a stream: 6.2.1), the units are judged by the grammar
# of 6.2.2 - each by what it is and by the unit in front of it that is not skipped -, and then the pictures are decoded.  A refusal
# names the unit: Refused.offset is the earliest unit the grammar refuses, or else the earliest slice that cannot be read.  The
# arithmetic is the quirks=False one above - the intra DC relative to its reset value with a prediction of 128 (intra_dc_mult times
# the reset value is 1024 at every precision), Chen-Wang, saturation, mismatch control - so every stream decode(quirks=False) accepts
# decodes to the same frames here.
# ---------------------------------------------------------------------------------------------------------------
#
# B pictures (b_pictures=True; option "decode_b_pictures" of the device decoder).  Everything above stays; added:
#   headers     picture_coding_type 3, whose picture header carries full_pel_backward_vector (must be 0, as the forward one) and
#               backward_f_code (read, not judged) behind the forward pair; D pictures stay refused.  In the picture_coding_extension
#               of a B picture all four f_codes are 1 .. 9 (f_code[1][*] of an I or P picture is not judged).
#   references  an anchor is an I or P picture.  A P picture predicts from the last anchor in front of it in coded order, a B picture
#               forward from the anchor before the last one and backward from the last one, whatever GOP headers lie between.  A B
#               picture with fewer than two anchors in front of it is refused at its picture header (the leading B pictures of an
#               open GOP at the stream's start).
#   macroblocks Table B-4; PMV[0][0] (forward) and PMV[0][1] (backward), both zero at the start of a slice and behind an intra
#               macroblock, a direction the macroblock does not use keeps its predictor; forward vectors with f_code[0][t], backward
#               with f_code[1][t]; chroma vectors halved toward zero per direction.  One direction: _predict from that anchor; both:
#               each prediction formed and rounded on its own, then (a + b + 1) >> 1 per sample (7.6.7.1).  A skipped macroblock
#               (7.6.6) takes the directions of the macroblock in front of it and the predictors as its vectors, has no residual and
#               leaves the predictors alone; it is refused behind an intra macroblock.  A vector of either direction that reads
#               outside the picture refuses the slice, a skipped macroblock's too (it carries the vector to another column).
#   order       Decoded.frames is in display order, from coded order and types alone (temporal_reference is not consulted): a B
#               picture is put out when decoded, an anchor when the next anchor arrives or at the end.  Decoded.display[p] is the
#               display index of coded picture p: p - 1 for a B picture, (coded index of the next anchor) - 1 for an anchor, N - 1 for
#               the last.  Decoded.pictures, .mbs and .slice_qcodes stay in coded order.
# Every stream accepted with b_pictures=False decodes to the same frames and fields with True.
# ---------------------------------------------------------------------------------------------------------------
#
# Interlaced frame pictures (interlaced=True; option "decode_interlaced" of the device decoder; b_pictures either way).  Added:
#   sequence    with progressive_sequence 0 a picture has 2 * ((height + 31) // 32) macroblock rows (6.3.3), the slice codes run to
#               that, and the coded picture is cropped to the header's size as always (_main_mbh).  A progressive_sequence 0 stream
#               with an odd (height + 15) // 16 is therefore another stream with the option than without.
#   extension   frame_pred_frame_dct 0 where progressive_sequence and progressive_frame are both 0 (6.3.10); top_field_first,
#               repeat_first_field and chroma_420_type are read and not acted on: one coded picture is one frame, both fields woven.
#               A picture with frame_pred_frame_dct 1 decodes as before.
#   modes       in a picture with frame_pred_frame_dct 0, behind macroblock_type: frame_motion_type (2 bits) if the macroblock has a
#               forward or a backward vector - 2 frame-based, 1 field-based, 0 (reserved) and 3 (dual prime) refuse the slice -, then
#               dct_type (1 bit) if it is intra or has a pattern; then quantiser_scale_code and the rest.
#   vectors     PMV[r][s], r = 0 / 1, s = forward / backward.  A frame vector is predicted from PMV[0][s] and sets PMV[1][s] to it
#               (7.6.3.3).  A field-based macroblock carries, per direction, field_select and vector for r = 0, then for r = 1; vector r
#               from PMV[r][s], the vertical component from PMV[r][s][1] >> 1, and PMV[r][s][1] = 2 * vector afterwards.  All of them
#               are zero at a slice's start, behind an intra macroblock, behind a P picture's macroblock without a vector and behind a
#               P picture's skipped macroblock.
#   prediction  field-based (7.6.4): vector 0 forms the macroblock's top-field lines, vector 1 its bottom-field lines, each from the
#               field of the anchor its select names (0: the even rows), the vector in half samples of that field: 16 x 8 at (16 col,
#               8 row) of a 16 mbw x 8 mbh field, chroma 8 x 4 at (8 col, 4 row) with both components / 2 toward zero.  A vector that
#               reads outside its field refuses the slice.  Both directions: each formed in full, then (a + b + 1) >> 1.
#   dct_type 1  luma blocks 0 / 1 are the macroblock's top-field lines (row k of the block is row 2k), blocks 2 / 3 its bottom-field
#               lines (row 2k + 1); chroma blocks are frame blocks.
#   skipped     frame prediction: a P picture's with the zero vector; a B picture's in the directions of the macroblock in front with
#               PMV[0][s] as frame vectors - behind a field-based macroblock twice its first field vector's vertical component.
# Decoded.mbs of such a picture carry motion_type, dct_type, selects[s][r] and vectors[s][r] besides the fields above.  Still
# refused: field pictures (without field_pictures, below), dual prime, concealment vectors.  Every stream accepted with interlaced=False decodes to the same frames
# and fields with True, but for the macroblock-row exception above.
# ---------------------------------------------------------------------------------------------------------------
#
# Several slices a row (extended=True; option "decode_extended" of the device decoder; b_pictures and interlaced either way).  Added
# (6.2.4, 6.3.16: the restricted slice structure Main Profile requires; 6.2.3.2, 6.3.11):
#   slices      a picture is any number of slices, 1 <= slice code <= mbh (mbh as the other options define it).  The grammar stays
#               local: the first slice behind a picture's extensions has code 1, every further one its predecessor's code or that code
#               + 1, and a picture may end only behind a slice with code mbh.  A slice's first macroblock_address_increment, escapes
#               included, gives its first column as increment - 1; nothing is skipped in front of it.  The macroblock loop runs until
#               nothing but zero bits is left in the unit (the standard's test of 23 zero bits gives the same verdict: 23 zero bits
#               begin no macroblock).  A slice without a macroblock is refused, and one whose column passes mbw - 1.  DC predictors and
#               all vector predictors reset at every slice start; skipped macroblocks inside a slice are what each picture type defines
#   continuity  judged behind the walk: the first slice of a row starts at column 0 and the row in front of it is full; a slice with its
#               predecessor's code starts at the predecessor's last column + 1; the picture's last slice ends at column mbw - 1.  A slice
#               that breaks one of these is refused at its own start code.  Refused.offset stays the earliest unit the grammar refuses,
#               else the earliest slice in error - one that cannot be read or one that breaks continuity (a slice behind an unreadable one
#               is not judged: the unreadable one is earlier)
#   header      behind quantiser_scale_code a bit 1 is intra_slice_flag: intra_slice (1 bit) and reserved_bits (7 bits) follow, read and
#               not judged; then, while the next bit is 1, extra_bit_slice and extra_information_slice (8 bits, skipped); then the
#               closing 0.  With intra_slice_flag 0 the header is as it was
#   matrices    quant_matrix_extension (identifier 3) among the units that may follow a picture_coding_extension, in any order with
#               user_data, copyright_extension and picture_display_extension; one a picture at most (a second is refused at the second),
#               anywhere else refused at its start code.  load_intra_quantiser_matrix and load_non_intra_quantiser_matrix with 64 bytes
#               each in zig-zag order (a weight of 0 refuses the unit), the two chroma load flags 0 (4:2:0 only), zero stuffing.  A
#               loaded matrix is in force from that picture on in coded order, each matrix on its own; any sequence header, repeated
#               ones included, puts both back to the sequence's
#   composite   composite_display_flag 1: the 20 bits behind it are read and not acted on
# Still refused: leading B pictures, D pictures - field pictures too without field_pictures, dual prime, concealment vectors and Table B-15 too without mb_tools,
# below -, and everything else the main syntax refuses, where it is refused.  Every stream accepted with extended=False, under any setting of the other two, decodes to
# the same frames and fields with True.
#
# The macroblock tools (decode(..., syntax="main", extended=True, mb_tools=True), b_pictures and interlaced either way): what is left of
# the macroblock layer of frame pictures.
#   Table B-15  with the picture's intra_vlc_format 1 the AC coefficients of INTRA blocks are read with Table B-15 (end of block
#               '0110'); non-intra blocks keep B-14 with its '1s' form; DC sizes, the escape body and the scans do not change
#   concealment with concealment_motion_vectors 1 an intra macroblock carries one forward frame vector (f_code[0][*], no motion type,
#               no select) and a marker bit 1, behind the quantiser and in front of the blocks.  The vector sets PMV[0][0] and
#               PMV[1][0]; it is not used and not judged against the picture's edges; such a macroblock does not reset the predictors.
#               An I picture with the flag carries f_code[0][*] 1 .. 9
#   dual prime  frame_motion_type 3 in a P picture with frame_pred_frame_dct 0: motion_code[0][0][0], dmvector[0], motion_code[0][0][1],
#               dmvector[1] ('0' 0, '10' +1, '11' -1); the vertical component is a field vector (predicted from PMV[0][0][1] >> 1, the
#               predictor twice the vector afterwards), PMV[1][0] = PMV[0][0].  With h(a) = (a + (a > 0)) >> 1 and top_field_first 1 the
#               derived vectors are T = (h(vx) + d0, h(vy) + d1 - 1) and B = (h(3 vx) + d0, h(3 vy) + d1 + 1); with top_field_first 0
#               the factors 1 and 3 change places.  Top-field lines: the mean of the top field by (vx, vy) and the bottom field by T;
#               bottom-field lines: the mean of the bottom field by (vx, vy) and the top field by B; every read inside its field
# Still refused: leading B pictures, D pictures, dual prime in a B picture - field pictures too without field_pictures, below.  Every stream accepted with mb_tools=False
# and extended=True decodes to the same frames with True.
#
# Field pictures (decode(..., syntax="main", interlaced=True, extended=True, mb_tools=True, field_pictures=True), b_pictures either way;
# option "decode_field_pictures" of the device decoder; 6.1.1.4, 6.3.10, 6.3.17, 7.6.2 - 7.6.3.6, 7.6.6, 7.6.7).  Added:
#   extension   picture_structure 1 (top field) and 2 (bottom field) where progressive_sequence, progressive_frame, frame_pred_frame_dct,
#               top_field_first and repeat_first_field are all 0; 0 (reserved) stays refused, all at the coding extension
#   pairs       a coded frame is one frame picture or two field pictures that follow each other in coded order.  A picture is a unit
#               whose picture header reads; its structure is that of the coding extension right behind it (3 where there is none).  A
#               field picture that no first field waits for is a first field; the next picture is its partner, whatever it is, and is
#               refused at its picture header unless it is a field of the other parity with the same temporal_reference and the same
#               picture_coding_type (or a P field behind an I field).  While a first field waits, a sequence header, a GOP header or a
#               sequence_end_code is refused at its start code; a first field no picture follows is refused at its own picture header
#   geometry    a field has mbh / 2 macroblock rows (mbh = 2 * ((height + 31) // 32)): the slice codes run to that, a field ends only
#               behind that code, continuity is judged per field.  Row r, line k of the field of parity p is frame line 32 r + 2 k + p
#   modes       field_motion_type (2 bits) where the macroblock has a vector: 1 field-based (one vector a direction), 2 16 x 8 (two), 3
#               dual prime (a P field only), 0 refused; no dct_type.  motion_vertical_field_select in front of every vector of the first
#               two kinds.  No component is halved or doubled.  Field-based: from PMV[0][s], PMV[1][s] = PMV[0][s] afterwards; 16 x 8:
#               vector r from and into PMV[r][s]; dual prime: no select, a dmvector behind each component, PMV[1][0] = PMV[0][0].  A
#               concealment vector carries a select (read, not used), sets PMV[0][0] and PMV[1][0], and its marker bit follows
#   prediction  the field a select names is the most recently decoded anchor field of that parity: the fields of the anchor frame(s)
#               - but for the second field of an anchor frame the field of the other parity is the first field of its own frame, and
#               that of its own parity belongs to the anchor frame in front (none in the stream's first frame: such a select refuses
#               the slice).  Field-based 16 x 16 (chroma 8 x 8, both components / 2 toward zero); 16 x 8: the upper half by vector 0, the
#               lower by vector 1 (chroma 8 x 4 each); dual prime: (a + b + 1) >> 1 of the field of the same parity by (vx, vy) and the
#               other one by (h(vx) + d0, h(vy) + d1 + e), h(a) = (a + (a > 0)) >> 1, e = -1 in a top field, +1 in a bottom field.  Every
#               read inside its field.  A P field's macroblock without a vector and its skipped macroblock: the zero vector from the
#               field of the same parity, the predictors reset; a B field's skipped macroblock: the directions in front, PMV[0][s],
#               field-based from the same parity
#   output      one frame a coded frame, both fields woven; a frame's type is its first field's (I + P is an I frame); display order,
#               Decoded.pictures (the frame picture's or the first field's fields), gops and repeated_headers count frames;
#               Decoded.fields, .mbs and .slice_qcodes are per coded picture.  A B frame needs two anchor frames in front of it
# Still refused: leading B pictures (without join, below), D pictures, dual prime in a B picture.  Every stream accepted with
# field_pictures=False and the other three on decodes to the same frames with True.
#
# Streams cut from a broadcast (decode(..., syntax="main", interlaced=True, extended=True, mb_tools=True, field_pictures=True,
# join=JOIN_HEAD | JOIN_TAIL), b_pictures either way; option "decode_join" of the device decoder).  Such a stream begins wherever the
# recording began, its GOPs are open, and it breaks off inside a picture.  Nothing above changes; decode_join reads the bytes [J, T) of
# the stream exactly as a stream of their own, and every offset it reports counts from the first byte of the input:
#   head (1)    J is the offset of the first sequence_header_code (00 00 01 B3) among the start codes; what lies in front of it is
#               not read any further and not judged.  Without one: Refused(0).  The header group at J is "the first sequence header"
#               of every rule above, and a wrong one is refused at its own unit - no later one is looked for.
#               Leading B pictures (b_pictures only): a B picture that begins a frame while fewer than two anchor frames have begun
#               since J is dropped where it was refused, a B field pair as a pair (the picture behind a first field is its partner).
#               A dropped picture's units are judged by the grammar as a kept picture's are - header, coding extension, the rules of a
#               pair, slice codes, one quant_matrix_extension at most - and a matrix it loads holds from that picture on; its slices
#               are not walked.  It is in no list of the result and has no frame, no display index: those are the kept frames' alone.
#               A P picture with no I frame in front of it since J stays refused
#   tail (2)    where the last unit that is not skipped is sequence_end_code nothing is dropped.  Otherwise F is the last picture start
#               code that begins a frame - paired as the plan pairs: the picture behind a waiting first field is its partner, whatever
#               it is; a picture start code whose header does not read begins a frame unless a first field waits, and leaves the pairing alone - and T the offset
#               of the first group_start_code or picture_start_code behind the last slice in front of F (behind the unit at J where
#               there is no such slice).  The units from T on are not judged; one frame counts as dropped.  A frame is known by its picture
#               start code alone: while the bytes behind the last whole frame hold none yet (a GOP header alone), that frame goes.  The rule is blunt: a
#               complete stream without sequence_end_code loses its last frame, which is why the tail is a bit of its own
# Decoded.join_offset = J (0 without bit 1), .tail_offset = T (len(data) where nothing was dropped behind), .dropped_leading and
# .dropped_trailing count frames.  A stream in which no frame is left is a stream without pictures.  Every stream accepted with join=0
# decodes to the same frames with join=1, and with join=2 or 3 where it ends with sequence_end_code.
#
# Damaged slices (decode(..., syntax="main", interlaced=True, extended=True, mb_tools=True, field_pictures=True, conceal=True), b_pictures
# either way, join 0 .. 3; option "decode_conceal" of the device decoder).  A slice that cannot be read no longer refuses the stream: it
# is dropped, the hole is patched from the frame in front, and the record is that of the undamaged stream.  These rules replace the ones
# above; they stay local - a unit and the unit in front of it that is not skipped:
#   grammar     a slice is legal behind a picture_coding_extension or behind a slice, whatever the two codes are.  A slice whose code is
#               above the picture's rows (a field's rows for a field) is a bad slice: counted, not walked, not refused.  A sequence
#               header, GOP header, picture header or sequence_end_code, and the end of the stream, are legal behind a slice of any code
#               or behind a picture_coding_extension (a picture with no slice left).  Everything else is judged as with conceal=False -
#               headers, extensions, the pairs, "P without an I frame", "B without two anchor frames", a second
#               quant_matrix_extension, the join window - and refused at the same unit: damage to a header stays a refusal
#   rows        the unit of concealment is the macroblock row of a coded picture (a field's row for a field).  A row is kept if and only
#               if the slices of the picture that carry its code, in stream order, all read, the first starts at column 0, each further
#               one starts one column behind the last column of the one in front, and the last ends at column mbw - 1.  Any other row is
#               concealed whole: no slice, a slice that does not read (a bad slice too), a gap, an overlap, a duplicate.  The rule is
#               blunt on purpose: where inside a slice an error is noticed is not pinned, only the verdict per slice is; and whatever a
#               damaged slice wrote lies in its own row, which is overwritten
#   patch       every macroblock of a concealed row of a frame picture is a P picture's skipped macroblock - forward, frame-based, the
#               zero vector, no residual -, of a field picture forward, field-based from the field of its own parity, the zero vector.
#               The reference is the frame the picture's forward reference names: for P the anchor frame in front, for B the earlier
#               of its two, for I the anchor frame in front as if it were P; a second field takes its own parity from that frame too,
#               never from its own.  No such frame (the first anchor frame of the stream or of the join window, both of its fields):
#               Y = U = V = 128, a grey row.  A concealed picture is a reference like any other
# Decoded.concealed lists (coded picture, row) of every concealed row (coded pictures as Decoded.fields counts them); Decoded.conceal is the
# report: first_offset - the offset, from the first byte of the input, of the picture start code of the first coded picture with a
# concealed row, len(data) where there is none -, bad_slices, concealed_rows, grey_rows, damaged_pictures (coded pictures).  Decoded.mbs
# and .slice_qcodes hold what the walks left and say nothing of a concealed row.  Every stream accepted with conceal=False decodes to the
# same frames with True, and a report of zeros.
# ---------------------------------------------------------------------------------------------------------------
JOIN_HEAD, JOIN_TAIL = 1, 2


class Refused(Exception):
    def __init__(self, offset, why=""):
        Exception.__init__(self, "unit at byte %d: %s" % (offset, why))
        self.offset = offset


_B1_INCREMENT = """1:1 2:011 3:010 4:0011 5:0010 6:00011 7:00010 8:0000111 9:0000110 10:00001011 11:00001010 12:00001001 13:00001000
14:00000111 15:00000110 16:0000010111 17:0000010110 18:0000010101 19:0000010100 20:0000010011 21:0000010010 22:00000100011
23:00000100010 24:00000100001 25:00000100000 26:00000011111 27:00000011110 28:00000011101 29:00000011100 30:00000011011
31:00000011010 32:00000011001 33:00000011000"""
_B1_ESCAPE = "00000001000"
# tables B-2 (I pictures) and B-3 (P pictures): code -> (macroblock_quant, macroblock_motion_forward, macroblock_pattern, macroblock_intra)
_B2_TYPE_I = {"1": (0, 0, 0, 1), "01": (1, 0, 0, 1)}
_B3_TYPE_P = {"1": (0, 1, 1, 0), "01": (0, 0, 1, 0), "001": (0, 1, 0, 0), "00011": (0, 0, 0, 1), "00010": (1, 1, 1, 0), "00001": (1, 0, 1, 0),
              "000001": (1, 0, 0, 1)}
# table B-4 (B pictures): code -> (macroblock_quant, macroblock_motion_forward, macroblock_motion_backward, macroblock_pattern, macroblock_intra)
_B4_TYPE_B = {"10": (0, 1, 1, 0, 0), "11": (0, 1, 1, 1, 0), "010": (0, 0, 1, 0, 0), "011": (0, 0, 1, 1, 0), "0010": (0, 1, 0, 0, 0), "0011": (0, 1, 0, 1, 0),
              "00011": (0, 0, 0, 0, 1), "00010": (1, 1, 1, 1, 0), "000011": (1, 1, 0, 1, 0), "000010": (1, 0, 1, 1, 0), "000001": (1, 0, 0, 0, 1)}
# table 7-6, q_scale_type 1: quantiser_scale of quantiser_scale_code 1 .. 31 (code 0 is forbidden; a slice that carries it gets 0, as
# with q_scale_type 0)
_NONLINEAR_SCALE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112]
# 7.3 figure 7-3: alternate scan, scan position of raster [v][u]
_ALTERNATE = [0, 4, 6, 20, 22, 36, 38, 52, 1, 5, 7, 21, 23, 37, 39, 53, 2, 8, 19, 24, 34, 40, 50, 54, 3, 9, 18, 25, 35, 41, 51, 55,
              10, 17, 26, 30, 42, 46, 56, 60, 11, 16, 27, 31, 43, 47, 57, 61, 12, 15, 28, 32, 44, 48, 58, 62, 13, 14, 29, 33, 45, 49, 59, 63]
MAIN_MAX_SIZE = 2048


def main_tables():
    """the raw tables of the main syntax, for tests: B-1 as (code, length, increment), the scale table, the alternate scan"""
    return dict(increment=_parse(_B1_INCREMENT), escape=_B1_ESCAPE, nonlinear=list(_NONLINEAR_SCALE), alternate=list(_ALTERNATE),
                type_i=dict(_B2_TYPE_I), type_p=dict(_B3_TYPE_P), type_b=dict(_B4_TYPE_B))


_TM = None


def _main_tables():
    global _TM
    if _TM is None:
        esc = (int(_B1_ESCAPE, 2), len(_B1_ESCAPE), "ESC")
        alt = np.zeros(64, np.int64)
        for raster, pos in enumerate(_ALTERNATE):
            alt[pos] = raster
        types = lambda t: _vlc_decoder([(int(bits, 2), len(bits), flags) for bits, flags in t.items()])
        _TM = dict(incr=_vlc_decoder(_parse(_B1_INCREMENT) + [esc]), type_i=types(_B2_TYPE_I), type_p=types(_B3_TYPE_P), type_b=types(_B4_TYPE_B), alt=alt)
    return _TM


class _UnitBits(BitReader):
    """the bits of one unit: from behind its start code to where the next one begins; nothing is read beyond"""
    def __init__(self, data, start, end):
        BitReader.__init__(self, data)
        self.pos, self.end = 8 * (start + 4), 8 * end

    def bits(self, n):
        if self.pos + n > self.end:
            raise ValueError("the unit ends at bit %d" % self.end)
        return BitReader.bits(self, n)

    def rest_is_zero(self):
        pad = (-self.pos) & 7
        return (self.bits(pad) == 0 if pad else True) and not any(self.d[self.pos >> 3:self.end >> 3])

    def only_zeros_left(self):
        """rest_is_zero without moving: whether nothing but zero bits is left in the unit"""
        at = self.pos
        zero = self.rest_is_zero()
        self.pos = at
        return zero


def start_codes(data):
    """[(offset, code)] of every 00 00 01 xx whose code byte lies inside the stream"""
    out, at = [], data.find(b"\x00\x00\x01")
    while at >= 0 and at + 3 < len(data):
        out.append((at, data[at + 3]))
        at = data.find(b"\x00\x00\x01", at + 3)
    return out


def _main_sequence_header(data, start, end):
    br = _UnitBits(data, start, end)
    h = dict(width=br.bits(12), height=br.bits(12), aspect=br.bits(4), frame_rate_code=br.bits(4), bit_rate=br.bits(18))
    assert br.bits(1) == 1
    h.update(vbv=br.bits(10), constrained=br.bits(1))
    zz = tables()["zz"]
    for name, default in (("intra_matrix", _INTRA_W), ("non_intra_matrix", [16] * 64)):
        w = list(default)
        if br.bits(1):                                          # load_..._quantiser_matrix: 64 bytes in zig-zag order (6.3.11)
            for k in range(64):
                w[int(zz[k])] = br.bits(8)
                assert w[int(zz[k])] != 0, "a matrix weight of 0 is forbidden"
        h[name] = w
    assert br.rest_is_zero()
    return h


def _main_sequence_extension(data, start, end, h):
    br = _UnitBits(data, start, end)
    assert br.bits(4) == 1
    h.update(profile_level=br.bits(8), progressive_sequence=br.bits(1), chroma_format=br.bits(2))
    assert br.bits(2) == 0 and br.bits(2) == 0, "size extensions"
    h["bit_rate"] |= br.bits(12) << 18
    assert br.bits(1) == 1
    h["vbv"] |= br.bits(8) << 10
    h.update(low_delay=br.bits(1))
    br.bits(7)
    assert h["chroma_format"] == 1
    assert 1 <= h["aspect"] <= 4 and 1 <= h["frame_rate_code"] <= 8 and h["bit_rate"] != 0, "forbidden or reserved value"
    assert br.rest_is_zero()


def _main_display_extension(data, start, end, h):
    br = _UnitBits(data, start, end)
    assert br.bits(4) == 2
    h.update(video_format=br.bits(3), colour_primaries=None, transfer_characteristics=None, matrix_coefficients=None)
    if br.bits(1):
        h.update(colour_primaries=br.bits(8), transfer_characteristics=br.bits(8), matrix_coefficients=br.bits(8))
        assert h["colour_primaries"] and h["transfer_characteristics"] and h["matrix_coefficients"], "0 is forbidden"
    dw = br.bits(14)
    assert br.bits(1) == 1
    h["display_size"] = (dw, br.bits(14))
    assert br.rest_is_zero()


def _main_picture_extension(data, start, end, ptype, b_pictures=False, interlaced=False, progressive_sequence=1, extended=False, mb_tools=False,
                            field_pictures=False):
    br = _UnitBits(data, start, end)
    assert br.bits(4) == 8
    pic = dict(f_code=[br.bits(4) for _ in range(4)])
    pic.update(intra_dc_precision=br.bits(2), picture_structure=br.bits(2), top_field_first=br.bits(1),
               frame_pred_frame_dct=br.bits(1), concealment_motion_vectors=br.bits(1), q_scale_type=br.bits(1),
               intra_vlc_format=br.bits(1), alternate_scan=br.bits(1), repeat_first_field=br.bits(1),
               chroma_420_type=br.bits(1), progressive_frame=br.bits(1), composite_display_flag=br.bits(1))
    if field_pictures and pic["picture_structure"] in (1, 2):   # a field picture: nothing progressive, no frame prediction, no field order
        assert not (progressive_sequence or pic["progressive_frame"] or pic["frame_pred_frame_dct"] or pic["top_field_first"] or pic["repeat_first_field"])
    else:
        assert pic["picture_structure"] == 3
    if pic["frame_pred_frame_dct"] != 1:                        # 6.3.10: 0 only where neither the sequence nor the frame is progressive
        assert interlaced and not progressive_sequence and not pic["progressive_frame"], "frame_pred_frame_dct"
    assert mb_tools or (pic["concealment_motion_vectors"] == 0 and pic["intra_vlc_format"] == 0)
    for f in pic["f_code"][:2]:                               # an I picture may carry 15, "not used" (6.3.10) - without concealment vectors
        assert 1 <= f <= 9 or (ptype == 1 and f == 15 and not pic["concealment_motion_vectors"]), "f_code"
    if b_pictures and ptype == 3:
        for f in pic["f_code"][2:]:
            assert 1 <= f <= 9, "f_code"
    if extended and pic["composite_display_flag"]:              # v_axis, field_sequence, sub_carrier, burst_amplitude, sub_carrier_phase
        br.bits(20)
    assert br.rest_is_zero()
    return pic


def _main_quant_extension(data, start, end):
    """quant_matrix_extension (6.2.3.2) -> [intra matrix or None, non-intra matrix or None], raster order"""
    br = _UnitBits(data, start, end)
    assert br.bits(4) == 3
    zz = tables()["zz"]
    out = [None, None]
    for m in range(2):
        if br.bits(1):                                          # load_..._quantiser_matrix: 64 bytes in zig-zag order
            w = [0] * 64
            for k in range(64):
                w[int(zz[k])] = br.bits(8)
                assert w[int(zz[k])] != 0, "a matrix weight of 0 is forbidden"
            out[m] = w
    assert br.bits(1) == 0 and br.bits(1) == 0, "chroma matrices belong to 4:2:2 and 4:4:4"
    assert br.rest_is_zero()
    return out


_SEQ, _SEQEXT, _DISP, _GOP, _PIC, _PICEXT, _SLICE, _END, _USER, _SKIPPED_EXT, _BAD, _QUANT = range(12)


def _main_role(data, pos, code, extended=False):
    if code == 0xB3:
        return _SEQ
    if code == 0xB8:
        return _GOP
    if code == 0xB7:
        return _END
    if code == 0x00:
        return _PIC
    if 1 <= code <= 0xAF:
        return _SLICE
    if code == 0xB2:
        return _USER
    if extended and code == 0xB5 and pos + 4 < len(data) and data[pos + 4] >> 4 == 3:
        return _QUANT                                           # quant_matrix_extension
    if code == 0xB5 and pos + 4 < len(data):                    # extension_start_code_identifier
        return {1: _SEQEXT, 2: _DISP, 8: _PICEXT, 4: _SKIPPED_EXT, 7: _SKIPPED_EXT}.get(data[pos + 4] >> 4, _BAD)
    return _BAD


def _main_mbh(hdr, interlaced=False):
    """macroblock rows of a frame picture (6.3.3): with interlaced=True a sequence that is not progressive has whole field macroblocks"""
    if interlaced and not hdr["progressive_sequence"]:
        return 2 * ((hdr["height"] + 31) // 32)
    return (hdr["height"] + 15) // 16


def _main_plan(data, b_pictures=False, interlaced=False, extended=False, mb_tools=False, field_pictures=False, dropped=None, conceal=False):
    """the grammar over the start codes -> (sequence fields, pictures, gops, repeated headers, number of start codes).  dropped (a
    list, with field_pictures): the leading B frames are dropped, not refused; their first pictures are appended to it.  conceal: the
    relaxed rules of the section "Damaged slices" - no order among the slice codes, a picture may end behind any slice or none"""
    n = len(data)
    ev = start_codes(data)
    if not ev or any(data[:ev[0][0]]):
        raise Refused(0, "no start code, or something in front of the first")
    ends = [p for p, _ in ev[1:]] + [n]
    roles = [_main_role(data, p, c, extended) for p, c in ev]
    last_nz = len(data.rstrip(b"\x00"))                         # one past the last byte that is not zero

    def group(i):
        """sequence_header at unit i, sequence_extension behind it, sequence_display_extension behind that and any user_data:
        -> the fields, or the offset of the first unit that is wrong"""
        if roles[i] != _SEQ or i + 1 >= len(ev):
            return ev[i][0]
        try:
            h = _main_sequence_header(data, ev[i][0], ends[i])
        except Exception:
            return ev[i][0]
        try:
            assert roles[i + 1] == _SEQEXT
            _main_sequence_extension(data, ev[i + 1][0], ends[i + 1], h)
        except Exception:
            return ev[i + 1][0]
        j = i + 2
        while j < len(ev) and roles[j] == _USER:
            j += 1
        h["display"] = False
        if j < len(ev) and roles[j] == _DISP:
            try:
                _main_display_extension(data, ev[j][0], ends[j], h)
            except Exception:
                return ev[j][0]
            h["display"] = True
        return h

    first = group(0)
    if not isinstance(first, dict):
        raise Refused(first, "the sequence header")
    if not (1 <= first["width"] <= MAIN_MAX_SIZE and 1 <= first["height"] <= MAIN_MAX_SIZE):
        raise Refused(ev[0][0], "the size")
    mbh = _main_mbh(first, interlaced)
    bad = []
    pictures, gops, repeats = [], [], 0
    prev = None                                                 # the unit in front that is not skipped
    have_i = False
    anchors = 0
    mats = [first["intra_matrix"], first["non_intra_matrix"]]   # the matrices in force (extended: a quant_matrix_extension replaces them)
    quant_seen = False
    rows = mbh                                                  # field_pictures: the macroblock rows of the picture whose coding extension was the last
    waiting = None                                              # field_pictures: the first field whose partner has not come
    frames, frame_i, frame_anchors = 0, False, 0                # field_pictures: the frames, whether one of them is an I frame, the anchor frames
    for i, (pos, code) in enumerate(ev):
        role, end = roles[i], ends[i]
        prole = roles[prev] if prev is not None else None
        top = prole in (_SEQEXT, _DISP) or (prole == _SLICE and ev[prev][1] == mbh)
        if field_pictures:                                      # a field ends behind the slice of its own last row
            top = prole in (_SEQEXT, _DISP) or (prole == _SLICE and ev[prev][1] == rows)
            if waiting is not None and role in (_SEQ, _GOP, _END):
                bad.append(pos)                                 # between the two fields of a frame
        if conceal:                                             # a picture ends behind a slice of any code, or with no slice left
            top = prole in (_SEQEXT, _DISP, _SLICE, _PICEXT)
        ok = True
        try:
            if role == _BAD:
                ok = False
            elif role == _SEQ:
                if i:
                    again = group(i)
                    if not isinstance(again, dict):
                        bad.append(again)
                    else:
                        ok = top and again == first             # 6.1.1.6: it says what the first one said, matrices included
                        repeats += 1
                        mats = [first["intra_matrix"], first["non_intra_matrix"]]
            elif role == _SEQEXT:
                ok = i > 0 and roles[i - 1] == _SEQ             # (read with its sequence header)
            elif role == _DISP:
                ok = prole == _SEQEXT
                _main_display_extension(data, pos, end, {})
            elif role == _USER:                                 # extension_and_user_data(0), (1), (2)
                ok = prole in (_SEQEXT, _DISP, _GOP, _PICEXT)
            elif role == _SKIPPED_EXT:                          # extension_data(2): copyright_extension, picture_display_extension
                ok = prole == _PICEXT
            elif role == _QUANT:                                # extension_data(2): at most one quant_matrix_extension a picture
                ok = prole == _PICEXT and not quant_seen
                quant_seen = True
                loaded = _main_quant_extension(data, pos, end)
                if ok and pictures:
                    mats = [loaded[m] if loaded[m] is not None else mats[m] for m in range(2)]
                    pictures[-1]["matrices"] = mats
            elif role == _GOP:
                ok = top
                br = _UnitBits(data, pos, end)
                tc = dict(drop=br.bits(1), hours=br.bits(5), minutes=br.bits(6))
                assert br.bits(1) == 1
                tc.update(seconds=br.bits(6), pictures=br.bits(6), closed_gop=br.bits(1), broken_link=br.bits(1))
                assert br.rest_is_zero()
                gops.append(tc)
            elif role == _PIC:
                ok = top or prole == _GOP
                br = _UnitBits(data, pos, end)
                pic = dict(temporal_reference=br.bits(10), type=br.bits(3), vbv_delay=br.bits(16), unit=i, slices=[])
                assert pic["type"] in ((1, 2, 3) if b_pictures else (1, 2)), "B and D pictures"
                if pic["type"] in (2, 3):
                    assert br.bits(1) == 0
                    pic["forward_f_code"] = br.bits(3)
                if pic["type"] == 3:
                    assert br.bits(1) == 0                      # full_pel_backward_vector
                    pic["backward_f_code"] = br.bits(3)
                assert br.bits(1) == 0                          # extra_bit_picture
                assert br.rest_is_zero()
                if dropped is not None and field_pictures:      # a leading B frame: its first picture, and the partner of such a one
                    pic["gone"] = waiting["gone"] if waiting is not None else pic["type"] == 3 and frame_anchors < 2
                gone = pic.get("gone", False)
                have_i = have_i or (pic["type"] == 1 and not gone)
                if not have_i and not gone:
                    bad.append(pos)                             # a P picture without a reference
                if pic["type"] == 3 and anchors < 2 and not gone:
                    bad.append(pos)                             # a B picture without two anchors in front of it
                anchors += pic["type"] != 3 and not gone
                pic["matrices"] = mats
                pictures.append(pic)
                if field_pictures:                              # the pairs; the two rules above once more, counted in frames
                    ps = data[ev[i + 1][0] + 6] & 3 if i + 1 < len(ev) and roles[i + 1] == _PICEXT and ev[i + 1][0] + 6 < n else 3
                    if waiting is not None:                     # the partner, whatever it is
                        legal = ps in (1, 2) and ps != waiting["ps"] and pic["temporal_reference"] == waiting["temporal_reference"] and \
                            (pic["type"] == waiting["type"] or (waiting["type"] == 1 and pic["type"] == 2))
                        if not legal:
                            bad.append(pos)
                        pic.update(frame=waiting["frame"], second=True)
                        waiting = None
                    else:
                        pic.update(frame=frames, second=False)
                        frames += not gone
                        frame_i = frame_i or (pic["type"] == 1 and not gone)
                        if ps in (1, 2):
                            waiting = dict(ps=ps, pos=pos, frame=pic["frame"], type=pic["type"], temporal_reference=pic["temporal_reference"], gone=gone)
                    if gone:
                        pass                                    # judged as a pair, and no more
                    elif not frame_i:
                        bad.append(pos)                         # a P picture without a reference
                    if pic["type"] == 3 and frame_anchors < 2 and not gone:
                        bad.append(pos)                         # a B picture without two anchor frames in front of it
                    frame_anchors += pic["type"] != 3 and not pic["second"] and not gone
            elif role == _PICEXT:
                ok = i > 0 and roles[i - 1] == _PIC
                ptype = (data[ev[i - 1][0] + 5] >> 3) & 7 if ok and ev[i - 1][0] + 5 < n else 0
                quant_seen = False
                if field_pictures and pos + 6 < n:              # the rows of this picture's slices, from the two bits alone
                    rows = mbh // 2 if data[pos + 6] & 3 in (1, 2) else mbh
                ext = _main_picture_extension(data, pos, end, ptype, b_pictures, interlaced, first["progressive_sequence"], extended, mb_tools, field_pictures)
                if ok and pictures and pictures[-1]["unit"] == i - 1:
                    pictures[-1].update(ext)
            elif role == _SLICE:
                ok = code <= mbh and (prole == _PICEXT if code == 1 else prole == _SLICE and ev[prev][1] == code - 1)
                if extended:                                    # the first has code 1, a further one its predecessor's code or that + 1
                    ok = code <= mbh and ((code == 1 and prole == _PICEXT) or (prole == _SLICE and ev[prev][1] in (code, code - 1)))
                if field_pictures:
                    ok = ok and code <= rows
                if conceal:                                     # behind the coding extension or a slice, whatever the two codes are
                    ok = prole in (_PICEXT, _SLICE)
                if ok and pictures:
                    pictures[-1]["slices"].append(i)
            else:                                               # sequence_end_code: the last one, only zeros behind it
                ok = top and i + 1 == len(ev) and last_nz <= pos + 4
        except Exception:
            ok = False
        if role not in (_USER, _SKIPPED_EXT, _BAD, _QUANT):
            prev = i
        if i + 1 == len(ev) and role != _END and ok:            # no sequence_end_code: the stream ends where a picture does
            prole = roles[prev] if prev is not None else None
            ok = prole in (_SEQEXT, _DISP) or (prole == _SLICE and ev[prev][1] == mbh)
            if field_pictures:
                ok = prole in (_SEQEXT, _DISP) or (prole == _SLICE and ev[prev][1] == rows)
            if conceal:
                ok = prole in (_SEQEXT, _DISP, _SLICE, _PICEXT) and role != _QUANT
        if not ok:
            bad.append(pos)
    if waiting is not None:
        bad.append(waiting["pos"])                              # a first field no picture follows
    if bad:
        raise Refused(min(bad), "the grammar of the start codes")
    if dropped is not None:
        dropped.extend(p for p in pictures if p.get("gone") and not p["second"])
        pictures = [p for p in pictures if not p.get("gone")]
    return first, pictures, gops, repeats, ev, ends


def _main_dequant(QF, intra, qscale, W, dc_mult):
    """7.4.2 with the stream's matrix, saturation (7.4.3) and mismatch control (7.4.4); an intra block's QF[0] is its DC relative to
    the reset value"""
    F = np.zeros(64, np.int64)
    for i in range(64):
        q = int(QF[i])
        if intra and i == 0:
            v = dc_mult * q
        else:
            v = 2 * q * int(W[i]) * qscale if intra else (2 * q + (1 if q > 0 else -1 if q < 0 else 0)) * int(W[i]) * qscale
            v = -((-v) // 32) if v < 0 else v // 32             # toward zero
        F[i] = v
    F = np.clip(F, -2048, 2047)
    if (int(F.sum()) & 1) == 0:
        F[63] += -1 if F[63] & 1 else 1
    return F


def display_order(types):
    """the display index of every coded picture from the picture types in coded order (3 = B): a B picture is put out when decoded,
    an anchor when the next anchor arrives, or at the end"""
    n = len(types)
    out, nxt = [0] * n, n
    for p in range(n - 1, -1, -1):
        if types[p] == 3:
            out[p] = p - 1
        else:
            out[p], nxt = nxt - 1, p
    return out


def _picture_reads(data, pos, end, b_pictures):
    """whether the picture header of the unit at pos reads, as _main_plan judges it"""
    try:
        br = _UnitBits(data, pos, end)
        br.bits(10)
        ptype = br.bits(3)
        br.bits(16)
        assert ptype in ((1, 2, 3) if b_pictures else (1, 2))
        for _ in range({1: 0, 2: 1, 3: 2}[ptype]):
            assert br.bits(1) == 0
            br.bits(3)
        assert br.bits(1) == 0
        return br.rest_is_zero()
    except Exception:
        return False


def join_window(data, join, b_pictures=False):
    """the window of a stream cut from a broadcast (the section "Streams cut from a broadcast") -> (J, T, frames dropped behind)"""
    data = bytes(data)
    n = len(data)
    ev = start_codes(data)
    j = 0                                                       # the unit at J
    if join & JOIN_HEAD:
        j = next((k for k, (_, code) in enumerate(ev) if code == 0xB3), None)
        if j is None:
            raise Refused(0, "no sequence header")
    J = ev[j][0] if join & JOIN_HEAD else 0
    if not join & JOIN_TAIL or not ev:
        return J, n, 0
    roles = [_main_role(data, p, c, True) for p, c in ev]
    ends = [p for p, _ in ev[1:]] + [n]
    significant = [k for k in range(j, len(ev)) if roles[k] not in (_USER, _SKIPPED_EXT, _BAD, _QUANT)]
    if significant and roles[significant[-1]] == _END:
        return J, n, 0
    F, waiting = None, False
    for k in range(j, len(ev)):
        if roles[k] != _PIC:
            continue
        if not _picture_reads(data, ev[k][0], ends[k], b_pictures):
            if not waiting:
                F = k                                           # it begins a frame, and leaves the pairing alone
            continue
        if waiting:
            waiting = False
            continue
        F = k
        waiting = k + 1 < len(ev) and roles[k + 1] == _PICEXT and ev[k + 1][0] + 6 < n and data[ev[k + 1][0] + 6] & 3 in (1, 2)
    if F is None:
        return J, n, 0
    s = max([k for k in range(j, F) if roles[k] == _SLICE], default=j)
    t = next((k for k in range(s + 1, F + 1) if roles[k] in (_GOP, _PIC)), F)      # (F is the unit at J itself: nothing is left, Refused(0))
    return J, ev[t][0], 1


def decode_join(data, b_pictures=False, join=JOIN_HEAD | JOIN_TAIL, conceal=False):
    """decode(..., join=): the bytes [J, T) as a stream of their own, its leading B frames dropped with JOIN_HEAD; offsets count from
    the first byte of data"""
    data = bytes(data)
    J, T, trailing = join_window(data, join, b_pictures)
    dropped = [] if join & JOIN_HEAD else None
    try:
        out = decode_main(data[J:T], b_pictures, True, True, True, True, dropped, conceal)
    except Refused as r:
        raise Refused(r.offset + J, "in the window [%d, %d): %s" % (J, T, r))
    if conceal:                                                 # offsets count from the first byte of the input
        out.conceal["first_offset"] = out.conceal["first_offset"] + J if out.concealed else len(data)
    out.join_offset, out.tail_offset, out.dropped_leading, out.dropped_trailing = J, T, len(dropped or ()), trailing
    return out


def decode_main(data, b_pictures=False, interlaced=False, extended=False, mb_tools=False, field_pictures=False, dropped=None, conceal=False):
    data = bytes(data)
    T, TM = tables(), _main_tables()
    hdr, pictures, gops, repeats, ev, ends = _main_plan(data, b_pictures, interlaced, extended, mb_tools, field_pictures, dropped, conceal)
    out = Decoded()
    if conceal:                                                 # (coded picture, row) of every concealed row; the report
        out.concealed = []
        out.conceal = dict(first_offset=len(data), bad_slices=0, concealed_rows=0, grey_rows=0, damaged_pictures=0)
    out.width, out.height, out.sequence, out.gops, out.repeated_headers, out.units = hdr["width"], hdr["height"], hdr, gops, repeats, len(ev)
    mbw, mbh = (out.width + 15) // 16, _main_mbh(hdr, interlaced)
    W, H = 16 * mbw, 16 * mbh
    cw, ch = (out.width + 1) // 2, (out.height + 1) // 2
    WI, WN = hdr["intra_matrix"], hdr["non_intra_matrix"]
    ref = None
    before = None                                               # the anchor before the last one: a B picture's forward reference
    held = None                                                 # field_pictures: the frame whose first field is decoded, and that field's type
    out.fields = []                                             # field_pictures: every coded picture (out.pictures: one a frame)
    for pic in pictures:
        out.pictures.append(pic)
        if extended:
            WI, WN = pic["matrices"]
        scan = TM["alt"] if pic["alternate_scan"] else T["zz"]
        dc_mult = 8 >> pic["intra_dc_precision"]
        Y = np.zeros((H, W), np.int64)
        U = np.zeros((H // 2, W // 2), np.int64)
        V = np.zeros((H // 2, W // 2), np.int64)
        mbs, qcodes = [], []
        fld = field_pictures and pic["picture_structure"] != 3
        if field_pictures:
            out.fields.append(pic)
            if pic["second"]:                                   # the second field goes into its first field's frame
                out.pictures.pop()
                Y, U, V = held[0]

        def predict_into(col, row, mv, ref=ref):
            cmv = [int(mv[0] / 2), int(mv[1] / 2)]              # toward zero (7.6.3.7)
            return (_predict(ref[0], 16 * col, 16 * row, mv[0], mv[1], 16, False), _predict(ref[1], 8 * col, 8 * row, cmv[0], cmv[1], 8, False),
                    _predict(ref[2], 8 * col, 8 * row, cmv[0], cmv[1], 8, False))

        def predict_b(col, row, fwd, bwd, mvs):
            """a B picture's prediction: from the anchor before the last (forward), the last one (backward), or the mean of both (7.6.7.1)"""
            p = ([predict_into(col, row, mvs[0], before)] if fwd else []) + ([predict_into(col, row, mvs[1], ref)] if bwd else [])
            return p[0] if len(p) == 1 else tuple((a + c + 1) >> 1 for a, c in zip(*p))

        def vector(br, pmv, t, f_code):
            """7.6.3.1: component t from its predictor, the motion code and the residual of f_code"""
            r_size = f_code - 1
            f = 1 << r_size
            m = T["motion"](br)
            if m and br.bits(1):
                m = -m
            delta = m
            if f != 1 and m != 0:
                delta = (abs(m) - 1) * f + br.bits(r_size) + 1
                delta = -delta if m < 0 else delta
            v = pmv[t] + delta
            if v < -16 * f:
                v += 32 * f
            elif v > 16 * f - 1:
                v -= 32 * f
            pmv[t] = v

        def store(col, row, pred, res):
            for b in range(6):
                r = res[b].reshape(8, 8)
                if b < 4:
                    oy, ox = 8 * (b >> 1), 8 * (b & 1)
                    Y[16 * row + oy:16 * row + oy + 8, 16 * col + ox:16 * col + ox + 8] = np.clip(pred[0][oy:oy + 8, ox:ox + 8] + r, 0, 255)
                else:
                    (U if b == 4 else V)[8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pred[b - 3] + r, 0, 255)

        def predict_field(col, row, vecs, sels, ref):
            """7.6.4 for a field-based macroblock: vector r with field select r forms the lines of parity r - 16 x 8 luma at (16 col,
            8 row) of the selected field, 8 x 4 chroma at (8 col, 4 row) with both components halved toward zero (7.6.3.7)"""
            planes = []
            for p, n in ((0, 16), (1, 8), (2, 8)):
                block = np.zeros((n, n), np.int64)
                for r in range(2):
                    mv = vecs[r] if p == 0 else (int(vecs[r][0] / 2), int(vecs[r][1] / 2))
                    block[r::2] = _predict_rect(ref[p][sels[r]::2], n * col, (n // 2) * row, mv[0], mv[1], n, n // 2)
                planes.append(block)
            return tuple(planes)

        def store_il(col, row, pred, res, dct_type):
            """store, or with dct_type 1: luma blocks 0 / 1 are the macroblock's top-field lines, 2 / 3 its bottom-field lines"""
            if not dct_type:
                return store(col, row, pred, res)
            for b in range(6):
                r = res[b].reshape(8, 8)
                if b < 4:
                    y0, ox = 16 * row + (b >> 1), 8 * (b & 1)
                    Y[y0:y0 + 16:2, 16 * col + ox:16 * col + ox + 8] = np.clip(pred[0][(b >> 1)::2, ox:ox + 8] + r, 0, 255)
                else:
                    (U if b == 4 else V)[8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pred[b - 3] + r, 0, 255)

        def read_blocks(br, intra, cbp, dc_pred, qcode):
            """the coded blocks of a macroblock -> six residuals (zeros where the pattern has none)"""
            qscale = _NONLINEAR_SCALE[qcode] if pic["q_scale_type"] else 2 * qcode
            res = []
            for b in range(6):
                r = np.zeros(64, np.int64)
                if (cbp >> (5 - b)) & 1:
                    QF = np.zeros(64, np.int64)
                    k = 0
                    comp = 0 if b < 4 else b - 3
                    if intra:
                        size = (T["dcy"] if b < 4 else T["dcc"])(br)
                        diff = 0
                        if size:
                            d = br.bits(size)
                            diff = d if d >> (size - 1) else d - (1 << size) + 1
                        dc_pred[comp] += diff
                        QF[0] = dc_pred[comp]
                        k = 1
                    first = not intra
                    b15 = mb_tools and intra and pic["intra_vlc_format"]
                    while True:
                        if first and br.peek(1) == 1:
                            br.bits(1)
                            run, lvl = 0, (-1 if br.bits(1) else 1)
                        else:
                            sym = T["ac15"](br) if b15 else T["ac"](br) if not (br.peek(2) == 0b11) else (br.bits(2), (0, 1))[1]
                            if sym == "EOB":
                                assert not first, "a coded non-intra block cannot start with EOB"
                                break
                            if sym == "ESC":
                                run = br.bits(6)
                                lvl = br.bits(12)
                                lvl = lvl - 4096 if lvl & 0x800 else lvl
                                assert lvl not in (0, -2048)
                            else:
                                run, lvl = sym
                                lvl = -lvl if br.bits(1) else lvl
                        first = False
                        k += run
                        assert k < 64, "coefficient index beyond 63"
                        QF[scan[k]] = lvl
                        k += 1
                    r = idct(_main_dequant(QF, intra, qscale, WI if intra else WN, dc_mult), False)
                res.append(r)
            return res

        def slice_extras(br):
            """behind quantiser_scale_code: extra_bit_slice 0 - or, extended, intra_slice_flag 1 with intra_slice, reserved_bits and
            any number of extra_information_slice bytes, each behind an extra_bit_slice 1, closed by a 0"""
            if not extended:
                assert br.bits(1) == 0                          # extra_bit_slice
                return
            if br.bits(1):                                      # intra_slice_flag
                br.bits(8)                                      # intra_slice, reserved_bits: read, not judged
                while br.bits(1):
                    br.bits(8)

        def more(br, col):
            """whether another macroblock follows: up to the row's end - or, extended, while anything but zero bits is left"""
            return col < mbw - 1 if not extended else not br.only_zeros_left()

        span = []                                               # extended: the columns of the slice's first and last macroblock

        def il_slice(br, row):
            """a slice of a picture with frame_pred_frame_dct 0, of any type (the section "Interlaced frame pictures" above); with
            mb_tools a slice of any picture: one with frame_pred_frame_dct 1 has no macroblock_modes() - frame prediction, frame DCT"""
            modes = not pic["frame_pred_frame_dct"]
            conceal = mb_tools and pic["concealment_motion_vectors"]
            qcode = br.bits(5)
            qcodes.append(qcode)
            slice_extras(br)
            ptype = pic["type"]
            refs = (ref, None) if ptype == 2 else (before, ref)  # the anchor of direction s
            dc_pred, col = [0, 0, 0], -1
            PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]          # PMV[r][s]
            dirs = None                                         # the directions of the macroblock in front (None: intra, or none)
            zero = [np.zeros(64, np.int64)] * 6

            def frame_pred(col, used, vecs):
                p = [predict_into(col, row, vecs[s], refs[s]) for s in (0, 1) if used[s]]
                return p[0] if len(p) == 1 else tuple((a + c + 1) >> 1 for a, c in zip(*p))

            def record(used, **kw):
                """what every record of the main syntax carries, and motion_type, dct_type, selects[s][r], vectors[s][r]"""
                m = dict(intra=False, mc=False, skipped=False, mv=(0, 0), cbp=0, qcode=qcode, motion_type=2, dct_type=0,
                         selects=((0, 0), (0, 0)), vectors=(((0, 0), (0, 0)), ((0, 0), (0, 0))))
                m.update(kw)
                if ptype == 3:
                    m.update(fwd=bool(used[0]), bwd=bool(used[1]), mv_b=m["vectors"][1][0] if used[1] else (0, 0))
                mbs.append(m)

            while more(br, col):
                incr = 0
                while True:                                     # macroblock_escape adds 33 (6.3.16)
                    sym = TM["incr"](br)
                    if sym != "ESC":
                        break
                    incr += 33
                    assert col + incr < mbw, "an increment passes the row's end"
                incr += sym
                assert extended or incr == 1 or col >= 0, "a slice starts at the row's first macroblock"
                assert col + incr < mbw, "an increment passes the row's end"
                if extended and col < 0:                        # the first increment places the slice: nothing is skipped in front of it
                    col, incr = incr - 2, 1
                    span[:] = [col + 1, col + 1]
                for k in range(1, incr):                        # 7.6.6: frame prediction, whatever the macroblock in front was
                    assert ptype != 1, "no macroblock is skipped in an I picture"
                    dc_pred = [0, 0, 0]
                    if ptype == 2:                              # the zero vector; the predictors reset
                        PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                        store(col + k, row, frame_pred(col + k, (1, 0), ((0, 0), None)), zero)
                        record(skipped=True, used=(1, 0))
                    else:                                       # the directions in front, PMV[0][s] read as frame vectors
                        assert dirs is not None, "a skipped macroblock behind an intra macroblock"
                        vecs = (tuple(PMV[0][0]), tuple(PMV[0][1]))
                        store(col + k, row, frame_pred(col + k, dirs, vecs), zero)
                        record(skipped=True, mc=bool(dirs[0]), mv=vecs[0] if dirs[0] else (0, 0), used=dirs,
                               vectors=tuple((vecs[s], vecs[s]) if dirs[s] else ((0, 0), (0, 0)) for s in (0, 1)))
                col += incr
                span[1:] = [col]
                bwd = 0
                if ptype == 3:
                    quant, mc, bwd, pattern, intra = TM["type_b"](br)
                else:
                    quant, mc, pattern, intra = (TM["type_i"] if ptype == 1 else TM["type_p"])(br)
                motion_type, dct_type = 2, 0                    # macroblock_modes(): frame_motion_type, dct_type
                if modes and (mc or bwd):
                    motion_type = br.bits(2)
                    assert motion_type in (1, 2) or (mb_tools and motion_type == 3 and ptype == 2), "frame_motion_type 0 is reserved, 3 is dual prime"
                if modes and (intra or pattern):
                    dct_type = br.bits(1)
                if quant:
                    qcode = br.bits(5)
                    assert qcode != 0, "quantiser_scale_code 0 is forbidden"
                sel = [[0, 0], [0, 0]]                          # [s][r]
                vec = [[(0, 0), (0, 0)], [(0, 0), (0, 0)]]      # [s][r]
                for s in (0, 1):
                    if not (mc, bwd)[s]:
                        continue
                    fh, fv = pic["f_code"][2 * s:2 * s + 2]
                    if motion_type == 2:                        # 7.6.3.3: both predictors of the direction follow a frame vector
                        vector(br, PMV[0][s], 0, fh)
                        vector(br, PMV[0][s], 1, fv)
                        PMV[1][s] = list(PMV[0][s])
                        vec[s] = [tuple(PMV[0][s])] * 2
                    elif motion_type == 3:                      # dual prime: one field vector without a select, a dmvector behind each component
                        dmv = [0, 0]
                        vector(br, PMV[0][0], 0, fh)
                        dmv[0] = (1 - 2 * br.bits(1)) if br.bits(1) else 0
                        half = [PMV[0][0][1] >> 1]
                        vector(br, half, 0, fv)
                        dmv[1] = (1 - 2 * br.bits(1)) if br.bits(1) else 0
                        PMV[0][0][1] = 2 * half[0]
                        PMV[1][0] = list(PMV[0][0])
                        vx, vy = PMV[0][0][0], half[0]
                        near = lambda a: (a + (a > 0)) >> 1     # division by 2 to the nearest integer, halves away from zero
                        mt, mb_ = (1, 3) if pic["top_field_first"] else (3, 1)
                        vec[0] = [(vx, vy), (vx, vy)]           # the same parity: top from top, bottom from bottom
                        vec[1] = [(near(mt * vx) + dmv[0], near(mt * vy) + dmv[1] - 1), (near(mb_ * vx) + dmv[0], near(mb_ * vy) + dmv[1] + 1)]
                        sel = [[0, 1], [1, 0]]                  # the opposite parity, as a second direction from the same picture
                    else:
                        for r in (0, 1):                        # 7.6.3.1: the vertical predictor is in frame units - DIV 2 in, times 2 out
                            sel[s][r] = br.bits(1)
                            vector(br, PMV[r][s], 0, fh)
                            half = [PMV[r][s][1] >> 1]
                            vector(br, half, 0, fv)
                            PMV[r][s][1] = 2 * half[0]
                            vec[s][r] = (PMV[r][s][0], half[0])
                if intra and conceal:                           # a frame vector with f_code[0][*] and a marker bit: kept in the predictors, not used
                    vector(br, PMV[0][0], 0, pic["f_code"][0])
                    vector(br, PMV[0][0], 1, pic["f_code"][1])
                    PMV[1][0] = list(PMV[0][0])
                    assert br.bits(1) == 1, "marker_bit"
                elif intra or (ptype == 2 and not mc):
                    PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]  # 7.6.3.4
                cbp = 63 if intra else (T["cbp"](br) if pattern else 0)
                used = (0, 0) if intra else (1, 1) if motion_type == 3 else (1, 0) if ptype == 2 else (mc, bwd)
                if intra:
                    pred = (np.full((16, 16), 128, np.int64), np.full((8, 8), 128, np.int64), np.full((8, 8), 128, np.int64))
                    dirs = None
                else:
                    dc_pred = [0, 0, 0]                         # 7.2.1
                    if motion_type == 2:
                        pred = frame_pred(col, used, (vec[0][0], vec[1][0]))
                    else:
                        p = [predict_field(col, row, vec[s], sel[s], ref if motion_type == 3 else refs[s]) for s in (0, 1) if used[s]]
                        pred = p[0] if len(p) == 1 else tuple((a + c + 1) >> 1 for a, c in zip(*p))
                    dirs = used if motion_type != 3 else (1, 0)
                res = read_blocks(br, intra, cbp, dc_pred, qcode)
                store_il(col, row, pred, res, dct_type)
                record(intra=bool(intra), mc=bool(mc), mv=vec[0][0] if mc else (0, 0), cbp=cbp, qcode=qcode, motion_type=motion_type, dct_type=dct_type,
                       used=used, selects=tuple(tuple(x) for x in sel), vectors=tuple(tuple(x) for x in vec))

        def fp_slice(br, row):
            """a slice of a field picture (the section "Field pictures" above): the field is rows par, par + 2, ... of the frame's planes,
            a reference field the rows of its parity of an anchor frame - or of this frame, for the second field of an anchor frame"""
            par = pic["picture_structure"] - 1
            ptype = pic["type"]
            cur = tuple(p[par::2] for p in (Y, U, V))
            fields_of = lambda frame: [None, None] if frame is None else [tuple(p[q::2] for p in frame) for q in (0, 1)]
            if ptype == 3:
                refs = (fields_of(before), fields_of(ref))
            else:
                refs = (fields_of(ref), [None, None])
                if pic["second"]:                               # the other parity: the first field of this frame
                    refs[0][1 - par] = tuple(p[(1 - par)::2] for p in (Y, U, V))
            conceal = pic["concealment_motion_vectors"]
            qcode = br.bits(5)
            qcodes.append(qcode)
            slice_extras(br)
            dc_pred, col = [0, 0, 0], -1
            PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]          # PMV[r][s]
            dirs = None                                         # the directions of the macroblock in front (None: intra, or none)
            zero = [np.zeros(64, np.int64)] * 6

            def part(field, col, mv, half):
                """one prediction from one field: half None 16 x 16 (chroma 8 x 8), else the upper (0) or lower (1) 16 x 8 (chroma 8 x 4)"""
                assert field is not None, "a select names a field that does not exist"
                cmv = (int(mv[0] / 2), int(mv[1] / 2))          # toward zero (7.6.3.7)
                h, y0 = (16, 0) if half is None else (8, 8 * half)
                return (_predict_rect(field[0], 16 * col, 16 * row + y0, mv[0], mv[1], 16, h),
                        _predict_rect(field[1], 8 * col, 8 * row + y0 // 2, cmv[0], cmv[1], 8, h // 2),
                        _predict_rect(field[2], 8 * col, 8 * row + y0 // 2, cmv[0], cmv[1], 8, h // 2))

            def mean(preds):
                return preds[0] if len(preds) == 1 else tuple((a + c + 1) >> 1 for a, c in zip(*preds))

            def whole(col, used, sel, vec):
                """field-based: one vector a direction, 16 x 16 from the field its select names"""
                return mean([part(refs[s][sel[s]], col, vec[s], None) for s in (0, 1) if used[s]])

            def fstore(col, pred, res):
                for b in range(6):
                    r = res[b].reshape(8, 8)
                    if b < 4:
                        oy, ox = 8 * (b >> 1), 8 * (b & 1)
                        cur[0][16 * row + oy:16 * row + oy + 8, 16 * col + ox:16 * col + ox + 8] = np.clip(pred[0][oy:oy + 8, ox:ox + 8] + r, 0, 255)
                    else:
                        cur[b - 3][8 * row:8 * row + 8, 8 * col:8 * col + 8] = np.clip(pred[b - 3] + r, 0, 255)

            def record(**kw):
                m = dict(intra=False, mc=False, skipped=False, mv=(0, 0), cbp=0, qcode=qcode, motion_type=1, dct_type=0,
                         selects=((par, par), (par, par)), vectors=(((0, 0), (0, 0)), ((0, 0), (0, 0))))
                m.update(kw)
                mbs.append(m)

            while more(br, col):
                incr = 0
                while True:                                     # macroblock_escape adds 33 (6.3.16)
                    sym = TM["incr"](br)
                    if sym != "ESC":
                        break
                    incr += 33
                    assert col + incr < mbw, "an increment passes the row's end"
                incr += sym
                assert col + incr < mbw, "an increment passes the row's end"
                if col < 0:                                     # the first increment places the slice: nothing is skipped in front of it
                    col, incr = incr - 2, 1
                    span[:] = [col + 1, col + 1]
                for k in range(1, incr):                        # 7.6.6: field prediction from the field of the same parity
                    assert ptype != 1, "no macroblock is skipped in an I picture"
                    dc_pred = [0, 0, 0]
                    if ptype == 2:                              # the zero vector; the predictors reset
                        PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]
                        fstore(col + k, whole(col + k, (1, 0), (par, par), ((0, 0), (0, 0))), zero)
                        record(skipped=True)
                    else:                                       # the directions in front, the predictors as the vectors
                        assert dirs is not None, "a skipped macroblock behind an intra macroblock"
                        vecs = (tuple(PMV[0][0]), tuple(PMV[0][1]))
                        fstore(col + k, whole(col + k, dirs, (par, par), vecs), zero)
                        record(skipped=True, mc=bool(dirs[0]), mv=vecs[0] if dirs[0] else (0, 0), fwd=bool(dirs[0]), bwd=bool(dirs[1]))
                col += incr
                span[1:] = [col]
                bwd = 0
                if ptype == 3:
                    quant, mc, bwd, pattern, intra = TM["type_b"](br)
                else:
                    quant, mc, pattern, intra = (TM["type_i"] if ptype == 1 else TM["type_p"])(br)
                motion_type = 1                                 # macroblock_modes(): field_motion_type, no dct_type
                if mc or bwd:
                    motion_type = br.bits(2)
                    assert motion_type in (1, 2) or (motion_type == 3 and ptype == 2), "field_motion_type 0 is reserved, 3 is dual prime"
                if quant:
                    qcode = br.bits(5)
                    assert qcode != 0, "quantiser_scale_code 0 is forbidden"
                preds = []                                      # the predictions to be formed: (field, vector, half)
                sels, vecs = [[par, par], [par, par]], [[(0, 0), (0, 0)], [(0, 0), (0, 0)]]      # [s][r]
                for s in (0, 1):
                    if not (mc, bwd)[s]:
                        continue
                    fh, fv = pic["f_code"][2 * s:2 * s + 2]
                    if motion_type == 1:                        # field-based: from PMV[0][s], PMV[1][s] follows
                        sel = br.bits(1)
                        vector(br, PMV[0][s], 0, fh)
                        vector(br, PMV[0][s], 1, fv)
                        PMV[1][s] = list(PMV[0][s])
                        preds.append([(refs[s][sel], tuple(PMV[0][s]), None)])
                        sels[s], vecs[s] = [sel, sel], [tuple(PMV[0][s])] * 2
                    elif motion_type == 2:                      # 16 x 8: vector r from and into PMV[r][s]
                        both = []
                        for r in (0, 1):
                            sel = br.bits(1)
                            vector(br, PMV[r][s], 0, fh)
                            vector(br, PMV[r][s], 1, fv)
                            both.append((refs[s][sel], tuple(PMV[r][s]), r))
                            sels[s][r], vecs[s][r] = sel, tuple(PMV[r][s])
                        preds.append(both)
                    else:                                       # dual prime: no select, a dmvector behind each component
                        dmv = [0, 0]
                        vector(br, PMV[0][0], 0, fh)
                        dmv[0] = (1 - 2 * br.bits(1)) if br.bits(1) else 0
                        vector(br, PMV[0][0], 1, fv)
                        dmv[1] = (1 - 2 * br.bits(1)) if br.bits(1) else 0
                        PMV[1][0] = list(PMV[0][0])
                        vx, vy = PMV[0][0]
                        near = lambda a: (a + (a > 0)) >> 1     # division by 2 to the nearest integer, halves away from zero
                        other = (near(vx) + dmv[0], near(vy) + dmv[1] + (1 if par else -1))
                        preds.append([(refs[0][par], (vx, vy), None)])
                        preds.append([(refs[0][1 - par], other, None)])
                        sels, vecs = [[par, par], [1 - par, 1 - par]], [[(vx, vy)] * 2, [other] * 2]
                if intra and conceal:                           # a select and a vector: kept in the predictors, not used; then the marker bit
                    br.bits(1)
                    vector(br, PMV[0][0], 0, pic["f_code"][0])
                    vector(br, PMV[0][0], 1, pic["f_code"][1])
                    PMV[1][0] = list(PMV[0][0])
                    assert br.bits(1) == 1, "marker_bit"
                elif intra or (ptype == 2 and not mc):
                    PMV = [[[0, 0], [0, 0]], [[0, 0], [0, 0]]]  # 7.6.3.4
                cbp = 63 if intra else (T["cbp"](br) if pattern else 0)
                if intra:
                    pred = (np.full((16, 16), 128, np.int64), np.full((8, 8), 128, np.int64), np.full((8, 8), 128, np.int64))
                    dirs = None
                else:
                    dc_pred = [0, 0, 0]                         # 7.2.1
                    if not preds:                               # a P field's macroblock without a vector: the zero vector, the same parity
                        preds = [[(refs[0][par], (0, 0), None)]]
                    formed = []
                    for group in preds:                         # a direction: one 16 x 16, or two 16 x 8 one above the other
                        parts = [part(f, col, mv, half) for f, mv, half in group]
                        formed.append(parts[0] if len(parts) == 1 else tuple(np.vstack((a, c)) for a, c in zip(*parts)))
                    pred = mean(formed)
                    dirs = (1, 0) if ptype == 2 else (mc, bwd)
                res = read_blocks(br, intra, cbp, dc_pred, qcode)
                fstore(col, pred, res)
                record(intra=bool(intra), mc=bool(mc), mv=vecs[0][0] if mc else (0, 0), cbp=cbp, qcode=qcode, motion_type=motion_type,
                       selects=tuple(tuple(x) for x in sels), vectors=tuple(tuple(x) for x in vecs), fwd=bool(mc), bwd=bool(bwd))

        front = []                                              # extended: [code, last column] of the slice in front

        def continuity(unit):
            """extended, behind a slice's walk: it has a macroblock; the first slice of a row starts at column 0 behind a row that is
            full, a further one where the slice in front ended; the picture's last slice ends the row"""
            code = ev[unit][1]
            assert span, "a slice without a macroblock"
            if conceal:                                         # per row: the first slice at column 0, a further one where the one in front ended
                st = rowstate.setdefault(code, [True, 0])
                st[0] = st[0] and span[0] == st[1]
                st[1] = span[1] + 1
                return
            if front and front[0] == code:
                assert span[0] == front[1] + 1, "a gap or an overlap between two slices of a row"
            else:
                assert span[0] == 0 and (not front or front[1] == mbw - 1), "a row's first slice starts at column 0, behind a full row"
            assert unit != pic["slices"][-1] or span[1] == mbw - 1, "the picture's last slice ends short"
            front[:] = [code, span[1]]

        rowstate = {}                                           # conceal: slice code -> [every slice so far read and joined, the next column]
        for row, unit in enumerate(pic["slices"]):
            pos = ev[unit][0]
            if conceal and ev[unit][1] > (mbh // 2 if fld else mbh):
                out.conceal["bad_slices"] += 1                  # a code above the picture's rows: counted, not walked
                continue
            if extended:                                        # the slice's code names its row
                row = ev[unit][1] - 1
                del span[:]
            try:
                br = _UnitBits(data, pos, ends[unit])
                if fld:
                    fp_slice(br, row)
                    assert br.rest_is_zero(), "only zero stuffing may follow the row's last macroblock"
                    continuity(unit)
                    continue
                if mb_tools or (interlaced and not pic["frame_pred_frame_dct"]):
                    il_slice(br, row)
                    assert br.rest_is_zero(), "only zero stuffing may follow the row's last macroblock"
                    if extended:
                        continuity(unit)
                    continue
                qcode = br.bits(5)
                qcodes.append(qcode)
                slice_extras(br)
                dc_pred, pmv, col = [0, 0, 0], [0, 0], -1
                pmvs, dirs = [[0, 0], [0, 0]], None             # a B picture's two predictors; the directions of the macroblock in front (None: intra, or none)
                while more(br, col):
                    incr = 0
                    while True:                                 # macroblock_escape adds 33 (6.3.16)
                        sym = TM["incr"](br)
                        if sym != "ESC":
                            break
                        incr += 33
                        assert col + incr < mbw, "an increment passes the row's end"
                    incr += sym
                    assert extended or incr == 1 or col >= 0, "a slice starts at the row's first macroblock"
                    assert col + incr < mbw, "an increment passes the row's end"
                    if extended and col < 0:                    # the first increment places the slice: nothing is skipped in front of it
                        col, incr = incr - 2, 1
                        span[:] = [col + 1, col + 1]
                    for k in range(1, incr) if pic["type"] == 3 else ():      # skipped in a B picture (7.6.6): the directions and vectors in front
                        assert dirs is not None, "a skipped macroblock behind an intra macroblock"
                        dc_pred = [0, 0, 0]
                        store(col + k, row, predict_b(col + k, row, dirs[0], dirs[1], pmvs), [np.zeros(64, np.int64)] * 6)
                        mbs.append(dict(intra=False, mc=bool(dirs[0]), skipped=True, mv=tuple(pmvs[0]) if dirs[0] else (0, 0), cbp=0, qcode=qcode,
                                        fwd=bool(dirs[0]), bwd=bool(dirs[1]), mv_b=tuple(pmvs[1]) if dirs[1] else (0, 0)))
                    for k in range(1, incr) if pic["type"] != 3 else ():      # skipped macroblocks (7.6.6): zero vector, predictors reset
                        assert pic["type"] == 2, "no macroblock is skipped in an I picture"
                        dc_pred, pmv = [0, 0, 0], [0, 0]
                        store(col + k, row, predict_into(col + k, row, (0, 0)), [np.zeros(64, np.int64)] * 6)
                        mbs.append(dict(intra=False, mc=False, skipped=True, mv=(0, 0), cbp=0, qcode=qcode))
                    col += incr
                    span[1:] = [col]
                    bwd = 0
                    if pic["type"] == 3:
                        quant, mc, bwd, pattern, intra = TM["type_b"](br)
                    else:
                        quant, mc, pattern, intra = (TM["type_i"] if pic["type"] == 1 else TM["type_p"])(br)
                    if quant:
                        qcode = br.bits(5)
                        assert qcode != 0, "quantiser_scale_code 0 is forbidden"
                    mv = [0, 0]
                    if pic["type"] == 3:
                        for d in (0, 1) if not intra else ():   # forward with f_code[0][t], backward with f_code[1][t]; an unused direction keeps its predictor
                            for t in range(2) if (mc, bwd)[d] else ():
                                vector(br, pmvs[d], t, pic["f_code"][2 * d + t])
                        if intra:
                            pmvs = [[0, 0], [0, 0]]             # 7.6.3.4
                        dirs = None if intra else (mc, bwd)
                        mv = list(pmvs[0]) if mc else [0, 0]
                    elif mc:
                        for t in range(2):                      # 7.6.3.1
                            r_size = pic["f_code"][t] - 1
                            f = 1 << r_size
                            m = T["motion"](br)
                            if m and br.bits(1):
                                m = -m
                            delta = m
                            if f != 1 and m != 0:
                                delta = (abs(m) - 1) * f + br.bits(r_size) + 1
                                delta = -delta if m < 0 else delta
                            v = pmv[t] + delta
                            if v < -16 * f:
                                v += 32 * f
                            elif v > 16 * f - 1:
                                v -= 32 * f
                            pmv[t] = mv[t] = v
                    else:
                        pmv = [0, 0]                            # 7.6.3.4: an intra macroblock, or a P picture's without a vector
                    cbp = 63 if intra else (T["cbp"](br) if pattern else 0)
                    if intra:
                        pred = (np.full((16, 16), 128, np.int64), np.full((8, 8), 128, np.int64), np.full((8, 8), 128, np.int64))
                    else:
                        dc_pred = [0, 0, 0]                     # 7.2.1
                        pred = predict_b(col, row, mc, bwd, pmvs) if pic["type"] == 3 else predict_into(col, row, mv)
                    qscale = _NONLINEAR_SCALE[qcode] if pic["q_scale_type"] else 2 * qcode
                    res = []
                    for b in range(6):
                        r = np.zeros(64, np.int64)
                        if (cbp >> (5 - b)) & 1:
                            QF = np.zeros(64, np.int64)
                            k = 0
                            comp = 0 if b < 4 else b - 3
                            if intra:
                                size = (T["dcy"] if b < 4 else T["dcc"])(br)
                                diff = 0
                                if size:
                                    d = br.bits(size)
                                    diff = d if d >> (size - 1) else d - (1 << size) + 1
                                dc_pred[comp] += diff
                                QF[0] = dc_pred[comp]
                                k = 1
                            first = not intra
                            while True:
                                if first and br.peek(1) == 1:
                                    br.bits(1)
                                    run, lvl = 0, (-1 if br.bits(1) else 1)
                                else:
                                    sym = T["ac"](br) if not (br.peek(2) == 0b11) else (br.bits(2), (0, 1))[1]
                                    if sym == "EOB":
                                        assert not first, "a coded non-intra block cannot start with EOB"
                                        break
                                    if sym == "ESC":
                                        run = br.bits(6)
                                        lvl = br.bits(12)
                                        lvl = lvl - 4096 if lvl & 0x800 else lvl
                                        assert lvl not in (0, -2048)
                                    else:
                                        run, lvl = sym
                                        lvl = -lvl if br.bits(1) else lvl
                                first = False
                                k += run
                                assert k < 64, "coefficient index beyond 63"
                                QF[scan[k]] = lvl
                                k += 1
                            r = idct(_main_dequant(QF, intra, qscale, WI if intra else WN, dc_mult), False)
                        res.append(r)
                    store(col, row, pred, res)
                    mbs.append(dict(intra=bool(intra), mc=bool(mc), skipped=False, mv=tuple(mv), cbp=cbp, qcode=qcode))
                    if pic["type"] == 3:
                        mbs[-1].update(fwd=bool(mc), bwd=bool(bwd), mv_b=tuple(pmvs[1]) if bwd else (0, 0))
                assert br.rest_is_zero(), "only zero stuffing may follow the row's last macroblock"
                if extended:
                    continuity(unit)
            except Refused:
                raise
            except Exception as e:
                if conceal:                                     # a slice that does not read: its whole row goes
                    out.conceal["bad_slices"] += 1
                    rowstate.setdefault(ev[unit][1], [True, 0])[0] = False
                    continue
                raise Refused(pos, "slice: %s" % e)
        if conceal:
            rows_, par_ = (mbh // 2, pic["picture_structure"] - 1) if fld else (mbh, 0)
            src = before if pic["type"] == 3 else ref           # the frame the forward reference names; an I picture's as if it were P
            hidden = [r for r in range(rows_) if not (rowstate.get(r + 1, [False, 0])[0] and rowstate[r + 1][1] == mbw)]
            for r in hidden:
                for k, (plane, n) in enumerate(((Y, 16), (U, 8), (V, 8))):
                    dst = plane[par_::2] if fld else plane
                    if src is None:
                        dst[n * r:n * r + n] = 128              # a grey row: no frame in front
                    else:
                        dst[n * r:n * r + n] = (src[k][par_::2] if fld else src[k])[n * r:n * r + n]
                out.concealed.append((len(out.fields) - 1, r))
            if hidden:
                c = out.conceal
                c["first_offset"] = min(c["first_offset"], ev[pic["unit"]][0])
                c["concealed_rows"] += len(hidden)
                c["grey_rows"] += len(hidden) if src is None else 0
                c["damaged_pictures"] += 1
        if field_pictures:                                      # a frame is done behind a frame picture or a second field; its type is its first picture's
            out.mbs.append(mbs)
            out.slice_qcodes.append(qcodes)
            if fld and not pic["second"]:
                held = ((Y, U, V), pic["type"])
                continue
            if (held[1] if fld else pic["type"]) != 3:
                before, ref = ref, (Y, U, V)
            out.frames.append(tuple(np.ascontiguousarray(p[:r, :c]).astype(np.uint8)
                                    for p, r, c in zip((Y, U, V), (out.height, ch, ch), (out.width, cw, cw))))
            continue
        if pic["type"] != 3:
            before, ref = ref, (Y, U, V)
        out.frames.append(tuple(np.ascontiguousarray(p[:r, :c]).astype(np.uint8)
                                for p, r, c in zip((Y, U, V), (out.height, ch, ch), (out.width, cw, cw))))
        out.mbs.append(mbs)
        out.slice_qcodes.append(qcodes)
    if b_pictures:
        out.display = display_order([p["type"] for p in (out.pictures if field_pictures else pictures)])
        coded = out.frames
        out.frames = [None] * len(coded)
        for p, d in enumerate(out.display):
            out.frames[d] = coded[p]
    return out
