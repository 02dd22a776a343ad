"""What the stream says about itself (m2v_set_stream_desc): what the encoder must produce - shared by tests/test_desc_cases.py and
tests/test_gpu_stream_desc.py.  Nothing but the header bytes depends on the description, so the stream of a sequence with a description
is an expected stream that gop_cases / scene_cases already build from the oracle, with its first 34 bytes written again from the ISO/IEC
13818-2 field widths, the four time-code bytes of every GOP header counted at the description's frame rate and, with repeat_headers,
the 34 bytes again in front of every GOP after the first.  Everything here comes from the oracle and from the field widths; nothing
looks at what the library computes."""
import functools

import gop_cases as G

M = G.M
SEQ_CODE = b"\x00\x00\x01\xb3"
FIELDS = ("frame_rate_code", "aspect_ratio_information", "bit_rate_400", "vbv_buffer_size_16k", "video_format", "colour_primaries",
          "transfer_characteristics", "matrix_coefficients", "display_width", "display_height", "repeat_headers", "reserved")
MODULE = dict(zip(FIELDS, (2, 1, 10000, 0, 1, 5, 5, 5, 0, 0, 0, 0)))            # RTL:2598-2617
RATE = {1: 24, 2: 24, 3: 25, 4: 30, 5: 30, 6: 50, 7: 60, 8: 60}                 # frames per second the time code counts at


def desc(**fields):
    """the module's description with the given fields replaced, as a dict"""
    assert set(fields) <= set(FIELDS)
    return dict(MODULE, **fields)


def struct(d):
    """a description (dict) as the library's StreamDesc"""
    return M.StreamDesc(*[d[k] for k in FIELDS])


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, width):
        assert 0 <= value < (1 << width), (value, width)
        self.v, self.n = (self.v << width) | value, self.n + width

    def bytes(self):
        pad = -self.n % 8
        return (self.v << pad).to_bytes((self.n + pad) // 8, "big")


def seq_headers(w, h, d):
    """sequence_header + sequence_extension + sequence_display_extension for the printed size w x h, bit by bit"""
    dw, dh = (d["display_width"], d["display_height"]) if d["display_width"] else (w, h)
    b = _Bits()
    for value, width in ((0x000001B3, 32), (w, 12), (h, 12), (d["aspect_ratio_information"], 4), (d["frame_rate_code"], 4),
                         (d["bit_rate_400"] & 0x3FFFF, 18), (1, 1), (d["vbv_buffer_size_16k"] & 0x3FF, 10), (0, 3),
                         (0x000001B5, 32), (1, 4), (0x44, 8), (0, 1), (1, 2), (0, 4), (d["bit_rate_400"] >> 18, 12), (1, 1),
                         (d["vbv_buffer_size_16k"] >> 10, 8), (0, 8),
                         (0x000001B5, 32), (2, 4), (d["video_format"], 3), (1, 1), (d["colour_primaries"], 8),
                         (d["transfer_characteristics"], 8), (d["matrix_coefficients"], 8), (dw, 14), (1, 1), (dh, 14)):
        b.put(value, width)
    out = b.bytes()
    assert len(out) == G.SEQ_HEADER_BYTES
    return out


def time_code(n, code):
    """the four bytes behind 00 00 01 B8 for a GOP that starts at frame n, counted at the frame rate of `code`: the module's formula with
    its 24 replaced by F; the six bits in front saturate at 63; marker, closed_gop = 1, broken_link = 0 and five zero bits"""
    F = RATE[code]
    pic, sec, mnt, hour = n % F, (n // F) % 60, (n // (60 * F)) % 60, min(n // (3600 * F), 63)
    v = (hour << 26) | (mnt << 20) | (1 << 19) | (sec << 13) | (pic << 7) | (2 << 5)
    return v.to_bytes(4, "big")


def printed_size(stream):
    """the size sequence_header prints (12 + 12 bits, stream bytes 4 - 6)"""
    return (stream[4] << 4) | (stream[5] >> 4), ((stream[5] & 15) << 8) | stream[6]


def described(stream, gop_first_frames, d, size=None):
    """an expected stream without a description -> the stream with description d.  gop_first_frames: the frame number of the I picture
    of every GOP, in order; size: the size to print (default: what the stream prints)"""
    head, gops = G.cut(stream)
    assert len(head) == G.SEQ_HEADER_BYTES and head[:4] == SEQ_CODE and len(gops) == len(gop_first_frames)
    w, h = size or printed_size(stream)
    new = seq_headers(w, h, d)
    body = b""
    for k, (g, n) in enumerate(zip(gops, gop_first_frames)):
        assert g[:4] == G.GOP_CODE
        if k and d["repeat_headers"]:
            body += new
        body += g[:4] + time_code(n, d["frame_rate_code"]) + g[8:]
    return G.finish(new + body)


def cadence(nframes, pf):
    """the first frames of the GOPs of the fixed cadence"""
    return list(range(0, nframes, pf + 1))


# the I-only clip: 62 GOPs of one 64 x 64 picture - 62 time codes across the second's rollover at every F
IONLY = dict(W=64, H=64, n=62, index=11, scene_len=62)


@functools.lru_cache(maxsize=None)
def ionly():
    """(frames, W, H) of the I-only clip"""
    c = IONLY
    a = M.synth.clip(c["W"], c["H"], c["n"], c["index"], scene_len=c["scene_len"])
    a.setflags(write=False)
    return a, c["W"], c["H"]
