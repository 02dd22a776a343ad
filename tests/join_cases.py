"""Streams cut from a broadcast in the device decoder (option "decode_join" = M2V_JOIN_HEAD | M2V_JOIN_TAIL on top of "decode_interlaced",
"decode_extended", "decode_mb_tools" and "decode_field_pictures", "decode_b_pictures" either way): the streams it is tried on and what
it must answer - shared by tests/test_join_cases.py (CPU) and tests/test_gpu_decode_join.py.  The definition is the expectation:
decoder.decode(stream, quirks=False, syntax="main", b_pictures=..., interlaced=True, extended=True, mb_tools=True, field_pictures=True,
join=...) - its frames and join record, or the offset its Refused names.  The known answers come from identities the new code did not
make: the definition WITH THE OPTION OFF on the stream the recording was cut from.  Nothing here looks at what the device computes.

The writers write macroblocks from given vectors and coefficients, not from a source, so an open-GOP stream is one stream of the
existing writer (tests/fld_writer.py) in which a later picture carries a sequence header and a GOP header with closed_gop 0: A, the
part in front of that header, is a closed stream; S2, the part from it on, begins with an I frame and B frames that refer to A's last
anchor.  open_gop() asserts that the whole is accepted with the option off - without that the identities show nothing.

Pictures are 16 x 32 (one macroblock a field, two slices a frame picture), 48 x 32 and 48 x 64 with the rows cut in several slices.

host_lib(): the j_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_j_host.hpp compiled with g++."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import ext_cases as EC
import fld_cases as F

M, D, FW, IC, PC = F.M, F.D, F.FW, F.IC, F.PC
Refused = M.decoder.Refused
HEAD, TAIL, BOTH = 1, 2, 3
GOP_OPEN = ("gop", b"\x00\x00\x01\xb8" + bytes([0x00, 0x08, 0x00, 0x00]))      # closed_gop 0, broken_link 0
JOIN_FIELDS = ("join_offset", "tail_offset", "dropped_leading", "dropped_trailing")


def spec(stream, b_pictures, join):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b_pictures, interlaced=True, extended=True, mb_tools=True, field_pictures=True,
                                join=join), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, b_pictures, join):
    key = (bytes(stream), bool(b_pictures), int(join))
    if key not in _specs:
        _specs[key] = spec(*key)
    return _specs[key]


def join_of(d, stream):
    """the join record the definition fixes: of a decoded stream, or of an option-off call"""
    return tuple(int(getattr(d, k)) for k in JOIN_FIELDS) if hasattr(d, "join_offset") else (0, len(stream), 0, 0)


class Join(ctypes.Structure):
    _fields_ = [("join_offset", ctypes.c_uint64), ("tail_offset", ctypes.c_uint64), ("dropped_leading", ctypes.c_uint32), ("dropped_trailing", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


_HARNESS = r"""
#include "dec_j_host.hpp"
extern "C" long long dec_j_host_decode(const uint8_t *es, uint64_t n, int layout, uint8_t *out, uint64_t cap, int b_pictures, int join, unsigned lanes,
                                       dec_host::Record *rec, dec_j_host::Join *jr)
{
    std::vector<uint8_t> frames;
    *rec = dec_j_host::decode(es, n, layout, cap, b_pictures != 0, join, frames, *jr, lanes);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
"""

_host = None


def host_lib():
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_dec_j_host_")
        src, so = os.path.join(d, "dec_j_host.cpp"), os.path.join(d, "libdec_j_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.dec_j_host_decode.restype = ctypes.c_longlong
        L.dec_j_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                        ctypes.POINTER(D.Stat), ctypes.POINTER(Join)]
        _host = L
    return _host


def host_decode(stream, b_pictures, join, layout="i420", lanes=256):
    """-> (frames [n, frame bytes] in display order or None, the record as a dict, the join record as a tuple)"""
    stream = bytes(stream)
    room = 1 << 22
    out = np.zeros(room, np.uint8)
    rec, jr = D.Stat(), Join()
    host_lib().dec_j_host_decode(stream, len(stream), M.LAYOUTS_420[layout], out.ctypes.data, room, int(bool(b_pictures)), int(join), lanes, ctypes.byref(rec), ctypes.byref(jr))
    r = {k: getattr(rec, k) for k in D.STAT_FIELDS}
    j = tuple(int(getattr(jr, k)) for k in JOIN_FIELDS)
    if r["status"] != D.OK:
        return None, r, j
    return out[:r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]).copy(), r, j


record_of = F.record_of


# ---- content ----
def frame(rng, letter, mbw=1, mbh=2, **kw):
    """one frame picture of mbw x mbh macroblocks"""
    return dict(IC.pictures(rng, letter, mbw, mbh, most=1 if mbw == 1 else 3)[0], **kw)


def fpair(rng, letters, first_ps=1, mbw=1, rows=1, anchor=True, **kw):
    return F.pair(rng, letters, first_ps, mbw, rows, anchor=anchor, most=1 if mbw == 1 else 3, **kw)


def units(L, kind):
    return [a for k, a in L["units"] if k == kind]


def open_gop(w, h, a, s2, b=True, **kw):
    """A + S2: -> (stream, log, the offset of S2's sequence header).  The first picture of s2 gets the sequence header and an open GOP
    header; the whole must be accepted with the option off"""
    s2 = [dict(s2[0], seq=True, gop=False, between=[GOP_OPEN] + list(s2[0].get("between", ())))] + list(s2[1:])
    s, L = FW.stream(w, h, list(a) + s2, **kw)
    assert F.spec_cached(s, b)[0] is not None, "A + S2 is refused with the option off"
    return s, L, units(L, "sequence")[1]


def kept_frames(letters):
    """the frames of S2 (their types in coded order) that bit 1 keeps: a B frame goes while fewer than two anchor frames have begun"""
    keep, anchors = [], 0
    for k, c in enumerate(letters):
        if c == "B" and anchors < 2:
            continue
        anchors += c != "B"
        keep.append(k)
    return keep


# ---- I5: name -> (stream, log, the cut, the frames of A, S2's frame types in coded order, dropped_leading stated as a literal) ----
@functools.lru_cache(maxsize=None)
def open_cases():
    out = {}
    rng = np.random.RandomState(101)
    fr = lambda c, **kw: frame(rng, c, **kw)
    # leading B frame pictures
    out["b_frames"] = open_gop(16, 32, [fr("I"), fr("P")], [fr("I"), fr("B"), fr("B"), fr("P"), fr("B")], end=False) + (2, "IBBPB", 2)
    # a leading B field pair, then a B frame picture
    a = fpair(rng, "II") + fpair(rng, "PP", 2)
    s2 = fpair(rng, "II", 2) + fpair(rng, "BB") + [fr("B")] + fpair(rng, "PP") + fpair(rng, "BB", 2)
    out["b_pair"] = open_gop(16, 32, a, s2) + (2, "IBBPB", 2)
    # an I + P field pair as the first anchor frame: its P field finds the first field of its own frame alone
    s2 = fpair(rng, "IP", 1, anchor=False) + fpair(rng, "BB", 2) + fpair(rng, "PP", 2) + fpair(rng, "BB")
    out["ip_anchor"] = open_gop(16, 32, [fr("I"), fr("P")], s2, end=False) + (2, "IBPB", 1)
    # I P with no B; I I
    out["i_p"] = open_gop(16, 32, [fr("I"), fr("P")], [fr("I"), fr("P"), fr("P")]) + (2, "IPP", 0)
    out["i_i"] = open_gop(16, 32, [fr("I"), fr("P")], [fr("I"), fr("B"), fr("I"), fr("B")], end=False) + (2, "IBIB", 1)
    # 48 x 64, the rows cut in several slices: a B pair and a B frame dropped
    a = fpair(rng, "IP", 1, 3, 2, anchor=False, cuts=F._cuts(2)) + fpair(rng, "PP", 2, 3, 2, cuts=F._cuts(2))
    s2 = fpair(rng, "II", 1, 3, 2, cuts=F._cuts(2)[::-1]) + fpair(rng, "BB", 2, 3, 2, cuts=F._cuts(2)) + [frame(rng, "B", 3, 4)] + [frame(rng, "P", 3, 4)] + \
        fpair(rng, "BB", 1, 3, 2, cuts=[[1, 2], [1, 2]])
    out["cut_rows"] = open_gop(48, 64, a, s2, end=False) + (2, "IBBPB", 2)
    # 48 x 32: a quant_matrix_extension carried by a dropped B picture, in force in the kept pictures behind it
    s2 = [frame(rng, "I", 3, 2), frame(rng, "B", 3, 2, extras=[EC.Q(intra=EC.A, non_intra=EC.B_)]), frame(rng, "P", 3, 2), frame(rng, "B", 3, 2)]
    out["matrix_in_a_dropped_b"] = open_gop(48, 32, [frame(rng, "I", 3, 2), frame(rng, "P", 3, 2)], s2) + (2, "IBPB", 1)
    return out


def without_matrix():
    """matrix_in_a_dropped_b's S2 without the extension: other frames - the kept pictures depend on it"""
    s, L, c, na, letters, dropped = open_cases()["matrix_in_a_dropped_b"]
    q = units(L, "quant_matrix")[0]
    end = [a for _, a in L["units"] if a > q][0]
    return s[c:q] + s[end:]


# ---- junk that holds no sequence_header_code ----
def no_b3(data):
    data = bytearray(data)
    at = data.find(b"\x00\x00\x01\xb3")
    while at >= 0:
        data[at + 3] = 0xB2
        at = data.find(b"\x00\x00\x01\xb3")
    return bytes(data)


@functools.lru_cache(maxsize=None)
def junk():
    rng = np.random.RandomState(102)
    s = open_cases()["b_frames"][0]
    out = {}
    out["random"] = no_b3(rng.randint(0, 256, 700).astype(np.uint8).tobytes())
    out["slices"] = b"".join(b"\x00\x00\x01" + bytes([1 + k % 0xAF, 0x5A, 0x80 | k & 0x7F]) for k in range(3000))      # thousands of slice start codes
    out["lone_prefix"] = b"\x00\x00\x01"
    for k in (1, 2, 3):
        out["cut_code_%d" % k] = s[k:12]                            # a cut through the four bytes of the sequence header code itself
    out["picture_tail"] = s[units(open_cases()["b_frames"][1], "slice")[1] + 2:open_cases()["b_frames"][2]]      # the end of a real picture
    assert all(b"\x00\x00\x01\xb3" not in v for v in out.values())
    return out


# ---- I3: a further coded frame, to be cut at every byte ----
@functools.lru_cache(maxsize=None)
def tail_base():
    """S: 16 x 32, I P B without sequence_end_code, accepted; and the further frames X (each begins with its GOP or picture header)"""
    rng = np.random.RandomState(103)
    pics = [frame(rng, "I"), frame(rng, "P"), frame(rng, "B")]
    s, L = FW.stream(16, 32, pics, end=False)
    more = {"frame_picture": [frame(rng, "P")], "gop_and_frame": [dict(frame(rng, "I"), gop=True)], "field_pair": fpair(rng, "PP"), "first_field": fpair(rng, "BB", 2)[:1]}
    out = {}
    for name, x in more.items():
        t, _ = FW.stream(16, 32, pics + x, end=False)
        assert t[:len(s)] == s
        out[name] = t[len(s):]
    return s, L, out


# ---- I6: three open GOPs ----
@functools.lru_cache(maxsize=None)
def three_gops():
    """16 x 32: I P B | I B B P B B | I B (pair) P (pair) B, every GOP with its sequence header and an open GOP header, no end code"""
    rng = np.random.RandomState(104)
    fr = lambda c, **kw: frame(rng, c, **kw)
    head = dict(seq=True, gop=False, between=[GOP_OPEN])
    pics = [fr("I"), fr("P"), fr("B")] + [fr("I", **head), fr("B"), fr("B"), fr("P"), fr("B"), fr("B")]
    g3 = fpair(rng, "II") + fpair(rng, "BB", 2) + fpair(rng, "PP", 2) + [fr("B")]
    g3[0].update(head)
    s, L = FW.stream(16, 32, pics + g3, end=False)
    assert F.spec_cached(s, True)[0] is not None
    return s, L, "IPB" + "IBBPBB" + "IBPB"


# ---- the refusals: name -> (stream, b, join, the offset of the unit the definition must name; None: accepted) ----
@functools.lru_cache(maxsize=None)
def refusals():
    out = {}
    rng = np.random.RandomState(105)
    J = junk()["random"]
    g = len(J)
    fr = lambda c, **kw: frame(rng, c, **kw)

    def s2(pics, **kw):
        """junk + a stream that begins with the sequence header of pics[0]"""
        s, L = FW.stream(16, 32, [dict(pics[0], gop=False, between=[GOP_OPEN])] + list(pics[1:]), **kw)
        return J + s, L

    base, L = s2([fr("I"), fr("B"), fr("P")])
    out["no_sequence_header"] = (J + base[g + units(L, "gop")[0]:], True, HEAD, 0)
    out["no_start_code"] = (bytes([7]) * 40, True, BOTH, 0)
    out["empty_behind_head"] = (J, True, HEAD, 0)
    # a broken header group at J: refused at its own unit although a good one follows
    out["marker_bit_of_the_header_at_j"] = (D.flip(base, 8 * (g + 4) + 50) + base[g:], True, HEAD, g)
    out["no_sequence_extension_at_j"] = (J + base[g:g + units(L, "sequence_ext")[0]] + base[g + units(L, "gop")[0]:], True, HEAD, g + units(L, "sequence_ext")[0])
    s, L = s2([fr("P"), fr("I")])
    out["p_in_front_of_the_first_i"] = (s, True, HEAD, g + units(L, "picture")[0])
    s, L = s2([fr("I"), fr("B"), fr("P")])
    out["b_without_b_pictures"] = (s, False, HEAD, g + units(L, "picture")[1])
    s, L = s2([fr("I"), fr("B", ext=dict(picture_structure=0)), fr("P")])
    out["dropped_b_illegal_extension"] = (s, True, HEAD, g + units(L, "picture_ext")[1])
    p = fpair(rng, "II") + fpair(rng, "BB") + fpair(rng, "PP")
    p[3]["ps"] = p[2]["ps"]
    s, L = s2(p)
    out["dropped_b_same_parity"] = (s, True, HEAD, g + units(L, "picture")[3])
    p = fpair(rng, "II") + fpair(rng, "BB") + fpair(rng, "PP")
    p[3] = F.field(rng, 2, 3 - p[2]["ps"], 1, 1, most=1)
    s, L = s2(p)
    out["dropped_b_p_partner"] = (s, True, HEAD, g + units(L, "picture")[3])
    p = fpair(rng, "II") + fpair(rng, "BB") + fpair(rng, "PP")
    p[3]["gop"] = True
    s, L = s2(p)
    out["gop_between_dropped_fields"] = (s, True, HEAD, g + units(L, "gop")[1])
    p = fpair(rng, "II") + fpair(rng, "BB")
    s, L = s2(p[:3])
    out["dropped_first_field_alone"] = (s, True, HEAD, g + units(L, "picture")[2])
    s, L = s2([fr("I"), fr("B", extras=[EC.Q(intra=EC.A), EC.Q(non_intra=EC.A)]), fr("P")])
    out["dropped_b_two_matrices"] = (s, True, HEAD, g + units(L, "quant_matrix")[1])
    b = fr("B")
    b["slices"].append(dict(b["slices"][1], code=3))
    s, L = s2([fr("I"), b, fr("P")])
    out["dropped_b_slice_code"] = (s, True, HEAD, g + units(L, "slice")[4])
    # a slice that cannot be read: in a kept picture refused, in a dropped one not walked
    bad = [dict(kind="pred", motion="field", motion_bits=0, fwd=(0, (0, 0)))]
    p = fpair(rng, "II") + fpair(rng, "BB") + fpair(rng, "PP")
    p[4]["slices"][0]["mbs"] = bad
    s, L = s2(p)
    out["slice_fault_kept"] = (s, True, HEAD, g + units(L, "slice")[4])
    p = fpair(rng, "II") + fpair(rng, "BB") + fpair(rng, "PP")
    p[2]["slices"][0]["mbs"] = [dict(bad[0], bwd=None)]
    s, L = s2(p)
    out["slice_fault_dropped"] = (s, True, HEAD, None)
    out["slice_fault_dropped_option_off"] = (s[g:], True, 0, units(L, "picture")[2])
    # a second sequence header that differs from the one at J
    other, Lo = FW.stream(32, 32, [frame(rng, "I", 2, 2)])
    s, L = s2([fr("I"), fr("P")], end=False)
    out["other_sequence_header"] = (s + other, True, HEAD, len(s))
    # D pictures stay refused
    s, L = s2([fr("I"), fr("P")])
    at = g + units(L, "picture")[1]
    out["d_picture"] = (s[:at + 5] + bytes([s[at + 5] & 0xC7 | 4 << 3]) + s[at + 6:], True, BOTH, at)
    # the tail alone does not look for a join point
    out["tail_with_junk_in_front"] = (base, True, TAIL, 0)
    # a first field, then a picture header that does not read: the partner, whatever it is - the frame goes as a whole
    ts, tL, more = tail_base()
    ff = more["first_field"]
    out["first_field_in_front_of_the_tail"] = (ts + ff + b"\x00\x00\x01\x00\x00\x0f", True, TAIL, None)
    # the tail alone on a stream whose first unit is its only picture start code: F is that unit, nothing is left of the stream
    out["tail_only_a_picture_start_code"] = (b"\x00\x00\x01\x00", True, TAIL, 0)
    at = units(tL, "picture")[0]
    out["tail_begins_at_a_picture_header"] = (ts[at:at + 6], True, TAIL, 0)
    out["tail_zeros_then_a_picture_start_code"] = (bytes(5) + b"\x00\x00\x01\x00\x12", True, TAIL, 0)
    out["p_first_with_both_bits"] = (out["p_in_front_of_the_first_i"][0][:-4], True, BOTH, out["p_in_front_of_the_first_i"][3])
    return out


# ---- plan streams: more than 256 events behind J ----
def _long_pictures(frames, seed, lead):
    """I, `lead` B frames (pairs and frame pictures in turn), then P B B ... of 16 x 32, a repeated sequence header now and then"""
    rng = np.random.RandomState(seed)
    letters = "I" + "B" * lead + "PBB" * frames
    pics = []
    for f, c in enumerate(letters[:frames]):
        if c != "I" and f % 4 == 3:
            new = [frame(rng, c)]
        else:
            new = fpair(rng, "IP" if c == "I" else c + c, 1 + (f // 3) % 2, anchor=f > 0)
        if f and f % 15 == 0 and c == "P":
            new[0].update(seq=True, gop=True)
        pics += new
    return pics, letters[:frames]


@functools.lru_cache(maxsize=None)
def plan_streams():
    """name -> (stream, b, join).  shift_k: k + 1 slice start codes of junk in front, k user_data units behind the sequence's extensions
    and a tail cut k bytes into its last frame: J, the first two anchor frames, the dropped B pairs, F and T fall at every position
    of a range of two events.  long: more than 256 kept frames.  long_junk: junk that holds more start codes than the event list's
    first size.  wide_k: more than 512 events behind J, three a range.  tests/test_join_cases.py
    states with reached() which positions of a range each of them meets"""
    out = {}
    for k in range(7):
        pics, letters = _long_pictures(64, 106, 2 + k % 3)
        s, L = FW.stream(16, 32, [dict(pics[0], gop=False, between=[GOP_OPEN])] + pics[1:], seq=dict(extras_behind=PC.users(k, 3)), end=False)
        assert len(L["fields"]) == len(units(L, "picture"))
        last = units(L, "picture")[max(i for i, f in enumerate(L["fields"]) if not f["second"])]      # the last picture that begins a frame
        stream = junk()["slices"][:6 * (k + 1)] + s[:last + 5 + 3 * k]
        assert 256 < len(M.decoder.start_codes(stream)) <= 512
        out["shift_%d" % k] = (stream, True, BOTH)
    pics, letters = _long_pictures(300, 107, 3)
    s, L = FW.stream(16, 32, [dict(pics[0], gop=False, between=[GOP_OPEN])] + pics[1:], end=False)
    out["long"] = (junk()["random"] + s, True, HEAD)
    j = junk()["slices"]
    assert len(M.decoder.start_codes(j)) > PC.first_guess(len(j) + len(s)) if hasattr(PC, "first_guess") else True
    out["long_junk"] = (j + s[:len(s) // 3], True, BOTH)
    for k in range(3):
        out["wide_%d" % k] = wide_stream(k)
    return out


def wide_stream(k):
    """-> (stream, b, join): more than 512 events behind J, so that a lane's range holds three; k user_data units behind the sequence's
    extensions move every edge"""
    pics, letters = _long_pictures(130, 109, 3)
    s, L = FW.stream(16, 32, [dict(pics[0], gop=False, between=[GOP_OPEN])] + pics[1:], seq=dict(extras_behind=PC.users(k, 5)), end=False)
    return junk()["cut_code_2"] + s[:-7], True, BOTH


def reached(stream, b, join):
    """from the start codes and the definition's join record alone: where the plan's ranges - `per` events each, cut behind J's event;
    `per0` over the whole list for the search of J - meet what the plan carries across them.  -> dict(per, per0, J: position of J's
    event in a range of the whole list, E1 / E2 / F / T: positions in a range behind J of the pictures that begin the first two
    anchor frames, of the picture that begins the frame the tail drops and of T's unit, dropped_pair_straddles: whether the two
    fields of some dropped B pair lie in two ranges, dropped_pair_inside: whether those of some pair lie in one)"""
    d, _ = spec_cached(stream, b, join)
    ev = M.decoder.start_codes(stream)
    offs = [p for p, _ in ev]
    jev, n = offs.index(d.join_offset), len(ev)
    per0, per = -(-n // 256), -(-(n - jev) // 256)
    out = dict(per=per, per0=per0, J=jev % per0, dropped_pair_straddles=False, dropped_pair_inside=False)
    waiting, anchors, begins = None, [], []
    for i in range(jev, n):
        pos, code = ev[i]
        if code != 0x00 or pos + 5 >= len(stream):
            continue
        ptype = (stream[pos + 5] >> 3) & 7
        field = i + 1 < n and ev[i + 1][1] == 0xB5 and ev[i + 1][0] + 6 < len(stream) and stream[ev[i + 1][0] + 4] >> 4 == 8 and \
            stream[ev[i + 1][0] + 6] & 3 in (1, 2)
        if waiting is not None:
            first, gone = waiting
            if gone:
                same = (first - jev) // per == (i - jev) // per
                out["dropped_pair_inside" if same else "dropped_pair_straddles"] = True
            waiting = None
            continue
        begins.append(i)
        gone = ptype == 3 and len(anchors) < 2
        if ptype != 3:
            anchors.append(i)
        if field:
            waiting = (i, gone)
    out["E1"], out["E2"] = ((a - jev) % per for a in anchors[:2])
    if d.dropped_trailing:
        out["F"] = (begins[-1] - jev) % per
        out["T"] = (offs.index(d.tail_offset) - jev) % per
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    """junk, an open GOP of field pairs and frame pictures of 16 x 32, a tail cut in its last frame"""
    rng = np.random.RandomState(108)
    pics = fpair(rng, "IP", 1, anchor=False) + fpair(rng, "BB", 2) + [frame(rng, "B")] + fpair(rng, "PP", 2) + fpair(rng, "BB") + [frame(rng, "P")]
    s, L = FW.stream(16, 32, [dict(pics[0], gop=False, between=[GOP_OPEN])] + pics[1:], end=False)
    return junk()["cut_code_2"], s[:-9], L


@functools.lru_cache(maxsize=None)
def altered(n=300):
    """[(name, stream)]: seeded bit flips, cuts and insertions anywhere behind the junk (decoded with "decode_b_pictures" on, join 3)"""
    j, s, L = altered_base()
    rng = np.random.RandomState(9)
    out = []
    for k in range(n):
        kind = k % 5
        if kind < 3:
            bit = int(rng.randint(0, 8 * len(s)))
            out.append(("flip%d" % bit, j + D.flip(s, bit)))
        elif kind == 3:
            cut = int(rng.randint(8, len(s)))
            out.append(("cut%d" % cut, j + s[:cut]))
        else:
            ins = int(rng.randint(4, len(s)))
            out.append(("ins%d" % ins, j + s[:ins] + bytes([int(rng.randint(0, 256))]) + s[ins:]))
    return out


def all_streams():
    """every stream of this file with the settings it is decoded under: (name, stream, b_pictures, join)"""
    out = []
    for name, (s, L, c, na, letters, dropped) in sorted(open_cases().items()):
        out += [("open_%s_%d" % (name, j), s[c:], True, j) for j in (1, 2, 3)] + [("open_%s_whole" % name, s, True, 3)]
    out += [("junk_" + n, v + open_cases()["b_pair"][0][open_cases()["b_pair"][2]:], True, 1) for n, v in sorted(junk().items())]
    out += [("refusal_" + n, v[0], v[1], v[2]) for n, v in sorted(refusals().items())]
    out += [("plan_" + n, v[0], v[1], v[2]) for n, v in sorted(plan_streams().items())]
    return out + [(n, s, True, 3) for n, s in altered()]
