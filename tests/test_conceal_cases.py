"""Damaged slices (option "decode_conceal"), on the CPU: decoder.decode(..., conceal=True) - the definition - and the g++ build of the
device's own functions (tools/dec_c_host.hpp over the c_ functions of csrc/m2v_decode_kernels.hpp) held to each other on every stream of
tests/conceal_cases.py - frames, record, join record and report, planned in 256 ranges of events, in one, and in numbers between - and
both held to answers the new code did not make:
   twins       the damaged stream equals the option-off decode of the twin the writer wrote with the concealed rows as forward,
               zero-vector, not-coded macroblocks, the pictures behind it included
   splice      I pictures alone against numpy: row r of frame n from the already spliced frame n - 1, grey in the first
   literals    every report from how the damage was made; a grey row is 128 in the cropped frame
   invariance  every stream the field-picture and join tests accept keeps bytes, record and join record, with a report of zeros
   refusals    each header rule stays a refusal at the offset stated from the writer's log
   wrong forms eight other ways to conceal, each shown to change a case
The refusals' offsets are stated by hand from the writer's log."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import conceal_cases as C

M, D, F, J = C.M, C.D, C.F, C.J
LANES = (256, 1, 2, 5, 37)


def frames_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for x, y in zip(a, b) for p, q in zip(x, y))


def agree(stream, b, join=0, lanes=(256,), layout="i420"):
    """the host build answers what the definition answers, planned in every number of ranges -> the definition's answer (None: refused)"""
    d, at = C.spec_cached(stream, b, join)
    for n in lanes:
        got, r, jr, cr = C.host_decode(stream, b, join, layout, n)
        if d is None:
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at) and jr == (0, len(stream), 0, 0) and cr == C.no_report(stream), (n, r, at)
            continue
        assert got is not None, (n, r)
        want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
        assert got.shape == want.shape and np.array_equal(got, want), n
        rec = C.record_of(d, stream)
        assert {k: int(r[k]) for k in rec} == rec and jr == J.join_of(d, stream) and cr == C.report_of(d, stream), (n, r, rec, jr, cr)
    return d


def test_keyword_rules():
    s = C.cases()["f16_1Pt_unreadable"]["stream"]
    kw = dict(quirks=False, syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True)
    for missing in ("interlaced", "extended", "mb_tools", "field_pictures"):
        with pytest.raises(ValueError):
            M.decoder.decode(s, conceal=True, **dict(kw, **{missing: False}))
    with pytest.raises(ValueError):
        M.decoder.decode(s, conceal=True, **dict(kw, syntax="module", quirks=True))
    with pytest.raises(M.decoder.Refused):
        M.decoder.decode(s, conceal=False, **kw)
    d = M.decoder.decode(s, conceal=True, **kw)
    assert d.conceal["bad_slices"] == 1 and d.concealed == [(1, 0)]


@pytest.mark.parametrize("base", sorted(C.bases()))
def test_cases(base):
    """every kind of damage in every picture of the base: the report is the literal, the frames are the twin's, the host build agrees;
    with the option off the stream is refused"""
    names = [n for n in sorted(C.cases()) if C.cases()[n]["base"] == base]
    assert len(names) >= 25
    kinds = {n.split("_", 2)[2] for n in names}
    assert {"unreadable", "removed", "no_slices", "code_af", "duplicated"} <= kinds
    twins = shown = 0
    for k, name in enumerate(names):
        c = C.cases()[name]
        s, b = c["stream"], c["b"]
        assert F.spec_cached(s, b)[0] is None, name                 # refused by the parent
        d = agree(s, b, 0, LANES if k % 6 == 0 else (256, 3), D.LAYOUTS[k & 3])
        assert d is not None and C.report_of(d, s) == c["report"], (name, C.report_of(d, s), c["report"])
        assert d.concealed == [(c["pic"], r) for r in c["rows"]], name
        clean = F.spec_cached(C.base_stream(base)[0], b)[0]
        assert C.record_of(d, s) == dict(C.record_of(clean, s), es_bytes=len(s)), name      # the record of the undamaged stream
        if c["twin"] is not None:
            t = F.spec_cached(c["twin"], b)[0]
            assert t is not None and frames_equal(d.frames, t.frames), name
            shown += not frames_equal(d.frames, clean.frames)
            twins += 1
    assert twins >= (0 if base == "i48" else 10)
    assert base in ("i48", "z48") or shown >= twins // 2, (shown, twins)      # the damage shows (but in a cropped row, or over a flat patch)


def test_cases_cover_every_picture_kind():
    """each kind of damage on an I, a P and a B picture, on a frame picture and on either field"""
    seen = {(C.shape(c["base"], c["pic"])[3], C.shape(c["base"], c["pic"])[2], n.split("_", 2)[2]) for n, c in C.cases().items()}
    for kind in ("unreadable", "removed", "no_slices", "code_af", "duplicated"):
        assert {(t, p) for t, p, k in seen if k == kind} == {(t, p) for t in (1, 2, 3) for p in (1, 2, 3)}, kind
    assert {(t, p) for t, p, k in seen if k == "last_rows"} >= {(t, p) for t in (1, 2, 3) for p in (1, 2, 3)}
    assert {(t, p) for t, p, k in seen if k == "code_other"} >= {(t, p) for t in (1, 2, 3) for p in (1, 2, 3)}
    for kind in ("one_of_three", "exchanged"):                      # the rows cut in three
        assert {(t, p) for t, p, k in seen if k == kind} == {(t, p) for t in (1, 2, 3) for p in (1, 2, 3)}, kind
    # a second I field with a frame in front of it (not a grey one), a row of three slices
    c = C.cases()["t48_7It_one_of_three"]
    assert C.base_stream("t48")[1]["fields"][7]["second"] and not c["grey"]


def test_chains():
    for name, c in sorted(C.chains().items()):
        d = agree(c["stream"], c["b"], c["join"], LANES)
        assert d is not None and C.report_of(d, c["stream"]) == c["report"], name
        assert sorted(d.concealed) == sorted((p, r) for p, rows in c["hidden"].items() for r in rows)
        t = F.spec_cached(c["twin"], c["b"])[0]
        assert t is not None and frames_equal(d.frames, t.frames), name


def test_all_i_stream_against_the_splice():
    """I pictures alone, a row gone in every second picture and then in every picture: numpy splices row r of frame n from the already
    spliced frame n - 1; the first frame's row is grey"""
    s, L = C.base_stream("i48")
    clean = F.spec_cached(s, False)[0]
    frame_of = [f["frame"] for f in L["fields"]]
    for step in (2, 1):
        x, hidden = s, {}
        for pic in range(len(L["fields"]) - 1, -1, -step):
            x = C.unreadable(x, pic, 0)
            hidden.setdefault(frame_of[pic], []).extend(C.lines_of("i48", pic, C.rows_of("i48", pic, [0])))
        d = agree(x, False, 0, LANES)
        want = C.splice(clean.frames, hidden)
        assert frames_equal(d.frames, want), step
        last = (d, want)
        n = len(range(len(L["fields"]) - 1, -1, -step))
        grey = 1 if 0 in hidden else 0
        assert C.report_of(d, x) == (C.picture_offset(x, min(p for p in range(len(L["fields"]) - 1, -1, -step))), n, n, grey, n)
    # unspliced: from the clean frame in front - another answer where two frames in a row are damaged (wrong form 7)
    unspliced = [C.splice([clean.frames[n - 1] if n else f, f], {1: hidden.get(n, [])})[1] if n else C.splice([f], {0: hidden.get(0, [])})[0]
                 for n, f in enumerate(clean.frames)]
    assert not frames_equal(unspliced, want) and frames_equal(unspliced[:1], want[:1])
    assert frames_equal(last[0].frames, last[1]) and not frames_equal(last[0].frames, unspliced)      # the decode is the spliced one, not this


def test_grey_row_literal():
    """the first picture of 48 x 48 (a frame picture, cropped) without its last two rows: lines 32 .. 47 are 128 in all three planes"""
    c = C.cases()["o48_0If_last_rows"]
    d = agree(c["stream"], c["b"], 0, LANES)
    assert c["report"] == (C.picture_offset(c["stream"], 0), 0, 2, 2, 1) and c["rows"] == [2, 3]
    Y, U, V = d.frames[0]
    assert Y.shape == (48, 48) and (Y[32:] == 128).all() and (U[16:] == 128).all() and (V[16:] == 128).all()
    clean = F.spec_cached(C.base_stream("o48")[0], True)[0]
    assert np.array_equal(Y[:32], clean.frames[0][0][:32]) and not (clean.frames[0][0][32:] == 128).all()
    # both fields of the first frame of 80 x 32
    for name in ("s80_0It_no_slices", "s80_1Ib_no_slices"):
        c = C.cases()[name]
        d = agree(c["stream"], c["b"], 0)
        par = C.shape("s80", c["pic"])[2] - 1
        assert c["report"][2:] == (1, 1, 1) and (d.frames[0][0][par::2] == 128).all() and not (d.frames[0][0][1 - par::2] == 128).all()


def test_accepted_streams_keep_their_answer():
    """every stream the field-picture tests accept, under "decode_join" 0 and 3; the join's open GOPs under 3"""
    n = 0
    for name, s, b in F.all_streams():
        d0, at = F.spec_cached(s, b)
        if d0 is None:
            continue
        for join in (0, 3):
            want = d0 if join == 0 else J.spec_cached(s, b, 3)[0]
            if want is None:
                continue
            d = agree(s, b, join, (256, 3) if len(s) < 20000 else (256,))
            assert d is not None and frames_equal(d.frames, want.frames) and C.record_of(d, s) == C.record_of(want, s), (name, join)
            assert J.join_of(d, s) == J.join_of(want, s) and C.report_of(d, s) == C.no_report(s), (name, join)
            n += 1
    assert n >= 40
    for name, (s, L, c, na, letters, dropped) in sorted(J.open_cases().items()):
        want = J.spec_cached(s[c:], True, 3)[0]
        d = agree(s[c:], True, 3, (256, 2))
        assert frames_equal(d.frames, want.frames) and J.join_of(d, s[c:]) == J.join_of(want, s[c:]) and C.report_of(d, s[c:]) == C.no_report(s[c:]), name


def test_the_join_tests_streams_keep_their_answer():
    """every stream of tests/join_cases.py that the join accepts - the open GOPs under 1, 2 and 3, junk in front, the plan streams, the
    accepted ones of its refusal list, every tenth altered one - and the tail cut at every seventh byte of each further frame: under its
    own "decode_join", and under 0 and 3 where those accept it too, the same frames, record and join record, a report of zeros"""
    streams = [(n, s, b, join) for n, s, b, join in J.all_streams() if not n.startswith(("flip", "cut", "ins"))]
    streams += [v for v in J.all_streams() if v[0].startswith(("flip", "cut", "ins"))][::10]
    base, L, more = J.tail_base()
    for name, x in sorted(more.items()):
        streams += [("tail_%s_%d" % (name, n), base + x[:n], True, 2) for n in range(1, len(x), 7)]
    n = 0
    for name, s, b, own in streams:
        for join in sorted({own, 0, 3}):
            want = (J.spec_cached(s, b, join) if join else F.spec_cached(s, b))[0]
            if want is None:
                continue
            d = agree(s, b, join, (256, 3) if len(s) < 4000 else (256,))
            assert d is not None and frames_equal(d.frames, want.frames) and C.record_of(d, s) == C.record_of(want, s), (name, join)
            assert J.join_of(d, s) == J.join_of(want, s) and C.report_of(d, s) == C.no_report(s), (name, join)
            n += 1
    assert n >= 80, n


def test_join_and_damage():
    g = J.junk()["random"]
    c = C.cases()["c48_2Pf_unreadable"]
    x = g + c["stream"][:-4]
    d = agree(x, True, 3, LANES)
    assert d is not None and (d.join_offset, d.dropped_trailing) == (len(g), 1)
    assert C.report_of(d, x) == (c["report"][0] + len(g),) + c["report"][1:]
    whole = C.spec_cached(c["stream"], True, 0)[0]
    assert frames_equal(d.frames, whole.frames[:len(d.frames)]) and len(d.frames) == len(whole.frames) - 1


def test_refusals_stay():
    cases = C.refusals()
    assert len(cases) >= 12
    s, L = C.base_stream("c48")
    assert cases["damaged_then_type_0"][3] == C.J.units(L, "picture")[5] and cases["no_coding_extension"][3] == C.J.units(L, "picture")[4]
    for name, (s, b, join, want) in sorted(cases.items()):
        assert agree(s, b, join, LANES) is None and C.spec_cached(s, b, join)[1] == want, (name, C.spec_cached(s, b, join), want)
        if not name.startswith(("damaged", "no_coding")):
            off = J.spec_cached(s, b, join) if join else F.spec_cached(s, b)
            assert off == (None, want), name                        # the same unit as with the option off
    for rule, name in sorted(C.RULES.items()):                      # each header rule by name: a case of its own, refused under the option
        assert name in cases, rule
    s, b, join, want = cases["second_quant_matrix_extension"]
    assert dict(M.decoder.start_codes(s))[want] == 0xB5 and s[want + 4] >> 4 == 3
    assert [p for p, c in M.decoder.start_codes(s) if c == 0xB5 and s[p + 4] >> 4 == 3][1] == want


def test_wrong_forms():
    """other ways to conceal, each another answer on a case where the right one is the definition's"""
    def differs(name, wrong):
        c = C.cases()[name]
        d = C.spec_cached(c["stream"], c["b"])[0]
        right = F.spec_cached(c["twin"], c["b"])[0]
        w = F.spec_cached(wrong, c["b"])[0]
        assert w is not None, name
        return frames_equal(d.frames, right.frames) and not frames_equal(d.frames, w.frames)
    hid = lambda name: {C.cases()[name]["pic"]: C.cases()[name]["rows"]}
    # 1: from the backward frame in a B picture
    assert differs("c48_5Bf_unreadable", C.twin("c48", hid("c48_5Bf_unreadable"), "bwd"))
    assert differs("o48_3Bt_no_slices", C.twin("o48", hid("o48_3Bt_no_slices"), "bwd"))
    # 2: a second P field from its own frame - the other parity is its own frame's first field
    assert C.shape("c48", 7)[3] == 2 and C.base_stream("c48")[1]["fields"][7]["second"]
    assert differs("c48_7Pt_no_slices", C.twin("c48", hid("c48_7Pt_no_slices"), "other_parity"))
    # 3: the opposite parity of the frame in front (a first field, a B field)
    assert not C.base_stream("o48")[1]["fields"][1]["second"]
    assert differs("o48_1Pb_no_slices", C.twin("o48", hid("o48_1Pb_no_slices"), "other_parity"))
    assert differs("c48_3Bb_no_slices", C.twin("c48", hid("c48_3Bb_no_slices"), "other_parity"))
    # 4: only the bad slice of a cut row
    c = C.cases()["c48_2Pf_one_of_three"]
    k, row = c["cut"]
    assert differs("c48_2Pf_one_of_three", C.twin("c48", {2: [row]}, {(2, row): [1]}))
    # 5: keeping an overlapping pair (a slice twice): the clean stream
    assert differs("c48_2Pf_duplicated", C.base_stream("c48")[0]) and differs("f16_6Pf_duplicated", C.base_stream("f16")[0])
    # 6: grey where a reference exists - the twin's frames with the row's lines at 128 in the damaged frame (the last one: nothing
    # predicts from it) are another answer
    c = C.cases()["o48_5Pf_unreadable"]
    d = C.spec_cached(c["stream"], True)[0]
    right = F.spec_cached(c["twin"], True)[0]
    grey = [tuple(p.copy() for p in f) for f in right.frames]
    (r,) = c["rows"]
    n = d.display[3]                                                # coded frame 3 (coded pictures 0, 1 + 2, 3 + 4, 5)
    assert n == len(d.frames) - 1 and 16 * r + 16 <= 48
    grey[n][0][16 * r:16 * r + 16] = 128
    grey[n][1][8 * r:8 * r + 8] = 128
    grey[n][2][8 * r:8 * r + 8] = 128
    assert frames_equal(d.frames, right.frames) and not frames_equal(d.frames, grey)
    # 7: an I picture that does not wait for its reference: test_all_i_stream_against_the_splice holds the decode against the unspliced form
    # 8: first_offset at the slice; 9: a bad code counted as a concealed row of its own; 10: a removed slice counted as bad - each
    # against the report the decode gives
    c = C.cases()["c48_5Bf_unreadable"]
    got = C.report_of(C.spec_cached(c["stream"], True)[0], c["stream"])
    assert got[0] == C.picture_offset(c["stream"], 5) and got[0] != C.slice_offset(c["stream"], 5, len(C.slice_codes(c["stream"], 5)) // 2)
    c = C.cases()["c48_5Bf_code_af"]
    assert C.report_of(C.spec_cached(c["stream"], True)[0], c["stream"])[1:3] == (1, 1)
    c = C.cases()["c48_5Bf_removed"]
    assert C.report_of(C.spec_cached(c["stream"], True)[0], c["stream"])[1:3] == (0, 1)


@pytest.mark.parametrize("name", sorted(C.plan_streams()))
def test_plan_streams(name):
    s, b, join = C.plan_streams()[name]
    d = agree(s, b, join, LANES if name != "long" else (256, 5))
    assert d is not None and d.conceal["damaged_pictures"] > 10 and d.conceal["bad_slices"] > 4
    assert len(M.decoder.start_codes(s)) > 256
    if name == "long":
        assert len(d.frames) > 256


def test_plan_streams_reach_every_position():
    """a picture without a slice, and an unreadable first slice, at every position of a range of two and of three events; the search
    for a slice's picture passes slice-less pictures at the front, in the middle and at the end (the host build refuses otherwise)"""
    two = [C.reached(C.plan_streams()["two_%d" % k][0]) for k in range(4)]
    assert all(r[0] == 2 for r in two)
    assert set().union(*(r[1] for r in two)) == {0, 1} and set().union(*(r[2] for r in two)) == {0, 1}
    three = [C.reached(C.plan_streams()["three_%d" % k][0]) for k in range(3)]
    assert all(r[0] == 3 for r in three)
    assert set().union(*(r[1] for r in three)) == {0, 1, 2} and set().union(*(r[2] for r in three)) == {0, 1, 2}
    s, L = C.base_stream("c48")
    n = len(L["fields"])
    for gone in ([0], [n - 1], [3], [0, 1, 2], [n - 2, n - 1], [2, 3, 4], list(range(n))):
        x = s
        for pic in sorted(gone, reverse=True):
            x = C.removed(x, pic, None)
        d = agree(x, True, 0, LANES)
        assert d is not None and d.conceal["damaged_pictures"] == len(gone) and d.conceal["bad_slices"] == 0, gone


FLIPS_REPORTED = 121             # the flips of the 300 whose report is not of zeros


def test_seeded_flips():
    """300 single-bit flips in slice payloads that leave the start codes alone: every one M2V_DEC_OK; the share with a report at least
    a quarter (the parent's definition refuses 82 of 200 such flips)"""
    flips = C.flips()
    assert len(flips) == 300
    s, L = F.altered_base()
    reports = 0
    for k, (name, x) in enumerate(flips):
        assert M.decoder.start_codes(x) == M.decoder.start_codes(s)
        d = agree(x, True, 0, (256, 4) if k % 10 == 0 else (256,))
        assert d is not None, name
        reports += C.report_of(d, x) != C.no_report(x)
    assert reports >= 75, reports
    assert reports == FLIPS_REPORTED, reports


def test_sanitizers():
    """every stream of conceal_cases.all_streams() through tools/dec_c_host_check.cpp built with AddressSanitizer and UBSan: a stand-alone
    program, each stream in an allocation of exactly its size, every walk into a heap block of exactly its row; its verdicts are the
    definition's"""
    streams = C.all_streams()
    root = D.ROOT
    d = tempfile.mkdtemp(prefix="m2v_dec_c_check_")
    exe, path = os.path.join(d, "dec_c_host_check"), os.path.join(d, "streams.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "fpga-mpeg2-encoder_amd", "csrc"),
                           "-I", os.path.join(root, "tools"), os.path.join(root, "tools", "dec_c_host_check.cpp"), "-o", exe])
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for name, s, b, join in streams:
            f.write(struct.pack("<IQ", int(bool(b)) | join << 1, len(s)) + bytes(s))
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == len(streams)
    for line, (name, s, b, join) in zip(lines[::5], streams[::5]):
        k, status, err, pictures, first, bad, rows, grey, pics, _ = line.split()
        d_, at = C.spec_cached(s, b, join)
        if d_ is None:
            assert (int(status), int(err)) == (D.SYNTAX, at), name
        else:
            assert (int(status), int(pictures), int(first), int(bad), int(rows), int(grey), int(pics)) == (D.OK, len(d_.frames)) + C.report_of(d_, s), name
