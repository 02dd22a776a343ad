"""Interlaced frame pictures (option "decode_interlaced") on the CPU: the il_ functions of csrc/m2v_decode_kernels.hpp and the serial
harness tools/dec_i_host.hpp, compiled with g++, against decoder.decode(..., syntax="main", interlaced=True) - frames, counts, verdict
and err_offset on every stream of tests/ilace_cases.py; known answers that need no decoder, as literal pictures; what the cases
reach, from the writer's log; the refusals; the invariant on the streams of main_cases and bpic_cases; the altered streams; and the
host build once under AddressSanitizer and UBSan as a stand-alone program.  tests/test_gpu_decode_ilace.py runs the same streams on
the device."""
import os
import subprocess

import numpy as np
import pytest

import bpic_cases as B
import dec_cases as D
import ilace_cases as I
import ilace_writer as IW
import main_cases as C

M = D.M


def check(stream, b_pictures, layouts=("i420",)):
    """the host build answers what the definition answers: frames and counts, or the refusal and its offset"""
    d, at = I.spec_cached(stream, b_pictures)
    for layout in layouts:
        f, r = I.host_decode(stream, b_pictures, layout)
        if d is None:
            assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0), (r, at)
        else:
            assert r["status"] == D.OK, r
            assert np.array_equal(f, D.frames_of(d, layout)) if d.frames else f.shape == (0, r["frame_bytes"]), layout
            want = I.record_of(d, stream)
            assert {k: r[k] for k in want} == want and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def same_frames(fa, fb):
    return len(fa) == len(fb) and all(np.array_equal(a, b) for x, y in zip(fa, fb) for a, b in zip(x, y))


# ---- the interface of the definition ----
def test_the_keyword():
    s = I.cases()["ip_32"][0]
    with pytest.raises(ValueError):
        M.decoder.decode(s, quirks=False, syntax="module", interlaced=True)
    with pytest.raises(ValueError):
        M.decoder.decode(s, interlaced=True)
    d = M.decoder.decode(s, quirks=False, syntax="main", interlaced=True)
    assert len(d.frames) == 3 and not hasattr(d, "display")
    assert {"motion_type", "dct_type", "selects", "vectors"} <= set(d.mbs[1][0])
    with pytest.raises(M.decoder.Refused):                          # without the option: the parent's answer, at the first coding extension
        M.decoder.decode(s, quirks=False, syntax="main")


def test_rows_rule_and_small_functions():
    """2 * ((height + 31) // 32) rows where the sequence is not progressive; tables B-2 / B-3 in Table B-4's form against the writer's;
    the field-DCT row map; the record's size"""
    L = I.host_lib()
    for h in range(1, 200):
        assert L.dec_i_host_rows(h, 1) == (h + 15) // 16 == IW.mb_rows(h, 1)
        assert L.dec_i_host_rows(h, 0) == 2 * ((h + 31) // 32) == IW.mb_rows(h, 0)
    assert (L.dec_i_host_rows(16, 0), L.dec_i_host_rows(40, 0), L.dec_i_host_rows(48, 0), L.dec_i_host_rows(576, 0)) == (2, 4, 4, 36)
    flags = dict(intra=0x01, coded=0x0A, nomc=0x02, not_coded=0x08)
    for ptype, table in ((1, IW.MW.TYPE_I), (2, IW.MW.TYPE_P)):
        for w in range(64):
            bits = format(w, "06b")
            want = [(len(c), flags[kind] | (0x10 if quant else 0)) for (kind, quant), c in table.items() if bits.startswith(c)]
            got = L.dec_i_host_type(w, ptype)
            assert (got & 255, got >> 8) == (want[0] if want else (0, 0)), (ptype, bits)
    for y in range(16):
        for x in range(16):
            assert L.dec_i_host_row_map(x, y, 0) == ((y >> 3) * 2 + (x >> 3)) << 8 | (y & 7)
            assert L.dec_i_host_row_map(x, y, 1) == ((y & 1) * 2 + (x >> 3)) << 8 | (y >> 1)
    assert L.dec_i_host_record_bytes() == 32


def test_no_field_vector_is_outside_through_chroma_alone():
    """the chroma block of a field prediction - 8 x 4 at (8 col, 4 row) of 8 mbw x 4 mbh with both components / 2 toward zero - lies
    inside whenever the luma block does: every place and vector of a 3 x 3 picture.  The refusal "outside through chroma alone"
    therefore has no stream; the rule is kept in il_field_inside and in the definition all the same"""
    L = I.host_lib()

    def ok(x0, y0, vx, vy, w, h, pw, ph):
        ix, iy, hx, hy = vx >> 1, vy >> 1, vx & 1, vy & 1
        return x0 + ix >= 0 and y0 + iy >= 0 and x0 + ix + w - 1 + hx < pw and y0 + iy + h - 1 + hy < ph
    inside = 0
    for col in range(3):
        for row in range(3):
            for vx in range(-70, 71):
                for vy in range(-40, 41):
                    luma = ok(16 * col, 8 * row, vx, vy, 16, 8, 48, 24)
                    chroma = ok(8 * col, 4 * row, int(vx / 2), int(vy / 2), 8, 4, 24, 12)
                    assert not luma or chroma, (col, row, vx, vy)
                    assert bool(L.dec_i_host_field_inside(col, row, vx, vy, 3, 3)) == (luma and chroma) == IW.field_inside(col, row, (vx, vy), 3, 3)
                    inside += luma
    assert inside > 10000


# ---- every case ----
@pytest.mark.parametrize("name", sorted(I.cases()))
def test_valid_cases(name):
    """every case in every 4:2:0 layout; the definition read what the writer wrote: every macroblock's place, motion type, DCT type,
    selects and vectors"""
    s, L = I.cases()[name]
    b = I.b_flag(name, L)
    d = check(s, b, D.LAYOUTS)
    assert d is not None and [p["type"] for p in d.pictures] == L["pictures"]
    assert d.units == D.prefixes(s) == len(L["units"]) and len(d.frames[0][0]) == d.height == d.sequence["height"]
    field_pics = [k for k, p in enumerate(d.pictures) if not p["frame_pred_frame_dct"]]
    read = [(k, m) for k in field_pics for m in d.mbs[k] if not m["skipped"]]
    assert len(read) == len(L["ilmbs"])
    for (k, m), w in zip(read, L["ilmbs"]):
        assert k == w["pic"] and m["intra"] == (w["kind"] == "intra") and m["cbp"] == w["cbp"]
        assert m["motion_type"] == (1 if w["motion"] == "field" else 2)
        assert m["dct_type"] == (w["dct"] or 0)
        for s_, v in enumerate((w["fwd"], w["bwd"])):
            if v is None:
                continue
            if w["motion"] == "field":
                assert m["selects"][s_] == (v[0][0], v[1][0]) and m["vectors"][s_] == (v[0][1], v[1][1]), (w, m)
            else:
                assert m["vectors"][s_] == (tuple(v), tuple(v)), (w, m)
        if w["quant"] is not None:
            assert m["qcode"] == w["quant"]
    if b and 3 in L["pictures"]:
        assert sorted(d.display) == list(range(len(d.frames)))


def test_sizes_of_the_cases():
    c = I.cases()
    assert len(c["wide"][1]["pictures"]) == 9 and [k for k, _ in c["wide"][1]["units"]].count("slice") == 72
    assert c["ipbb"][1]["pictures"] == [1, 2, 3, 3]
    d = I.spec_cached(c["ipb_16"][0], True)[0]
    assert (d.width, d.height) == (16, 16) and len(d.slice_qcodes[0]) == 2
    d = I.spec_cached(c["crop_40"][0], True)[0]
    assert d.height == 40 and len(d.slice_qcodes[0]) == 4           # three rows in a progressive sequence
    # the mixed stream holds pictures of both kinds
    d = I.spec_cached(c["mixed"][0], True)[0]
    assert [p["frame_pred_frame_dct"] for p in d.pictures] == [0, 1, 0, 0]


# ---- the known answers: literal pictures no decoder made ----
@pytest.mark.parametrize("name", sorted(I.known()))
def test_known_answers(name):
    s, L, want = I.known()[name]
    d = check(s, I.b_flag(name, L))
    assert d is not None and len(d.frames) == len(want)
    for k, (got, exp) in enumerate(zip(d.frames, want)):
        for plane, (g, e) in enumerate(zip(got, exp)):
            assert np.array_equal(g, e), (name, k, plane, g[:, 0].tolist(), e[:, 0].tolist())


def test_known_answers_say_what_they_claim():
    K = I.known()
    A, Bv = I.A_, I.B_
    # field DCT against frame DCT: the same bits but for one per macroblock
    a, b = K["field_dct_1"][0], K["field_dct_0"][0]
    assert len(a) == len(b) and sum(bin(x ^ y).count("1") for x, y in zip(a, b)) == 4
    assert K["field_dct_1"][2][0][0][:4, 0].tolist() == [A, Bv, A, Bv] and K["field_dct_0"][2][0][0][6:10, 0].tolist() == [A, A, Bv, Bv]
    # the selects: swapped, all A, all B
    assert K["selects_10"][2][1][0][:2, 0].tolist() == [Bv, A] and (K["selects_00"][2][1][0] == A).all() and (K["selects_11"][2][1][0] == Bv).all()
    # scale, doubling, halving: columns 1 and 2 are written with zero deltas
    L = K["vector_scale"][1]
    row0 = [v for v in L["vectors"]][:10]                           # (f_code, wrap, component, delta): column 0 two vectors (each from its own
    # predictor, zero at the slice's start), column 1 one, column 2 two
    assert [v[2:] for v in row0] == [(0, 0), (16, 16), (0, 0), (16, 16), (0, 0), (32, 0), (0, 0), (16, 0), (0, 0), (16, 0)]
    want = K["vector_scale"][2][1][0]
    assert all((want[16 * r:16 * r + 16] == I.ROWS[r + 1]).all() for r in range(2))
    # a frame vector of 16: eight lines
    want = K["frame_vector_16"][2][1][0]
    assert (want[:8] == I.ROWS[0]).all() and (want[8:16] == I.ROWS[1]).all()
    # the half sample inside one field; a frame half-sample would have mixed A and B
    assert (K["field_half_sample"][2][1][0][:16] == A).all() and (A + Bv + 1) >> 1 != A
    # chroma: 0 and -1, not -1 and -2
    assert (K["chroma_vector_1"][2][1][1][8:16] == I.CROWS[1]).all()
    c = K["chroma_vector_3"][2][1][1]
    assert c[8:10, 0].tolist() == [(I.CROWS[0] + I.CROWS[1] + 1) >> 1] * 2 and (c[10:16] == I.CROWS[1]).all()
    # the B picture's skipped macroblock: one in every row but the last, behind a field-based one
    L = K["b_skip"][1]
    assert [m["incr"] for m in L["ilmbs"] if m["type"] == 3 and m["row"] == 0] == [1, 2]
    assert [m["inherited"] for m in L["ilmbs"] if m["type"] == 3 and m["row"] == 0][1] == ((1, 0), (0, 32), (0, 0))
    # sixteen lines: two slices
    assert [k for k, _ in K["sixteen_lines"][1]["units"]].count("slice") == 2


# ---- what the cases reach (from the writer's log, not from a decoder) ----
def test_coverage():
    mbs = [m for _, L in I.cases().values() for m in L["ilmbs"]]
    p = {m["motion"] for m in mbs if m["type"] == 2 and m["motion"]}
    assert p == {"frame", "field"}
    b = {(m["motion"], m["fwd"] is not None, m["bwd"] is not None) for m in mbs if m["type"] == 3 and m["motion"]}
    assert b == {(t, f, k) for t in ("frame", "field") for f, k in ((True, False), (False, True), (True, True))}
    assert {m["dct"] for m in mbs if m["kind"] == "intra"} == {0, 1}
    assert {m["dct"] for m in mbs if m["kind"] != "intra" and m["cbp"]} == {0, 1}
    assert {m["dct"] for m in mbs if m["kind"] == "nomc"} == {0, 1}
    assert set().union(*(L["selects"] for _, L in I.cases().values())) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set().union(*(L["resets"] for _, L in I.cases().values())) == {"slice", "intra", "nomc", "p_skip"}
    # skipped macroblocks of both picture types, a B picture's behind a field-based macroblock
    assert {m["type"] for m in mbs if m["incr"] > 1} == {2, 3}
    assert any(m["inherited"] and m["inherited"][1] != (0, 0) for m in mbs if m["type"] == 3)
    # pictures that read, and do not act on, top_field_first, repeat_first_field, chroma_420_type
    assert len(I.cases()["mixed"][1]["pictures"]) == 4


# ---- refusals ----
@pytest.mark.parametrize("name", sorted(I.refusals()))
def test_refusals(name):
    s, b, want = I.refusals()[name]
    d, at = I.spec_cached(s, b)
    assert d is None and at == want, (at, want)
    check(s, b)


def test_refusals_have_accepted_twins():
    """what each refusal changes is what refuses it: the same pictures without the change decode"""
    rng = np.random.RandomState(61)
    base = I.pictures(rng, "IPB", 2, 2)
    still = I.fmb(0, (0, 0), 1, (0, 0))
    base[1]["slices"][0]["mbs"] = [dict(still), dict(still)]
    base[1]["slices"][1]["mbs"] = [dict(still), dict(still)]
    s, _ = IW.stream(32, 32, base)
    assert check(s, True) is not None
    # one half sample inside each edge
    for row, col, v in ((0, 1, (-1, 0)), (0, 0, (1, 0)), (1, 0, (0, -1)), (0, 0, (0, 1))):
        for r in (0, 1):
            p = [dict(q) for q in base]
            mbs = [dict(still), dict(still)]
            mbs[col] = I.fmb(0, v if r == 0 else (0, 0), 1, v if r == 1 else (0, 0))
            p[1] = dict(p[1], slices=[dict(sl) for sl in p[1]["slices"]])
            p[1]["slices"][row] = dict(q=3, mbs=mbs)
            assert check(IW.stream(32, 32, p)[0], True) is not None, (row, col, v, r)
    # a B picture is accepted with the option on; the rows of a progressive sequence accept one slice for sixteen lines
    s, b, _ = I.refusals()["b_picture_with_b_off"]
    assert check(s, True) is not None
    one = IW.stream(16, 16, I.pictures(np.random.RandomState(65), "IP", 1, 1), seq=dict(progressive=1))[0]
    assert I.spec(one, False)[1] is not None                        # (field pictures in a progressive sequence: refused at the extension)
    prog = [dict(C.intra_picture(np.random.RandomState(1), 1, 1))]
    s16 = IW.stream(16, 16, prog, seq=dict(progressive=1))[0]
    assert check(s16, False) is not None and I.spec(IW.stream(16, 16, prog, rows=1)[0], False)[0] is None


def test_option_off_is_the_parent():
    """interlaced=False: a stream with frame_pred_frame_dct 0 is refused at its first picture coding extension"""
    for name in ("ip_32", "ipb_48", "field_dct_1"):
        s, L = I.cases()[name]
        first = [a for k, a in L["units"] if k == "picture_ext"][0]
        assert I.spec(s, I.b_flag(name, L), interlaced=False) == (None, first)


# ---- the invariant ----
def test_streams_the_main_syntax_accepts_are_what_they_were():
    """every valid stream of main_cases (b_pictures off and on) and bpic_cases (on) with the option on equals the option off:
    frames, pictures, macroblocks, quantisers, counts.  (They are progressive sequences, or have an even number of macroblock rows:
    the stated exception does not arise.)  The refusals of both suites keep their offsets; frame_pred_frame_dct 0 stays refused
    there because those pictures say progressive_frame 1"""
    fields = lambda d: (d.pictures, d.mbs, d.slice_qcodes, d.gops, d.repeated_headers, d.units, d.sequence, getattr(d, "display", None))
    n = 0
    for suite, flags in ((C, (False, True)), (B, (True,))):
        for name, (s, _) in sorted(suite.cases().items()):
            for b in flags:
                off, on = I.spec(s, b, interlaced=False)[0], check(s, b)
                assert off is not None and on is not None and same_frames(off.frames, on.frames) and fields(off) == fields(on), name
                assert off.sequence["progressive_sequence"] == 1 or ((off.height + 15) // 16) % 2 == 0
                n += 1
    assert n >= 40
    for name, (s, want) in sorted(C.refusals().items()):
        assert I.spec_cached(s, False) == (None, want), name
        check(s, False)
    for name, (s, want) in sorted(B.refusals().items()):
        assert I.spec_cached(s, True) == (None, want), name
        check(s, True)


def test_the_stated_exception():
    """progressive_sequence 0 with an odd (height + 15) // 16: three slices a picture without the option, four with it"""
    pics = [C.intra_picture(np.random.RandomState(2), 3, 3)]
    s3 = IW.stream(40, 40, pics, rows=3)[0]
    assert I.spec(s3, False, interlaced=False)[0] is not None and I.spec(s3, False)[0] is None
    check(s3, False)


# ---- altered streams ----
def test_altered_streams():
    cases = I.altered()
    assert check(I.altered_base()[0], True) is not None
    assert len(cases) == 300
    accepted = sum(I.spec_cached(x, True)[0] is not None for _, x in cases)
    refused = len(cases) - accepted
    print("%d altered streams: %d refused, %d accepted by the definition" % (len(cases), refused, accepted))
    assert accepted >= 30 and refused >= 100
    for name, x in cases:
        check(x, True)


def test_edges():
    s = I.cases()["ipbb"][0]
    fb = 48 * 48 * 3 // 2
    f, r = I.host_decode(s, True, cap=4 * fb - 1)
    assert f is None and r["status"] == D.OVERFLOW and r["out_bytes"] == 0
    assert I.host_decode(s, True, cap=4 * fb)[1]["status"] == D.OK
    for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64)):
        check(x, True)
        check(x, False)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(s, b) for _, s, b in I.all_streams()] + [(s, False) for s, _ in C.cases().values()] + [(s, True) for s, _ in B.cases().values()]
    path = tmp_path / "streams.bin"
    path.write_bytes(I.pack_streams(items))
    exe = str(tmp_path / "dec_i_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_i_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    for k in (0, 5, len(I.cases()), len(I.cases()) + 3, 100, 300, len(items) - 1):
        want = I.host_decode(items[k][0], items[k][1], D.LAYOUTS[k & 3])[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
