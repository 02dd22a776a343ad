"""The main syntax of the device decoder on the CPU: the main_ functions of csrc/m2v_decode_kernels.hpp and the serial harness
tools/dec_main_host.hpp, compiled with g++, against decoder.decode(..., syntax="main") - frames, counts, verdict and err_offset on
every stream of tests/main_cases.py; the invariant that ties the two syntaxes together; known answers that need no decoder at all;
what the cases reach, from the writer's log; the refusals and about a thousand altered streams; the tables typed twice; and the host
build once under AddressSanitizer and UBSan as a stand-alone program.  tests/test_gpu_decode_main.py runs the same streams on the device."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dec_cases as D
import dec_writer as W
import main_cases as C
import main_writer as MW

M = D.M


def check(stream, layouts=("i420",)):
    """the host build answers what the definition answers: frames and counts, or the refusal and its offset"""
    d, at = C.spec_cached(stream)
    for layout in layouts:
        f, r = C.host_decode(stream, layout)
        if d is None:
            assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0), (r, at)
        else:
            assert r["status"] == D.OK, r
            assert np.array_equal(f, D.frames_of(d, layout)) if d.frames else f.shape == (0, r["frame_bytes"]), layout
            want = C.record_of(d, stream)
            assert {k: r[k] for k in want} == want and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_valid_cases(name):
    s, L = C.cases()[name]
    d = check(s, D.LAYOUTS)
    assert d is not None and [p["type"] for p in d.pictures] == L["pictures"]
    assert d.units == D.prefixes(s) == len(L["units"])
    # the definition read what the writer wrote: every macroblock's place and kind, skipped ones in between
    coded = [m for mbs in d.mbs for m in mbs if not m["skipped"]]
    assert len(coded) == len(L["mbs"])
    for m, w in zip(coded, L["mbs"]):
        assert m["intra"] == (w["kind"] == "intra") and m["mc"] == (w["kind"] in ("coded", "not_coded")) and m["mv"] == w["mv"] and m["cbp"] == w["cbp"]
    assert sum(m["skipped"] for mbs in d.mbs for m in mbs) == sum(i - 1 for i in L["incrs"])


# ---- the invariant: what M2V_DEC_ISO accepts in the module syntax decodes to the same frames and counts in the main syntax ----
def _superset(stream):
    d, _ = D.spec(stream, False)
    if d is None:
        return False
    m = check(stream)
    assert m is not None, "accepted by the module syntax, refused by the main syntax"
    assert all(np.array_equal(a, b) for fa, fb in zip(d.frames, m.frames) for a, b in zip(fa, fb)) and len(d.frames) == len(m.frames)
    assert (len(d.pictures), len(d.gops), d.repeated_headers, d.width, d.height) == (len(m.pictures), len(m.gops), m.repeated_headers, m.width, m.height)
    assert d.slice_qcodes == m.slice_qcodes
    return True


def test_superset_invariant_written_streams():
    streams = [D.small(), D.described(), W.qcodes()[0], W.dc_range()[0], W.escapes()[0], W.saturate()[0], W.pmv_chain()[0]]
    streams += [W.sized(w, h)[0] for w, h in W.SMALL_SIZES] + [s for s, _ in W.stuffed()]
    assert all(_superset(s) for s in streams)


def test_superset_invariant_encoded_streams():
    streams = list(D.tile_streams(conformant=True)[:2]) + [D.ionly_stream(), D.twin_streams()["unref"], D.recon_streams()["conformant"]["stream"]]
    assert all(_superset(s) for s in streams)


def test_superset_invariant_altered_streams():
    """the altered streams of tests/test_dec_cases.py: each one the module syntax accepts is accepted here with the same frames (the
    others may go either way: the main syntax is wider)"""
    s = D.small()
    cases = [x for _, x in D.altered()] + [D.flip(s, b) for b in range(8 * D.first_slice(s))] + list(D.handmade().values()) + list(W.refusals().values())
    accepted = sum(_superset(x) for x in cases)
    wider = sum(C.spec_cached(x)[0] is not None for x in cases) - accepted
    print("%d altered streams: %d accepted by both, %d by the main syntax only" % (len(cases), accepted, wider))
    assert accepted >= 100 and wider >= 1


# ---- known answers ----
@pytest.mark.parametrize("prec", (0, 1, 2, 3))
def test_flat_intra_picture(prec):
    for value in (16, 128, 131, 235):
        s = C.flat_intra(value, prec)
        d = check(s)
        assert d.pictures[0]["intra_dc_precision"] == prec
        assert all((p == value).all() for p in d.frames[0]), (prec, value)


def test_still_p_pictures_repeat_the_picture_before():
    rng = np.random.RandomState(4)
    s, L = MW.stream(48, 32, [C.intra_picture(rng, 3, 2), C.still_p(3, 2, "skipped"), C.still_p(3, 2, "not_coded"), C.still_p(3, 2, "skipped", f_code=(5, 7))])
    assert L["incrs"].count(2) == 4 and 2 in L["pictures"]
    d = check(s)
    for k in (1, 2, 3):
        assert all(np.array_equal(a, b) for a, b in zip(d.frames[0], d.frames[k]))


@pytest.mark.parametrize("f,dx,dy", ((2, 12, 0), (4, 40, 0), (2, -13, 10), (4, 0, -33)))
def test_whole_pel_vectors_beyond_8_pel(f, dx, dy):
    """160 x 96: every macroblock the shift leaves inside the picture carries the vector (2 dx, 2 dy), the others the zero vector; the
    P picture's macroblocks are the I picture's, moved"""
    rng = np.random.RandomState(8)
    inside = lambda col, row: W.inside(col, row, (2 * dx, 2 * dy), 10, 6)
    p = dict(type=2, f_code=(f, f), slices=[dict(q=2, mbs=[dict(kind="not_coded", mv=(2 * dx, 2 * dy) if inside(col, row) else (0, 0)) for col in range(10)])
                                           for row in range(6)])
    s, L = MW.stream(160, 96, [C.intra_picture(rng, 10, 6), p])
    moved = [(m["col"], m["row"]) for m in L["mbs"] if m["pic"] == 1 and m["mv"] != (0, 0)]
    assert len(moved) >= 12 and max(abs(dx), abs(dy)) > 8
    d = check(s)
    (y0, u0, v0), (y1, u1, v1) = d.frames
    for col, row in moved:
        assert np.array_equal(y1[16 * row:16 * row + 16, 16 * col:16 * col + 16], y0[16 * row + dy:16 * row + dy + 16, 16 * col + dx:16 * col + dx + 16])
        if dx % 2 == 0 and dy % 2 == 0:
            for a, b in ((u0, u1), (v0, v1)):
                assert np.array_equal(b[8 * row:8 * row + 8, 8 * col:8 * col + 8], a[8 * row + dy // 2:8 * row + dy // 2 + 8, 8 * col + dx // 2:8 * col + dx // 2 + 8])


def _pair(seed, a, b, seq_a=None, seq_b=None):
    """the same pictures written twice with different parameters -> the two decoded"""
    out = []
    for params, seq in ((a, seq_a), (b, seq_b)):
        rng = np.random.RandomState(seed)
        pics = [C.intra_picture(rng, 3, 2, **params), C.random_p(rng, 3, 2, **params)]
        for p in pics:                                              # (no macroblock quantisers: the slice's code is the parameter)
            for sl in p["slices"]:
                for m in sl["mbs"]:
                    m.pop("quant", None)
        out.append(check(MW.stream(48, 32, pics, seq=seq)[0]))
    return out


def test_nonlinear_code_9_is_linear_code_5():
    a, b = _pair(12, dict(qst=1, q=9), dict(qst=0, q=5))
    assert MW.scale(9, 1) == MW.scale(5, 0) == 10
    assert all(np.array_equal(x, y) for fa, fb in zip(a.frames, b.frames) for x, y in zip(fa, fb))
    c, _ = _pair(12, dict(qst=1, q=10), dict(qst=0, q=5))
    assert not all(np.array_equal(x, y) for fa, fb in zip(c.frames, b.frames) for x, y in zip(fa, fb))


def test_double_weight_is_double_scale():
    """weight 2w with scale s against weight w with scale 2s: 2 w s = w 2 s in every product of 7.4.2"""
    double = lambda m: [2 * v for v in m]
    a, b = _pair(13, dict(q=3), dict(q=6), dict(intra_matrix=double(C.MATRIX_A), non_intra_matrix=double(C.MATRIX_B)),
                 dict(intra_matrix=C.MATRIX_A, non_intra_matrix=C.MATRIX_B))
    assert all(np.array_equal(x, y) for fa, fb in zip(a.frames, b.frames) for x, y in zip(fa, fb))
    c, _ = _pair(13, dict(q=3), dict(q=3), dict(intra_matrix=C.MATRIX_A, non_intra_matrix=C.MATRIX_B))
    assert not all(np.array_equal(x, y) for fa, fb in zip(c.frames, b.frames) for x, y in zip(fa, fb))


@pytest.mark.parametrize("raster", (1, 8, 9, 24, 35, 56, 62, 63))
def test_alternate_scan_places_the_same_coefficient(raster):
    def one(alt):
        k = MW.scan_position(raster, alt)
        blk = dict(dc=5, coefs=[(k - 1, 37, False)])
        pic = dict(type=1, alt=alt, slices=[dict(q=4, mbs=[dict(kind="intra", blocks=[blk] * 6) for _ in range(3)]) for _ in range(2)])
        return check(MW.stream(48, 32, [pic])[0])
    a, b = one(1), one(0)
    assert MW.scan_position(raster, 1) != MW.scan_position(raster, 0) or raster in (63,)
    assert all(np.array_equal(x, y) for x, y in zip(a.frames[0], b.frames[0])) and len(set(a.frames[0][0].reshape(-1).tolist())) > 1


def test_table_b1():
    """prefix-free, and the sum of 2 ^ -length: one code of 1 bit, two of 3, 4, 5 and 7 bits, six of 8 and 10, twelve of 11, and the
    escape's 11 - 2025 / 2048 (the stuffing code of ISO/IEC 11172-2 and the unused codes are the rest)"""
    codes = list(MW.B1) + [MW.B1_ESCAPE]
    assert len(set(codes)) == 34
    assert not any(a != b and b.startswith(a) for a in codes for b in codes)
    assert sum(Fraction(1, 2 ** len(c)) for c in codes) == Fraction(1, 2) + 2 * Fraction(1, 8) + 2 * Fraction(1, 16) + 2 * Fraction(1, 32) + 2 * Fraction(1, 128) \
        + 6 * Fraction(1, 256) + 6 * Fraction(1, 1024) + 13 * Fraction(1, 2048) == Fraction(2025, 2048)


def test_tables_typed_twice_agree():
    """main_writer's Table B-1, table 7-6 and figure 7-3 against decoder.py's and the kernels header's"""
    t = M.decoder.main_tables()
    L = C.host_lib()
    assert [(int(b, 2), len(b), k + 1) for k, b in enumerate(MW.B1)] == t["increment"] and MW.B1_ESCAPE == t["escape"]
    assert [0] + list(MW.NONLINEAR) == t["nonlinear"] and [v for row in MW.ALTERNATE for v in row] == t["alternate"]
    by_code = {b: k + 1 for k, b in enumerate(MW.B1)}
    by_code[MW.B1_ESCAPE] = 34
    for w in range(1 << 11):                                        # every window of 11 bits
        bits = format(w, "011b")
        want = [(len(b), v) for b, v in by_code.items() if bits.startswith(b)]
        got = L.dec_main_host_increment(w)
        assert (got & 255, got >> 8) == (want[0] if want else (0, 0)), bits
    for code in range(32):
        assert L.dec_main_host_scale(code, 1) == MW.scale(code, 1) and L.dec_main_host_scale(code, 0) == 2 * code
    for r in range(64):
        assert L.dec_main_host_scan(1, MW.scan_position(r, 1)) == r == L.dec_main_host_scan(0, MW.scan_position(r, 0))
        assert L.dec_main_host_zigzag_position(r) == MW.scan_position(r, 0)
    assert {"".join(k): v for k, v in ((b, f) for b, f in t["type_p"].items())} == {b: (int(q), int(k in ("coded", "not_coded")), int(k in ("coded", "nomc")), int(k == "intra"))
                                                                                   for (k, q), b in MW.TYPE_P.items()}


def test_vector_reconstruction_every_f_code():
    """7.6.3.1 for every f_code: each prediction at the range's ends and around zero, every motion code, residuals at both ends"""
    L = C.host_lib()
    for f_code in range(1, 10):
        r_size = f_code - 1
        f = 1 << r_size
        wrapped = set()
        for pmv in sorted({-16 * f, -16 * f + 1, -f, -1, 0, 1, f, 16 * f - 2, 16 * f - 1}):
            for code in range(-16, 17):
                for residual in sorted({0, f // 2, f - 1}) if code and f > 1 else (0,):
                    delta = code if f == 1 or code == 0 else (((abs(code) - 1) * f) + residual + 1) * (1 if code > 0 else -1)
                    v = pmv + delta
                    if v < -16 * f:
                        v, _ = v + 32 * f, wrapped.add(1)
                    elif v > 16 * f - 1:
                        v, _ = v - 32 * f, wrapped.add(-1)
                    assert L.dec_main_host_vector(pmv, code, residual, r_size) == v, (f_code, pmv, code, residual)
        assert wrapped == {1, -1}


# ---- what the cases reach (from the writer's log, not from a decoder) ----
def test_coverage():
    logs = {name: L for name, (_, L) in C.cases().items()}
    types = set().union(*[L["types"] for L in logs.values()])
    assert types >= {(1, "intra", False), (1, "intra", True)} | {(2, k, q) for (k, q) in MW.TYPE_P}
    assert set(logs["escapes"]["incrs"]) >= {1, 2, 33, 34, 67}
    vectors = logs["fcodes"]["vectors"] + logs["fcodes_wide"]["vectors"]
    assert {f for f, _, _, _ in logs["fcodes"]["vectors"]} == set(range(1, 10)) and {f for f, _, _, _ in logs["fcodes_wide"]["vectors"]} == {1, 6, 7, 8, 9}
    for f in range(1, 10):
        F = 1 << (f - 1)
        assert max(abs(d) for ff, _, _, d in vectors if ff == f) > (8 * F - 1 if f > 1 else 4)          # a delta beyond the range of the f_code below
        if f >= 2:
            assert any(abs(d) > 1 and (abs(d) - 1) % F for ff, _, _, d in vectors if ff == f)          # a residual that is not zero
    # a wrap in each direction for every f_code up to 8: 1 .. 5 at 160 x 96, 6 .. 8 at 1088 x 16.  f_code 9's range is +-2048 pel, and
    # a wrap needs consecutive vectors more than half the range's width, 2048 pel, apart: no picture within the size limit of 2048
    # holds two such vectors (test_vector_reconstruction_every_f_code holds the function to 7.6.3.1 for all nine)
    assert {(f, w) for f, w, _, _ in vectors if w} == {(f, w) for f in range(1, 9) for w in (1, -1)}
    assert {(f, w) for f, w, _, _ in logs["fcodes_wide"]["vectors"] if w and f > 1} == {(f, w) for f in (6, 7, 8) for w in (1, -1)}
    params = [p for L in logs.values() for p in L["params"]]
    assert {p[1] for p in params} == {0, 1, 2, 3} and {p[2] for p in params} == {0, 1} and {p[3] for p in params} == {0, 1}
    quants = set(logs["scales"]["quants"]) | {(q, p[2]) for p, qs in zip(logs["scales"]["params"], logs["scales"]["qcodes"]) for q in qs}
    assert quants >= {(c, t) for c in (1, 8, 9, 31) for t in (0, 1)}
    kinds = lambda name: [k for k, _ in logs[name]["units"]]
    assert "display_ext" not in kinds("no_display") and "gop" not in kinds("no_gop") and "end" not in kinds("no_end")
    assert not {"display_ext", "gop", "end"} & set(kinds("bare"))
    # every transparent unit in every place: (the unit in front that is not transparent, the transparent unit)
    t = kinds("transparent")
    places, prev = set(), None
    for k in t:
        if k in ("user", "copyright", "picture_display"):
            places.add((prev, k))
        else:
            prev = k
    assert places == {("sequence_ext", "user"), ("display_ext", "user"), ("gop", "user"), ("picture_ext", "user"), ("picture_ext", "copyright"),
                      ("picture_ext", "picture_display")}
    assert ("sequence_ext", "user") in {(a, b) for a, b in zip(kinds("transparent_no_display"), kinds("transparent_no_display")[1:])}
    p = logs["changing"]["params"]
    assert all(a != b for a, b in zip(p, p[1:])) and len({x[0] for x in p}) >= 6
    r = kinds("repeats")
    assert r.count("sequence") == 3 and ("display_ext", "gop") in set(zip(r, r[1:])) and ("display_ext", "picture") in set(zip(r, r[1:]))
    seqs = {name: C.spec_cached(s)[0].sequence for name, (s, _) in C.cases().items() if name.startswith("matrix")}
    default_i, default_n = M.decoder.iso_tables()["intra_w"], [16] * 64
    assert seqs["matrix_intra"]["intra_matrix"] == C.MATRIX_A and seqs["matrix_intra"]["non_intra_matrix"] == default_n
    assert seqs["matrix_non_intra"]["intra_matrix"] == default_i and seqs["matrix_non_intra"]["non_intra_matrix"] == C.MATRIX_B
    assert seqs["matrix_both"]["intra_matrix"] == C.MATRIX_A and seqs["matrix_both"]["non_intra_matrix"] == C.MATRIX_B


# ---- refusals ----
@pytest.mark.parametrize("name", sorted(C.refusals()))
def test_refusals(name):
    """one stream per line of the header's "still M2V_DEC_SYNTAX" list: refused by the definition at the unit the writer put the fault
    into, and by the host build at the same offset"""
    s, want = C.refusals()[name]
    d, at = C.spec_cached(s)
    assert d is None and at == want, (at, want)
    check(s)


def test_altered_streams():
    cases = C.altered()
    assert len(cases) >= 1000
    base = C.altered_base()[0]
    assert check(base) is not None
    refused = accepted = 0
    for name, x in cases:
        d = check(x)
        refused, accepted = refused + (d is None), accepted + (d is not None)
    print("%d altered streams: %d refused, %d accepted" % (len(cases), refused, accepted))
    assert refused >= 0.3 * len(cases) and accepted >= 0.1 * len(cases)


def test_edges():
    for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64), b"\x00\x00\x01\xb5"):
        check(x)
    # sequence headers and no picture: accepted, no frames (a decision on record: the module syntax accepts its header group with an
    # end code behind it too); with and without sequence_end_code, with user_data behind the headers
    t, L = C.cases()["transparent"]
    cut = [a for k, a in L["units"] if k == "gop"][0]
    for x in (t[:cut], t[:cut] + b"\x00\x00\x01\xb7", t[:cut] + bytes(9)):
        d = check(x, D.LAYOUTS)
        assert d is not None and d.frames == [] and d.pictures == [] and (d.width, d.height) == (48, 32)
        f, r = C.host_decode(x)
        assert f.shape == (0, 2304) and (r["status"], r["pictures"], r["out_bytes"], r["frame_bytes"]) == (D.OK, 0, 0, 2304)
    s = C.cases()["types"][0]
    f, r = C.host_decode(s, cap=3 * 2304 - 1)
    assert f is None and r["status"] == D.OVERFLOW and r["out_bytes"] == 0
    assert C.host_decode(s, cap=3 * 2304)[1]["status"] == D.OK


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(s, "iso") for s, _ in C.cases().values()] + [(s, "iso") for s, _ in C.refusals().values()] + [(x, "iso") for _, x in C.altered()]
    items += [(x, "iso") for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64), D.small(), W.escapes()[0], W.saturate()[0])]
    path = tmp_path / "streams.bin"
    path.write_bytes(D.pack_streams(items))
    exe = str(tmp_path / "dec_main_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_main_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    for k in (0, 5, len(C.cases()), len(C.cases()) + 3, 400, 900, len(items) - 1):
        want = C.host_decode(items[k][0], D.LAYOUTS[k & 3])[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
