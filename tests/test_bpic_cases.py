"""B pictures (option "decode_b_pictures") on the CPU: the bp_ functions of csrc/m2v_decode_kernels.hpp and the serial harness
tools/dec_b_host.hpp, compiled with g++, against decoder.decode(..., syntax="main", b_pictures=True) - frames in display order, counts,
verdict and err_offset on every stream of tests/bpic_cases.py; Table B-4 typed three times; known answers that need no decoder; what
the cases reach, from the writer's log; the coded orders; the refusals; the altered streams; and the host build once under
AddressSanitizer and UBSan as a stand-alone program.  tests/test_gpu_decode_bpic.py runs the same streams on the device."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bpic_cases as B
import bpic_writer as BW
import dec_cases as D
import main_cases as C

M = D.M


def check(stream, layouts=("i420",)):
    """the host build answers what the definition answers: frames and counts, or the refusal and its offset"""
    d, at = B.spec_cached(stream)
    for layout in layouts:
        f, r = B.host_decode(stream, layout)
        if d is None:
            assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0), (r, at)
        else:
            assert r["status"] == D.OK, r
            assert np.array_equal(f, D.frames_of(d, layout)) if d.frames else f.shape == (0, r["frame_bytes"]), layout
            want = B.record_of(d, stream)
            assert {k: r[k] for k in want} == want and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def same_frames(fa, fb):
    return all(np.array_equal(a, b) for a, b in zip(fa, fb))


def closed_form(types):
    """the display index of every coded picture: p - 1 for a B picture, (coded index of the next anchor) - 1 for an anchor, N - 1 for the last"""
    anchors = [p for p, t in enumerate(types) if t != 3]
    return [p - 1 if t == 3 else ([a for a in anchors if a > p] + [len(types)])[0] - 1 for p, t in enumerate(types)]


# ---- the interface of the definition ----
def test_the_keyword():
    s = B.cases()["types"][0]
    with pytest.raises(ValueError):
        M.decoder.decode(s, quirks=False, syntax="module", b_pictures=True)
    with pytest.raises(ValueError):
        M.decoder.decode(s, b_pictures=True)
    d = M.decoder.decode(s, quirks=False, syntax="main", b_pictures=True)
    assert d.display == [0, 3, 1, 2] and len(d.frames) == 4
    assert not hasattr(M.decoder.decode(C.cases()["types"][0], quirks=False, syntax="main"), "display")


@pytest.mark.parametrize("name", sorted(B.cases()))
def test_valid_cases(name):
    """every case in every 4:2:0 layout; the definition read what the writer wrote: every B macroblock's place, directions, vectors,
    pattern and quantiser, the skipped ones in between with what they inherit"""
    s, L = B.cases()[name]
    d = check(s, D.LAYOUTS)
    assert d is not None and [p["type"] for p in d.pictures] == L["pictures"] and 3 in L["pictures"]
    assert d.units == D.prefixes(s) == len(L["units"])
    assert d.display == closed_form(L["pictures"]) and sorted(d.display) == list(range(len(d.frames)))
    bpics = [k for k, t in enumerate(L["pictures"]) if t == 3]
    read = [(k, m) for k in bpics for m in d.mbs[k]]
    coded = [(k, m) for k, m in read if not m["skipped"]]
    assert len(coded) == len(L["bmbs"])
    at = 0
    for w in L["bmbs"]:
        for j in range(w["incr"] - 1):                              # the skipped ones in front of it
            k, m = read[at]
            front, pf, pb = w["inherited"]
            assert m["skipped"] and (m["fwd"], m["bwd"]) == (bool(front[0]), bool(front[1])) and m["cbp"] == 0
            assert m["mv"] == (pf if front[0] else (0, 0)) and m["mv_b"] == (pb if front[1] else (0, 0))
            at += 1
        k, m = read[at]
        at += 1
        assert k == w["pic"] and not m["skipped"] and m["intra"] == w["intra"] and m["cbp"] == w["cbp"]
        assert (m["fwd"], m["bwd"]) == (w["fwd"] is not None, w["bwd"] is not None)
        assert m["mv"] == (w["fwd"] or (0, 0)) and m["mv_b"] == (w["bwd"] or (0, 0))
        if w["quant"] is not None:
            assert m["qcode"] == w["quant"]
    assert at == len(read)


def test_one_size_above_the_small_ones():
    s, L = B.wide()
    assert L["pictures"].count(3) == 16 and max(L["incrs"]) == 2
    assert check(s) is not None


# ---- Table B-4 ----
def test_table_b4():
    """eleven codes: two each of 2, 3, 4 and 5 bits, three of 6; prefix-free; Kraft sum 63 / 64 ('000000' is no code)"""
    codes = list(BW.TYPE_B.values()) + list(BW.TYPE_B_INTRA.values())
    assert len(set(codes)) == 11 and sorted(len(c) for c in codes) == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6]
    assert not any(a != b and b.startswith(a) for a in codes for b in codes)
    assert sum(Fraction(1, 2 ** len(c)) for c in codes) == Fraction(63, 64) and "000000" not in codes


def test_table_b4_typed_three_times():
    """bpic_writer's Table B-4 against decoder.py's and the kernels header's, every window of 6 bits through the host function"""
    t = M.decoder.main_tables()["type_b"]
    mine = {code: (q, f, b, p, 0) for (f, b, p, q), code in BW.TYPE_B.items()}
    mine.update({code: (q, 0, 0, 0, 1) for q, code in BW.TYPE_B_INTRA.items()})
    assert mine == t
    L = B.host_lib()
    for w in range(64):
        bits = format(w, "06b")
        want = [(len(c), v) for c, v in mine.items() if bits.startswith(c)]
        got = L.dec_b_host_type(w)
        if not want:
            assert got == 0 and bits == "000000"
            continue
        q, f, b, p, i = want[0][1]
        assert (got & 255, got >> 8) == (want[0][0], q << 4 | f << 3 | b << 2 | p << 1 | i), bits


# ---- what the cases reach (from the writer's log, not from a decoder) ----
def test_coverage():
    logs = {name: L for name, (_, L) in B.cases().items()}
    lines = set(BW.TYPE_B) | {("intra", 0), ("intra", 1)}
    assert logs["types"]["btypes"] == lines                          # every line of Table B-4, the three quantiser lines among them
    assert {q for m in logs["types"]["bmbs"] if (q := m["quant"]) is not None} >= {2, 9, 31, 5}
    # skipped behind forward-only, backward-only and bidirectional macroblocks, with vectors that are not zero
    inherited = {m["inherited"][0] for m in logs["skips"]["bmbs"] if m["inherited"]}
    assert inherited == {(1, 0), (0, 1), (1, 1)}
    assert all(any(v != (0, 0) for v, used in zip(m["inherited"][1:], m["inherited"][0]) if used) for m in logs["skips"]["bmbs"] if m["inherited"])
    # an intra macroblock between two predicted ones: the vectors behind it start from zero, and would differ otherwise
    row = [m for m in logs["predictors"]["bmbs"] if m["row"] == 0]
    assert [m["intra"] for m in row] == [False, True, False] and row[0]["fwd"] != (0, 0) and row[0]["bwd"] != (0, 0)
    behind = [v for v in logs["predictors"]["bvectors"]][4:8]        # (direction, f_code, wrap, component, delta, predictor before)
    assert all(v[5] == 0 and v[4] == v[3] for v in behind) and [v[3] for v in behind] == [-2, 2, -4, 2]
    assert [v[3] - p for v, p in zip(behind, row[0]["fwd"] + row[0]["bwd"])] != [v[4] for v in behind]
    # the unused direction's predictor survives: the backward delta of the third macroblock of row 1 counts from the first's vector
    row = [m for m in logs["predictors"]["bmbs"] if m["row"] == 1]
    assert [(m["fwd"] is not None, m["bwd"] is not None) for m in row] == [(True, True), (True, False), (False, True)]
    last = logs["predictors"]["bvectors"][-2:]
    assert [v[0] for v in last] == [1, 1] and (last[0][5], last[1][5]) == row[0]["bwd"] != (0, 0)
    assert (last[0][4], last[1][4]) == (row[2]["bwd"][0] - row[0]["bwd"][0], row[2]["bwd"][1] - row[0]["bwd"][1])
    # half-pel: the four combinations forward, backward and in both; f_codes that differ between the directions
    cells = {(m["fwd"] is not None, m["bwd"] is not None, (m["fwd"] or m["bwd"])[0] & 1, (m["fwd"] or m["bwd"])[1] & 1) for m in logs["half_pel"]["bmbs"]}
    assert cells == {(f, b, hx, hy) for f, b in ((True, False), (False, True), (True, True)) for hx in (0, 1) for hy in (0, 1)}
    assert all(m["fwd"] != m["bwd"] for m in logs["half_pel"]["bmbs"] if m["fwd"] and m["bwd"] and m["fwd"] != (0, 0))
    assert all(p[0][:2] != p[0][2:] for p in logs["half_pel"]["params"] if len(p[0]) == 4)
    # a wrap in each direction of each predictor for f_codes 1 .. 4
    assert {(d, f, w) for d, f, w, _, _, _ in logs["wraps"]["bvectors"] if w} == {(d, f, w) for d in (0, 1) for f in (1, 2, 3, 4) for w in (1, -1)}
    # the coded orders, and GOP headers only where an open-GOP one is written
    for letters in B.ORDERS:
        L = logs["order_" + letters]
        assert "".join(" IPB"[t] for t in L["pictures"]) == letters
        assert [k for k, _ in L["units"]].count("gop") == 1 + letters[1:].count("I")
    assert set(logs["params"]["params"][2:]) == {((2, 1, 1, 3), 3, 1, 1), ((3, 3, 2, 2), 2, 0, 0)}


# ---- known answers ----
def test_still_b_pictures_between_flat_anchors():
    """anchors of 100 and 103: forward only 100, backward only 103, both (100 + 103 + 1) >> 1 = 102; a row of skipped macroblocks
    repeats the macroblock in front"""
    for name, value in (("still_forward", 100), ("still_backward", 103), ("still_both", 102), ("still_skipped", 102)):
        s, L = B.cases()[name]
        d = check(s)
        assert d.display == [0, 2, 1]
        assert all((p == 100).all() for p in d.frames[0]) and all((p == 103).all() for p in d.frames[2])
        assert all((p == value).all() for p in d.frames[1]), name
    assert B.cases()["still_skipped"][1]["incrs"].count(2) == 2


def test_half_pel_against_numpy():
    """the B pictures of the half-pel case from the decoded anchors alone: each prediction rounded on its own, then the mean; the
    macroblocks without residual.  The anchors' interpolated sums are odd somewhere in every block, so both roundings show"""
    s, L = B.cases()["half_pel"]
    d = check(s)
    fwd, bwd = d.frames[d.display[0]][0].astype(np.int64), d.frames[d.display[1]][0].astype(np.int64)

    def block(ref, col, row, mv):
        ix, iy, hx, hy = mv[0] >> 1, mv[1] >> 1, mv[0] & 1, mv[1] & 1
        y0, x0 = 16 * row + iy, 16 * col + ix
        p = ref[y0:y0 + 17, x0:x0 + 17]
        a, b, c, e = p[:16, :16], p[:16, 1:17], p[1:17, :16], p[1:17, 1:17]
        sums = (a + b + c + e) if hx and hy else (a + b) if hx else (a + c) if hy else None
        odd = sums is not None and bool((sums & (3 if hx and hy else 1)).any())
        return ((a + b + c + e + 2) >> 2 if hx and hy else (a + b + 1) >> 1 if hx else (a + c + 1) >> 1 if hy else a), odd
    seen_odd = checked = 0
    for m in L["bmbs"]:
        if m["cbp"]:
            continue
        parts = [block(ref, m["col"], m["row"], mv) for ref, mv in ((fwd, m["fwd"]), (bwd, m["bwd"])) if mv is not None]
        want = parts[0][0] if len(parts) == 1 else (parts[0][0] + parts[1][0] + 1) >> 1
        got = d.frames[d.display[m["pic"]]][0][16 * m["row"]:16 * m["row"] + 16, 16 * m["col"]:16 * m["col"] + 16]
        assert np.array_equal(got, want), m
        seen_odd += any(o for _, o in parts)
        checked += 1
    assert checked == 8 and seen_odd >= 5


# ---- order ----
@pytest.mark.parametrize("letters", B.ORDERS)
def test_order(letters):
    """every picture of the stream against the same picture decoded alone behind the anchors in front of it (coded order): its frame
    lies at the closed form's display index"""
    s, L = B.cases()["order_" + letters]
    d = check(s)
    types = L["pictures"]
    assert d.display == closed_form(types) == M.decoder.display_order(types)
    rng = np.random.RandomState(11)
    pics = B.order_pictures(rng, letters)
    full = B.spec(BW.stream(48, 32, pics)[0])[0]
    for p, t in enumerate(types):
        alone = [q for k, q in enumerate(pics[:p]) if types[k] != 3] + [pics[p]]
        one = B.spec(BW.stream(48, 32, [dict(q, gop=(k == 0), seq=(k == 0)) for k, q in enumerate(alone)])[0])[0]
        assert same_frames(one.frames[one.display[-1]], full.frames[full.display[p]]), (letters, p)
    assert len(set(f[0].tobytes() for f in full.frames)) == len(types)


def test_streams_without_b_pictures_are_what_they_were():
    """the superset: every stream of main_cases.cases() with the option on equals the option off - frames, pictures, macroblocks,
    quantisers, counts -, display = coded; and every refusal of the main syntax but the B picture's keeps its offset"""
    for name, (s, _) in sorted(C.cases().items()):
        off, on = C.spec_cached(s)[0], check(s)
        assert on.display == list(range(len(on.frames))) and len(on.frames) == len(off.frames)
        assert all(same_frames(a, b) for a, b in zip(off.frames, on.frames))
        assert (on.pictures, on.mbs, on.slice_qcodes, on.gops, on.repeated_headers, on.units, on.sequence) == \
               (off.pictures, off.mbs, off.slice_qcodes, off.gops, off.repeated_headers, off.units, off.sequence)
    for name, (s, want) in sorted(C.refusals().items()):
        if name != "b_picture":
            assert B.spec_cached(s) == (None, want), name
            check(s)


# ---- refusals ----
@pytest.mark.parametrize("name", sorted(B.refusals()))
def test_refusals(name):
    s, want = B.refusals()[name]
    d, at = B.spec_cached(s)
    assert d is None and at == want, (at, want)
    check(s)


def test_b_picture_refused_as_before_with_the_option_off():
    s, want = C.refusals()["b_picture"]
    assert B.spec(s, b_pictures=False) == (None, want) == C.spec_cached(s)
    # with the option on the same stream - I B - is refused at the same header for another reason: one anchor in front
    assert B.spec(s) == (None, want)
    for name, (x, _) in sorted(B.cases().items()):
        first_b = [a for (k, a), t in zip([u for u in B.cases()[name][1]["units"] if u[0] == "picture"], B.cases()[name][1]["pictures"]) if t == 3][0]
        assert B.spec(x, b_pictures=False) == (None, first_b), name


# ---- altered streams ----
def test_altered_streams():
    cases = B.altered()
    assert check(B.altered_base()[0]) is not None
    s, L = B.altered_base()
    pic, first = [a for k, a in L["units"] if k == "picture"][2], [a for k, a in L["units"] if k == "slice"][4]
    assert [n for n, _ in cases if n.startswith("bit")] == ["bit%d" % b for b in range(8 * pic, 8 * first)]
    assert sum(not n.startswith("bit") for n, _ in cases) >= 300
    accepted = sum(B.spec_cached(x)[0] is not None for _, x in cases)
    refused = len(cases) - accepted
    print("%d altered streams: %d refused, %d accepted by the definition" % (len(cases), refused, accepted))
    assert accepted >= 50 and refused >= 50
    for name, x in cases:
        check(x)


def test_edges():
    s = B.cases()["order_IPBBI"][0]
    f, r = B.host_decode(s, cap=5 * 2304 - 1)
    assert f is None and r["status"] == D.OVERFLOW and r["out_bytes"] == 0
    assert B.host_decode(s, cap=5 * 2304)[1]["status"] == D.OK
    for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64)):
        check(x)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(s, "iso") for _, s in B.all_streams()] + [(B.wide()[0], "iso")] + [(s, "iso") for s, _ in C.cases().values()]
    path = tmp_path / "streams.bin"
    path.write_bytes(D.pack_streams(items))
    exe = str(tmp_path / "dec_b_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_b_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    for k in (0, 5, len(B.cases()), len(B.cases()) + 3, 100, 400, len(items) - 1):
        want = B.host_decode(items[k][0], D.LAYOUTS[k & 3])[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
