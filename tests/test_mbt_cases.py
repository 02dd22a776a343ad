"""Table B-15, concealment motion vectors and dual prime (option "decode_mb_tools") on the CPU: the t_ functions of
csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_t_host.hpp, compiled with g++, against
decoder.decode(..., syntax="main", extended=True, mb_tools=True) - frames, counts, verdict and err_offset on every stream of
tests/mbt_cases.py; the known answers, which the new code did not make (the option-off decoder on twin streams, the numpy reference
tests/mbt_ref.py with every classic wrong form shown to change the frames, one literal picture); the refusals with their offsets
stated by hand; the streams of the extended option; the invariants of Table B-15 against the project's own B-14; the altered
streams; and the host build once under AddressSanitizer and UBSan as a stand-alone program.
tests/test_gpu_decode_mbt.py runs the same streams on the device."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dec_cases as D
import ext_cases as X
import mbt_cases as T
import mbt_ref as TR
import mbt_writer as TW

M = D.M


def check(stream, b, i, layouts=("i420",)):
    """the host build answers what the definition answers: frames and counts, or the refusal and its offset"""
    d, at = T.spec_cached(stream, b, i)
    for layout in layouts:
        f, r = T.host_decode(stream, b, i, layout)
        if d is None:
            assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0), (r, at)
        else:
            assert r["status"] == D.OK, r
            assert np.array_equal(f, D.frames_of(d, layout)) if d.frames else f.shape == (0, r["frame_bytes"]), layout
            want = T.record_of(d, stream)
            assert {k: r[k] for k in want} == want and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def same_frames(fa, fb):
    return len(fa) == len(fb) and all(np.array_equal(a, b) for x, y in zip(fa, fb) for a, b in zip(x, y))


# ---- the interface of the definition ----
def test_the_keyword():
    s, L, b, i = T.cases()["b15_mixed"]
    with pytest.raises(ValueError):                                 # mb_tools without extended
        M.decoder.decode(s, quirks=False, syntax="main", b_pictures=True, mb_tools=True)
    with pytest.raises(ValueError):
        M.decoder.decode(s, mb_tools=True)
    d = M.decoder.decode(s, quirks=False, syntax="main", b_pictures=True, extended=True, mb_tools=True)
    assert len(d.frames) == 4
    with pytest.raises(M.decoder.Refused) as e:                     # without the option: the parent's answer, at the first coding extension
        M.decoder.decode(s, quirks=False, syntax="main", b_pictures=True, extended=True)
    assert e.value.offset == [a for k, a in L["units"] if k == "picture_ext"][0]


# ---- Table B-15 against the project's own B-14 ----
def _bits(code, length):
    return format(code, "0%db" % length)


def b14():
    """the project's B-14 as {(run, level): code string}; (0, 1) in its '11' form"""
    return {pair: _bits(code, length) for code, length, pair in M.decoder.iso_tables()["ac"]}


def test_b15_codes_the_pairs_of_b14():
    """(a) B-15 codes exactly B-14's 111 (run, level) pairs, plus end of block, plus escape - in all three typings"""
    for table in (TW.b15_codes(), {pair: _bits(c, l) for c, l, pair in M.decoder.b15_table()}):
        assert len(table) == 111 and set(table) == set(b14())
        assert len(set(table.values()) | {TW.B15_EOB, TW.ESCAPE}) == 113
    assert M.decoder._B15_EOB == TW.B15_EOB == "0110" and M.decoder._B14_ESCAPE == TW.ESCAPE == "000001"
    assert {pair: _bits(c, l) for c, l, pair in M.decoder.b15_table()} == TW.b15_codes()


def test_b15_shares_the_long_codes():
    """(b) the 70 codes the tables share are B-14's that begin with seven zero bits, but for the ten pairs (0, 8) .. (0, 15), (1, 5),
    (2, 4); the B-14 codewords of those ten begin no code of B-15"""
    t14, t15 = b14(), TW.b15_codes()
    moved = set(TW.B15_MOVED)
    assert moved == {(0, l) for l in range(8, 16)} | {(1, 5), (2, 4)} == set(M.decoder._B15_MOVED)
    long14 = {p for p, c in t14.items() if c.startswith("0000000")}
    assert moved <= long14 and len(long14 - moved) == 70
    assert {p for p in t14 if t14[p] == t15[p]} == (long14 - moved) | {(3, 1), (5, 1)}      # two of the 41 short codes are B-14's as well
    assert set(TW.B15) == set(t14) - (long14 - moved) and len(TW.B15) == 41
    every = list(t15.values()) + [TW.B15_EOB, TW.ESCAPE]
    for p in moved:
        assert not any(t14[p].startswith(c) or c.startswith(t14[p]) for c in every), p


def test_b15_short_codes_are_prefix_free_and_complete():
    """(c) the 41 codes, '0110' and '000001' are prefix-free and their Kraft sum is 1 - 2^-7: every window that does not begin with
    seven zeros begins exactly one of them"""
    codes = list(TW.B15.values()) + [TW.B15_EOB, TW.ESCAPE]
    assert len(codes) == len(set(codes)) == 43
    assert not any(a != b and a.startswith(b) for a in codes for b in codes)
    assert sum(Fraction(1, 2 ** len(c)) for c in codes) == 1 - Fraction(1, 2 ** 7)
    assert not any(c.startswith("0000000") for c in codes)


def test_b15_lookup_agrees_on_every_window():
    """(d) all 2^17 windows give the same (length, run, level) in vlc_ac15 and in decoder.py's table - with zeros and with ones behind
    the window"""
    table = {_bits(c, l): pair for c, l, pair in M.decoder.b15_table()}
    table[TW.B15_EOB], table[TW.ESCAPE] = (0, 0), (1, 0)
    by_len = {}
    for bits, pair in table.items():
        by_len.setdefault(len(bits), {})[int(bits, 2)] = pair
    want = np.zeros(1 << 17, np.uint32)
    w = np.arange(1 << 17, dtype=np.uint32)
    for n, codes in by_len.items():
        for code, (run, level) in codes.items():
            hit = (w >> (17 - n)) == code
            assert not want[hit].any()                              # prefix-free: one code a window at most
            want[hit] = n | run << 8 | level << 16
    assert max(by_len) <= 17
    for fill in (0, 1):
        got = np.zeros(1 << 17, np.uint32)
        T.host_lib().dec_t_host_ac15(17, fill, got.ctypes.data)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert (want[w >> 10 != 0] != 0).all() and (want == 0).sum() > 0


def test_half():
    """h(a) = (a + (a > 0)) >> 1 is a / 2 rounded to the nearest integer, halves away from zero - stated without a shift"""
    for a in range(-40, 41):
        want = (abs(a) + 1) // 2 * (1 if a > 0 else -1)
        assert T.host_lib().dec_t_host_half(a) == want == TR.half(a)


# ---- every case ----
@pytest.mark.parametrize("name", sorted(T.cases()))
def test_valid_cases(name):
    s, L, b, i = T.cases()[name]
    d = check(s, b, i, D.LAYOUTS)
    assert d is not None and [p["type"] for p in d.pictures] == L["pictures"]
    assert d.units == D.prefixes(s) == len(L["units"])
    frames = [check(s, bb, ii).frames for bb, ii in T.settings(b, i)]
    assert len(frames) == len(T.settings(b, i)) and all(same_frames(frames[0], f) for f in frames[1:])
    if b:
        assert T.spec_cached(s, False, i)[0] is None
    if i:
        assert T.spec_cached(s, b, False)[0] is None


@pytest.mark.parametrize("name", sorted(T.known()))
def test_known_answers(name):
    """frames the new code did not make: the option-off definition on the twin stream, tests/mbt_ref.py, a literal"""
    s, b, i, want = T.known()[name]
    d = check(s, b, i)
    assert d is not None and same_frames(d.frames, want)
    assert T.spec(s, b, i, mb_tools=False)[0] is None               # the stream itself needs the option


def test_what_the_cases_reach():
    """from the writer's log: all 113 codes of Table B-15 with both signs, escapes at both ends of the level range and a forced one,
    '0110' directly behind the DC; B-15 in intra macroblocks of P and B pictures beside coded non-intra blocks in the same slice, both
    scans, several slices a row; concealment vectors in I, P and B pictures, one in front of a predicted macroblock's vector, one
    behind predictors that were not zero; every dmvector, both orders of the fields"""
    c = T.cases()
    L = c["b15_every_code"][1]
    pairs = set(TW.b15_codes())
    assert len(pairs) == 111 and L["b15"] == {(r, l, s) for r, l in pairs for s in (False, True)} | {(None, 0, 0)}
    esc = L["b15_escapes"]
    assert {(0, 2047), (0, -2047), (62, 1), (0, 1), (0, 41), (32, 1)} <= set(esc)
    L = c["b15_mixed"][1]
    assert L["pictures"] == [1, 2, 3, 3] and {p[3] for p in L["params"]} == {0, 1}           # both scans
    for pic in (1, 2, 3):                                           # an intra and a coded predicted macroblock in one slice
        rows = {}
        for m, cut in ((m, [x for x in L["cuts"] if x["pic"] == pic and x["row"] == m["row"] and x["first"] <= m["col"] <= x["last"]][0]) for m in L["tmbs"] if m["pic"] == pic):
            rows.setdefault((m["row"], cut["first"]), set()).add("intra" if m["kind"] == "intra" else "coded" if m["cbp"] else "plain")
        assert any({"intra", "coded"} <= kinds for kinds in rows.values()), pic
    assert max(x["slices"] for x in L["cuts"]) >= 2
    assert {c[n][1]["pictures"][p] for n in ("cmv_ip", "cmv_b", "cmv_fields") for p, *_ in c[n][1]["cmvs"]} == {1, 2, 3}
    L = c["cmv_ip"][1]
    assert any(behind and v != (0, 0) for p, r, col, v, behind in L["cmvs"] if p == 1) and L["kept"] >= 1
    assert c["cmv_b"][1]["kept"] >= 1 and c["cmv_fields"][1]["kept"] >= 1
    duals = [x for n in ("dual_vectors", "dual_bottom_field_first", "dual_predictors") for x in c[n][1]["duals"]]
    assert {x[4][0] for x in duals} == {x[4][1] for x in duals} == {-1, 0, 1} and {x[5] for x in duals} == {0, 1}
    assert any(v[0] > 0 and v[0] & 1 for *_, v, d, t in duals) and any(v[1] < 0 and v[1] & 1 for *_, v, d, t in duals)
    L = c["all_tools"][1]
    assert L["duals"] and L["cmvs"] and L["b15"] and L["selects"]


@pytest.mark.parametrize("name", sorted(T.dual_cases()))
def test_every_wrong_form_changes_the_frames(name):
    """tests/mbt_ref.py agrees with the definition as it stands, and each classic wrong form changes the frames of its case"""
    s, log, wrong = T.dual_cases()[name]
    d = check(s, False, True)
    good = TR.frames(log)
    assert d is not None and same_frames(d.frames, good)
    for w in wrong:
        assert not same_frames(TR.frames(log, w), good), w


def test_every_wrong_form_has_a_case():
    assert {w for _, _, wrong in T.dual_cases().values() for w in wrong} == set(TR.WRONG)


# ---- the refusals ----
@pytest.mark.parametrize("name", sorted(T.refusals()))
def test_refusals(name):
    """the offset is stated by hand, from the writer's log"""
    s, b, i, t, want = T.refusals()[name]
    assert T.spec_cached(s, b, i, t) == (None, want), name
    if t:
        check(s, b, i)
    else:                                                           # the stream is a valid one of the option
        assert check(s, b, i) is not None
        f, r = X.host_decode(s, b, i)                               # and the extended path's harness refuses it where the definition does
        assert f is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want)


def test_refusals_reach_what_they_name():
    r = T.refusals()
    assert len([n for n in r if n.startswith("b14_code_of_")]) == 10
    s, b, i, t, at = r["dual_with_frame_pred_frame_dct_1"]
    assert T.spec_cached(s, b, True, t) == (None, at)               # whatever "decode_interlaced" says
    for name in ("derived_outside_top", "derived_outside_bottom", "derived_outside_left", "derived_outside_right"):
        assert r[name][4] > 0


# ---- the streams of the extended option ----
def test_streams_of_the_extended_option_keep_their_answers():
    """every valid case, known answer, refusal and older refusal of ext_cases decodes, option on, to the verdict, the offset and the
    frames it has with the option off - but for the two whose flag is legal now: they are still refused, at the slice the flag garbles"""
    n = 0
    for name, s, b, i in T.extended_streams():
        off = X.spec_cached(s, b, i)
        on = T.spec_cached(s, b, i)
        if name in T.NEWLY_LEGAL:
            assert on[0] is None and on[1] > off[1] and s[on[1]:on[1] + 3] == b"\x00\x00\x01" and 1 <= s[on[1] + 3] <= 0xAF, name
            check(s, b, i)
            continue
        assert (on[0] is None) == (off[0] is None) and on[1] == off[1], name
        d = check(s, b, i)
        if d is not None:
            assert same_frames(d.frames, off[0].frames) and T.record_of(d, s) == T.record_of(off[0], s), name
        n += 1
    assert n >= 120


def test_invariant_on_the_valid_streams_of_the_older_options():
    for name, (s, b, i) in sorted(X.older_valid().items()):
        off, _ = X.spec_cached(s, b, i, False)
        on = check(s, b, i)
        assert off is not None and on is not None and same_frames(off.frames, on.frames), name
        assert T.record_of(off, s) == T.record_of(on, s)


# ---- altered streams ----
def test_altered_streams():
    """300 seeded alterations of the slice data of the stream with all three tools: the host build gives the definition's verdict and
    offset on each.  Both verdicts occur more than a tenth of the time"""
    cases = T.altered()
    assert len(cases) == 300
    accepted = sum(check(x, False, True) is not None for _, x in cases)
    assert 30 <= accepted <= 270, accepted


def test_degenerate_inputs():
    for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64), b"\x00\x00\x01\xb5\x80", b"\x00\x00\x01\x01"):
        for b in (False, True):
            check(x, b, False)
            check(x, b, True)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(s, b, i) for _, s, b, i in T.all_streams()] + [(s, b, i) for _, s, b, i in T.extended_streams()]
    path = tmp_path / "streams.bin"
    path.write_bytes(T.pack_streams(items))
    exe = str(tmp_path / "dec_t_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_t_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    for k in (0, 5, len(T.cases()), len(T.cases()) + 3, 100, 300, len(items) - 1):
        want = T.host_decode(items[k][0], items[k][1], items[k][2], D.LAYOUTS[k & 3])[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
