"""Field pictures (option "decode_field_pictures") on the CPU: the fp_ functions of csrc/m2v_decode_kernels.hpp and the serial harness
tools/dec_f_host.hpp, compiled with g++, against decoder.decode(..., syntax="main", interlaced=True, extended=True, mb_tools=True,
field_pictures=True) - frames, counts, verdict and err_offset on every stream of tests/fld_cases.py; the known answers, which the new
code did not make (the option-off decoder on the two progressive twins, the numpy reference tests/fld_ref.py with every classic wrong
form shown to change the frames, a literal picture); the refusals with their offsets stated by hand; the streams of the older options,
which keep their answers; the altered streams; the plan streams, planned in 256 ranges of events and in other numbers of them; and the
host build once under AddressSanitizer and UBSan as a stand-alone program.  tests/test_gpu_decode_fld.py runs the same streams on the
device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dec_cases as D
import ext_cases as X
import fld_cases as F
import fld_ref as FR
import ilace_cases as IC
import mbt_cases as T

M = D.M


def check(stream, b, layouts=("i420",), lanes=(256,)):
    """the host build answers what the definition answers: frames and counts, or the refusal and its offset"""
    d, at = F.spec_cached(bytes(stream), b)
    for layout in layouts:
        for n in lanes:
            f, r = F.host_decode(stream, b, layout, lanes=n)
            if d is None:
                assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0), (r, at, n)
            else:
                assert r["status"] == D.OK, r
                assert np.array_equal(f, D.frames_of(d, layout)) if d.frames else f.shape == (0, r["frame_bytes"]), (layout, n)
                want = F.record_of(d, stream)
                assert {k: r[k] for k in want} == want and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def flat(frames):
    return np.stack([np.concatenate([p.reshape(-1) for p in f]) for f in frames])


# ---- the interface of the definition ----
def test_the_keyword():
    s, L, b = F.cases()["ip_only"]
    kw = dict(quirks=False, syntax="main", interlaced=True, extended=True, mb_tools=True)
    for missing in ("interlaced", "extended", "mb_tools"):
        with pytest.raises(ValueError):
            M.decoder.decode(s, field_pictures=True, **dict(kw, **{missing: False}))
    with pytest.raises(ValueError):
        M.decoder.decode(s, field_pictures=True)
    assert len(M.decoder.decode(s, field_pictures=True, **kw).frames) == 4
    with pytest.raises(M.decoder.Refused) as e:                      # without the keyword: the parent's refusal, at the first coding extension
        M.decoder.decode(s, **kw)
    assert e.value.offset == [a for k, a in L["units"] if k == "picture_ext"][0]


# ---- the valid cases ----
@pytest.mark.parametrize("name", sorted(F.cases()))
def test_valid_cases(name):
    s, L, b = F.cases()[name]
    d = check(s, b, D.LAYOUTS, lanes=(256, 1))
    assert d is not None and [p["type"] for p in d.fields] == L["pictures"]
    assert [(p["picture_structure"], p["second"], p["frame"]) for p in d.fields] == [(f["ps"], f["second"], f["frame"]) for f in L["fields"]]
    assert len(d.frames) == len(d.pictures) == 1 + L["fields"][-1]["frame"]
    assert F.spec_cached(s, b, False)[0] is None                     # refused with the option off
    for bb in F.settings(b):
        assert check(s, bb) is not None


def test_what_the_cases_reach():
    """from the writer's log: every motion type in P and B fields of either parity, either select in either direction and in either
    half, dual prime in both parities, every kind of pair in either order, skipped runs in P and B fields, macroblocks without a vector,
    concealment vectors, Table B-15, frame pictures between field pairs, rows cut 3, 1 + 2 and 1 + 1 + 1, a second field that reads the
    first field of its own frame and one that cannot read its own parity"""
    mbs, pairs, fields, b15, cuts = [], set(), [], 0, set()
    for name, (s, L, b) in F.cases().items():
        mbs += L["fmbs"]
        pairs |= L["pairs"]
        fields += L["fields"]
        b15 += len(L["b15"])
        cuts |= {c["slices"] for c in L["cuts"]}
    assert {(m["type"], m["ps"], m["motion"]) for m in mbs if m["motion"]} >= {(t, ps, k) for t in (2, 3) for ps in (1, 2) for k in ("field", "16x8")} | {(2, 1, "dual"), (2, 2, "dual")}
    assert pairs == {(ps, a, c) for ps in (1, 2) for a, c in ((1, 1), (1, 2), (2, 2), (3, 3))}
    for name in ("fwd", "bwd"):
        assert {m[name][0] for m in mbs if m["motion"] == "field" and not m["skipped"] and m[name] is not None} == {0, 1}
        assert {(m[name][0][0], m[name][1][0]) for m in mbs if m["motion"] == "16x8" and m[name] is not None} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {m["type"] for m in mbs if m["skipped"]} == {2, 3}
    assert any(m["skipped"] and m["fwd"] is not None and m["bwd"] is not None for m in mbs) and any(m["skipped"] and m["type"] == 3 and m["bwd"] is None for m in mbs)
    assert any(m["kind"] == "nomc" for m in mbs) and any(m["cmv"] is not None and m["cmv"][0] == 1 for m in mbs) and b15
    assert {f["ps"] for f in fields} == {1, 2, 3} and cuts >= {1, 2, 3}
    second_p = [m for m in mbs if m["type"] == 2 and m["second"] and m["motion"] == "field"]
    assert {m["fwd"][0] == m["ps"] - 1 for m in second_p} == {False, True}      # the first field of its own frame, and the frame in front
    firsts = [m for m in mbs if m["frame"] == 0 and m["second"] and m["type"] == 2 and m["motion"]]
    assert firsts and all(m["motion"] == "field" and m["fwd"][0] != m["ps"] - 1 or m["motion"] == "16x8" for m in firsts)


# ---- the known answers ----
@pytest.mark.parametrize("name", sorted(F.known()))
def test_known_answers(name):
    """frames the new code did not make: the option-off definition on the two progressive twins, tests/fld_ref.py, a literal"""
    s, b, want = F.known()[name]
    d = check(s, b, lanes=(256, 2))
    assert d is not None and np.array_equal(D.frames_of(d), flat(want)), name


def test_the_twins_are_option_off_streams():
    s, halves = F.twin()
    for h in halves:
        assert M.decoder.decode(h, quirks=False, syntax="main", b_pictures=True).frames[0][0].shape == (32, 48)
    assert F.spec_cached(s, True, False)[0] is None


@pytest.mark.parametrize("name", sorted(F.ref_cases()))
def test_every_wrong_form_changes_the_frames(name):
    s, log, b, wrong = F.ref_cases()[name]
    good = flat(FR.frames(log))
    for w in wrong:
        assert not np.array_equal(flat(FR.frames(log, w)), good), w


def test_every_wrong_form_has_a_case():
    assert {w for v in F.ref_cases().values() for w in v[3]} == set(FR.WRONG) and len(FR.WRONG) == 15


# ---- the refusals ----
@pytest.mark.parametrize("name", sorted(F.refusals()))
def test_refusals(name):
    """the offset is stated by hand, from the writer's log"""
    s, b, f, want = F.refusals()[name]
    assert F.spec_cached(s, b, f) == (None, want), name
    if f:
        check(s, b, lanes=(256, 1, 3))


def test_the_refusals_break_a_stream_that_is_accepted():
    """the stream every refusal breaks in one place decodes as it stands"""
    assert len(F.refusals()) >= 24
    s, L = F.FW.stream(32, 32, F.refusal_base())
    assert check(s, True) is not None and len(L["fields"]) == 6


# ---- the older options keep their answers ----
NEWLY_LEGAL = {"older_main_field_picture"}                           # its picture_structure is legal now: a first field alone, refused at its own picture header


def test_streams_of_the_older_options_keep_their_answers():
    """every stream of mbt_cases, ext_cases and ilace_cases gives the same answer with the option on as with it off (the three options
    it needs on both times) - but for the one that was refused for being a field picture: it is still refused, one unit earlier, as a
    first field that no picture follows"""
    n = 0
    streams = [(k, s, b) for k, s, b, i in T.all_streams()] + [(k, s, b) for k, s, b, i in X.all_streams()] + [(k, s, b) for k, s, b in IC.all_streams()]
    for name, s, b in streams:
        off = F.spec_cached(bytes(s), b, False)
        on = F.spec_cached(bytes(s), b, True)
        if name in NEWLY_LEGAL:
            units = [a for a, _ in M.decoder.start_codes(s)]
            assert off[0] is None and on[0] is None and on[1] == units[units.index(off[1]) - 1] and s[on[1] + 3] == 0x00
            n += 1
            continue
        assert (off[0] is None) == (on[0] is None) and off[1] == on[1], name
        if off[0] is not None:
            assert np.array_equal(D.frames_of(off[0]), D.frames_of(on[0])) and F.record_of(off[0], s) == F.record_of(on[0], s)
        check(s, b)
    assert n == len(NEWLY_LEGAL) and len(streams) > 1000


# ---- altered streams, plan streams ----
def test_altered_streams():
    """300 seeded alterations of the units of an I P B B stream of field pairs: the host build gives the definition's verdict and offset
    on each.  Between 30 and 270 are refused"""
    cases = F.altered()
    assert len(cases) == 300
    refused = sum(check(x, True) is None for _, x in cases)
    assert 30 <= refused <= 270, refused


@pytest.mark.parametrize("name", sorted(F.plan_streams()))
def test_plan_streams(name):
    """a pair parted by a range's edge plans as one inside a range does: the same answer in 256 ranges, in one, and in numbers between"""
    s, L, b = F.plan_streams()[name]
    nev = len(M.decoder.start_codes(s))
    assert nev > 256
    d = check(s, b, lanes=(256, 1, 7, 100))
    assert d is not None and len(d.frames) == 1 + L["fields"][-1]["frame"]
    if name == "long":
        assert len(d.frames) > 256


def test_the_shifts_put_an_edge_at_every_position_of_a_pair():
    """over shift_0 .. shift_6 a range's edge falls in front of every kind of unit of a pair: the second field's header, a field's
    coding extension, a field's slice - and between the two slices of a frame picture"""
    seen = set()
    for k in range(7):
        s, L, b = F.plan_streams()["shift_%d" % k]
        ev = M.decoder.start_codes(s)
        per = (len(ev) + 255) // 256
        kinds = {a: kind for kind, a in L["units"]}
        second = {}
        n = -1
        for kind, a in L["units"]:
            if kind == "picture":
                n += 1
            second[a] = n >= 0 and L["fields"][n]["second"], n >= 0 and L["fields"][n]["ps"]
        for i in range(per, len(ev), per):
            at = ev[i][0]
            seen.add((kinds[at], second[at][0], second[at][1] != 3, kinds[ev[i - 1][0]]))
    for kind in ("picture", "picture_ext", "slice"):
        assert any(s[0] == kind and s[1] and s[2] for s in seen), kind           # in front of a second field's units
        assert any(s[0] == kind and not s[1] and s[2] for s in seen), kind       # and of a first field's
    assert any(s[0] == "slice" and not s[2] and s[3] == "slice" for s in seen)   # between a frame picture's slices


def test_degenerate_inputs():
    for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64), b"\x00\x00\x01\xb5\x80", b"\x00\x00\x01\x01", b"\x00\x00\x01\x00\x00\x0f\xff\xf8\x00\x00\x01\xb5\x8f\xff\xf1"):
        for b in (False, True):
            check(x, b)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(s, b) for _, s, b in F.all_streams()] + [(v[0], v[2]) for v in T.cases().values()]
    path = tmp_path / "streams.bin"
    path.write_bytes(b"".join([struct.pack("<I", len(items))] + [struct.pack("<IQ", int(bool(b)), len(s)) + bytes(s) for s, b in items]))
    exe = str(tmp_path / "dec_f_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_f_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    for line, (s, b) in zip(lines, items):
        k, status, err, pictures, _ = line.split()
        d, at = F.spec_cached(bytes(s), b)
        assert (int(status), int(err)) == ((D.OK, 0) if d is not None else (D.SYNTAX, at)), line
