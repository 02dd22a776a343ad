"""Several slices a row, slice header extras, quant_matrix_extension and composite_display_flag 1 (option "decode_extended") on the CPU:
the x_ functions of csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_x_host.hpp, compiled with g++, against
decoder.decode(..., syntax="main", extended=True) - frames, counts, verdict and err_offset on every stream of tests/ext_cases.py; the
known answers, which the new code did not make (the option-off decoder on a twin stream, and literal pictures); the refusals with
their offsets stated by hand; the refusals and the valid streams of the older options; what the cases reach, from the writer's log;
the altered streams; and the host build once under AddressSanitizer and UBSan as a stand-alone program.
tests/test_gpu_decode_ext.py runs the same streams on the device."""
import os
import subprocess

import numpy as np
import pytest

import dec_cases as D
import ext_cases as X

M = D.M


def check(stream, b, i, layouts=("i420",)):
    """the host build answers what the definition answers: frames and counts, or the refusal and its offset"""
    d, at = X.spec_cached(stream, b, i)
    for layout in layouts:
        f, r = X.host_decode(stream, b, i, layout)
        if d is None:
            assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0), (r, at)
        else:
            assert r["status"] == D.OK, r
            assert np.array_equal(f, D.frames_of(d, layout)) if d.frames else f.shape == (0, r["frame_bytes"]), layout
            want = X.record_of(d, stream)
            assert {k: r[k] for k in want} == want and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def same_frames(fa, fb):
    return len(fa) == len(fb) and all(np.array_equal(a, b) for x, y in zip(fa, fb) for a, b in zip(x, y))


# ---- the interface of the definition ----
def test_the_keyword():
    s, L, b, i = X.cases()["ip_cut"]
    with pytest.raises(ValueError):
        M.decoder.decode(s, quirks=False, syntax="module", extended=True)
    with pytest.raises(ValueError):
        M.decoder.decode(s, extended=True)
    d = M.decoder.decode(s, quirks=False, syntax="main", extended=True)
    assert len(d.frames) == 2 and sum(len(q) for q in d.slice_qcodes) == len(L["cuts"]) == 7
    with pytest.raises(M.decoder.Refused) as e:                     # without the option: the parent's answer, at the first second slice of a row
        M.decoder.decode(s, quirks=False, syntax="main")
    slices = [a for k, a in L["units"] if k == "slice"]
    assert e.value.offset in slices[1:]


def test_spans_and_continuity():
    """x_continuous over every pair of spans of a row of three: exactly the pairs that continue each other pass"""
    L = X.host_lib()
    span = lambda code, a, b: L.dec_x_host_span(1, code, a, b)
    for a in range(3):
        for b in range(a, 3):
            assert bool(L.dec_x_host_continuous(span(1, a, b), 0, 0, 2, 3)) == (a == 0)                  # a picture's first slice
            assert bool(L.dec_x_host_continuous(span(2, a, b), span(1, 0, 2), 1, 2, 3)) == (a == 0 and b == 2)      # the last one, on a new row
            for c in range(3):
                for e in range(c, 3):
                    assert bool(L.dec_x_host_continuous(span(1, a, b), span(1, c, e), 1, 3, 3)) == (a == e + 1)      # the same row
                    assert bool(L.dec_x_host_continuous(span(2, a, b), span(1, c, e), 1, 3, 3)) == (a == 0 and e == 2)   # the next row
                    assert bool(L.dec_x_host_continuous(span(1, a, b), span(1, c, e), 2, 3, 3)) == (a == e + 1 and b == 2)


# ---- every case ----
@pytest.mark.parametrize("name", sorted(X.cases()))
def test_valid_cases(name):
    s, L, b, i = X.cases()[name]
    d = check(s, b, i, D.LAYOUTS)
    assert d is not None and [p["type"] for p in d.pictures] == L["pictures"]
    assert d.units == D.prefixes(s) == len(L["units"])
    assert [len(q) for q in d.slice_qcodes] == [sum(c["pic"] == k for c in L["cuts"]) for k in range(len(d.pictures))]


@pytest.mark.parametrize("name", sorted(X.known()))
def test_known_answers(name):
    """frames the new code did not make: the option-off definition on the twin stream, or literal pictures"""
    s, b, i, want = X.known()[name]
    d = check(s, b, i)
    assert d is not None and same_frames(d.frames, want)
    if name not in ("flat_literal",):
        assert X.spec(s, b, i, extended=False)[0] is None           # the stream itself needs the option


def test_what_the_cases_reach():
    """from the writer's log: every way of cutting a row of three, a cut in front of and behind a skipped run, predictors that were not
    zero reset by a cut, every length of the extras with intra_slice either way, every combination of the load flags, a first
    increment behind macroblock_escape, 288 slices"""
    c = X.cases()
    rows = {}
    for name in ("ipbb_cut", "ipbb_cut_shifted", "ip_cut"):         # (a row with a skipped macroblock cannot be cut next to it: the cycle is shifted)
        for cut in c[name][1]["cuts"]:
            rows.setdefault((name, c[name][1]["pictures"][cut["pic"]], cut["pic"], cut["row"]), []).append((cut["first"], cut["last"]))
    ways = {((0, 2),), ((0, 0), (1, 2)), ((0, 1), (2, 2)), ((0, 0), (1, 1), (2, 2))}
    assert {tuple(v) for v in rows.values()} == ways
    for ptype in (1, 2, 3):                                         # every picture type cut in two and in three
        assert {len(v) for k, v in rows.items() if k[1] == ptype} >= {2, 3}, ptype
    L = c["ipbb_cut"][1]
    assert L["dc_rederived"] >= 1 and L["vectors_rederived"] >= 1
    assert any(x["skip_behind_first"] for x in L["cuts"] if x["pic"] == 1)                     # a P picture's skipped macroblock inside a slice
    L = c["skip_run"][1]
    mid = [x for x in L["cuts"] if x["pic"] == 1 and x["first"] == 1][0]
    assert (mid["last"], mid["skip_behind_first"], mid["skip_before_last"], mid["slices"]) == (3, True, True, 3)
    L = c["fields_cut"][1]
    row1 = [m for m in L["ilmbs"] if m["pic"] == 1 and m["motion"] == "field" and m["incr"] in (1, 2, 3)]
    assert len([x for x in L["cuts"] if x["pic"] == 1 and x["slices"] == 3]) == 3 and len(row1) >= 3      # field vectors on either side of a cut
    assert L["vectors_rederived"] >= 1
    assert [x["first"] for x in c["escape"][1]["cuts"]] == [0, 33, 34]
    assert len(c["many"][1]["cuts"]) == 288 and all(x["first"] == x["last"] for x in c["many"][1]["cuts"])
    assert set(c["headers"][1]["extras"]) >= {(0, 0), (1, 1), (3, 0), (0, 1), (1, 0), (3, 1)}
    loads = [c["quant_" + n][1]["loads"][0] for n in ("intra", "non_intra", "both", "neither")]
    assert loads == [(1, 0), (0, 1), (1, 1), (0, 0)]
    for k, kinds in enumerate((["user", "quant_matrix"], ["quant_matrix", "picture_display"], ["picture_display", "quant_matrix", "user", "copyright"])):
        units = [u for u, _ in c["quant_beside_%d" % k][1]["units"]]
        at = units.index("picture_ext")
        assert units[at + 1:at + 1 + len(kinds)] == kinds
    assert [u for u, _ in c["quant_per_picture"][1]["units"]].count("sequence") == 2
    assert c["quant_coded_order"][1]["pictures"] == [1, 2, 3, 3]


# ---- the refusals ----
@pytest.mark.parametrize("name", sorted(X.refusals()))
def test_refusals(name):
    """the offset is stated by hand, from the writer's log"""
    s, b, i, want = X.refusals()[name]
    assert X.spec_cached(s, b, i) == (None, want), name
    check(s, b, i)


def test_refusals_of_the_older_options_stay():
    """every refusal of main_cases, bpic_cases and ilace_cases that is not about a construct the option accepts is refused at the same
    unit with the option on (bpic's skipped_last_of_row: a slice that ends short may be continued now, so the rule names the next one)"""
    assert len(X.older_refusals()) >= 60
    for name, (s, b, i, want) in sorted(X.older_refusals().items()):
        assert X.spec_cached(s, b, i) == (None, want), name
        check(s, b, i)


# ---- the invariant ----
def test_invariant_on_the_valid_streams_of_the_older_options():
    """every stream the main syntax accepts with the option off decodes with it on to the same frames and the same record"""
    assert len(X.older_valid()) >= 50
    for name, (s, b, i) in sorted(X.older_valid().items()):
        off, _ = X.spec_cached(s, b, i, False)
        on = check(s, b, i)
        assert off is not None and on is not None and same_frames(off.frames, on.frames), name
        assert X.record_of(off, s) == X.record_of(on, s) and off.slice_qcodes == on.slice_qcodes


def test_every_setting_of_the_other_two_options():
    """a cut I / P stream of progressive pictures decodes to the same frames under all four settings"""
    s = X.cases()["ip_cut"][0]
    frames = [check(s, b, i).frames for b in (False, True) for i in (False, True)]
    assert all(same_frames(frames[0], f) for f in frames[1:])
    s = X.cases()["ipbb_cut"][0]                                    # B pictures with "decode_b_pictures" off: at the first B picture's header
    at = [a for k, a in X.cases()["ipbb_cut"][1]["units"] if k == "picture"][2]
    assert X.spec_cached(s, False, False) == (None, at) and check(s, False, True) is None


# ---- altered streams ----
def test_altered_streams():
    """300 seeded alterations of a cut stream with slice extras and a quant_matrix_extension.  Counted on the CPU before the bound was
    written: the definition accepts 145 of the 300 and refuses 155; of the evenly sampled half the GPU test takes it accepts 54 and
    refuses 96 - both more than a tenth"""
    cases = X.altered()
    assert len(cases) == 300
    accepted = sum(check(x, True, False) is not None for _, x in cases)
    assert 30 <= accepted <= 270
    sample = X.altered_sample()
    acc = sum(X.spec_cached(x, True, False)[0] is not None for _, x in sample)
    assert len(sample) == 150 and 15 <= acc <= 135


def test_degenerate_inputs():
    for x in (b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64), b"\x00\x00\x01\xb5\x30", b"\x00\x00\x01\x01"):
        for b in (False, True):
            check(x, b, False)
            check(x, b, True)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(s, b, i) for _, s, b, i in X.all_streams()] + list(X.older_valid().values())
    path = tmp_path / "streams.bin"
    path.write_bytes(X.pack_streams(items))
    exe = str(tmp_path / "dec_x_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_x_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    for k in (0, 5, len(X.cases()), len(X.cases()) + 3, 100, 300, len(items) - 1):
        want = X.host_decode(items[k][0], items[k][1], items[k][2], D.LAYOUTS[k & 3])[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
