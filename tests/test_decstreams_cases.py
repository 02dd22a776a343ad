"""Several streams per call on the CPU: tools/dec_host.hpp's decode_streams - the serial run of what m2v_decode_streams.hip runs,
plan_streams and the output locator included - against the model of tests/decstreams_cases.py on every batch, both modes, all four
layouts; every batch asserted to hold what its name says; the host build once more under AddressSanitizer and UBSan as a stand-alone
program, every segment and the output in allocations of exactly their sizes; check() shown to reject and name single alterations; and
one-line changes of the shared arithmetic each caught by a named batch.  tests/test_gpu_decode_streams_batch.py runs the same batches
on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dec_cases as D
import decstreams_cases as S

M = D.M
GAP = b"\x00\x00\x01"                      # between the segments: a prefix that would make a start code with a segment's first byte


def run(name, layout, mode, cap=None, decode_batch=0, level_bytes=0, lib=None):
    batch = S.batches()[name]
    data, seg = S.place(batch, GAP, lead=1)
    recs, buf = S.host_decode_streams(data, seg, layout, mode, cap=cap, decode_batch=decode_batch, level_bytes=level_bytes, lib=lib)
    S.check(recs, buf, S.expected(batch, layout, mode, cap=cap), base=S.GUARD, segments=seg)
    return recs, buf


def test_record_is_the_headers():
    assert ctypes.sizeof(S.StreamStat) == 88 == M.DECODE_STREAM_STAT_DTYPE.itemsize
    assert M.DECODE_STREAM_STAT_DTYPE.names == ("es_offset", "out_offset", "rec") and M.DECODE_STREAM_STAT_DTYPE["rec"] == M.DECODE_STAT_DTYPE
    hdr = open(os.path.join(D.ROOT, "include", "m2v_mi355x.h")).read()
    for word in ("m2v_decode_streams_device", "m2v_decode_streams_report", "m2v_decode_stream_stat"):
        assert word in hdr
    assert {"m2v_decode_streams_device", "m2v_decode_streams_report"} <= set(M.EXPORTS)
    assert callable(M.frames_of_stream) and callable(M.Mpeg2Encoder.decode_streams) and callable(M.Mpeg2Encoder.decode_streams_report)


NAMES = ("one", "smallest", "mixed", "mixed_reversed", "verdicts", "two_bad", "three", "chunks", "events", "many")      # of S.batches(), without building them


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_model(name):
    assert set(S.batches()) == set(NAMES)
    for mode, _ in S.BOTH:
        for layout in D.LAYOUTS:
            run(name, layout, mode)
    # the probe call reports the layout the decode has
    batch = S.batches()[name]
    data, seg = S.place(batch, GAP, lead=1)
    recs, _ = S.host_decode_streams(data, seg, probe=True)
    want = S.expected(batch, probe=True)["records"]
    assert [(r["out_offset"], r["out_bytes"], r["status"]) for r in recs] == [(w["out_offset"], w["out_bytes"], w["status"]) for w in want]


def test_batches_hold_what_they_say():
    B = S.batches()
    stages = {name: [w["stage"] for w in S.expected(b, mode=mode)["records"]] for name, b in B.items() if name != "many" for mode in ("iso",)}
    for name in ("one", "smallest", "mixed", "mixed_reversed", "three", "chunks", "events"):
        assert set(stages[name]) == {None}, name
    for mode in ("iso", "module"):
        assert [w["stage"] for w in S.expected(B["verdicts"], mode=mode)["records"]] == [None, "probe", None, "slice", None, "probe", "probe", None]
        assert [w["stage"] for w in S.expected(B["two_bad"], mode=mode)["records"]] == [None, "slice", None]
    # the slice-stage refusal is a flip the single-stream probe accepts and the single-stream decode refuses
    fname, x = S.slice_refusal()
    assert fname.startswith("flip") and D.host_decode(x, cap=0)[1]["status"] == D.OVERFLOW and D.host_decode(x)[1]["status"] == D.SYNTAX
    assert S.expected(B["two_bad"])["records"][1]["err_offset"] == D.two_bad_slices()[1]
    # mixed sizes: frame_bytes 3 in front puts the next stream at an odd output offset; five sizes in one call
    mixed = S.expected(B["mixed"])["records"]
    assert mixed[0]["frame_bytes"] == 3 and mixed[1]["out_offset"] % 2 == 1
    assert [(w["width"], w["height"]) for w in mixed] == [(1, 1), (32, 32), (17, 33), (64, 64), (80, 112)]
    # the chunk options cut where claimed: pictures per stream 3, 2, 62, 2
    ch = S.expected(B["chunks"])["records"]
    assert [w["pictures"] for w in ch] == [3, 2, 62, 2] and [(w["width"], w["height"]) for w in ch] == [(32, 32), (64, 64), (64, 64), (32, 32)]
    flat = [(b, p) for b, w in enumerate(ch) for p in range(w["pictures"])]
    data, seg = S.place(B["chunks"], GAP, lead=1)
    for k in (1, 2, 3, 5):
        assert S.host_chunks(data, seg, decode_batch=k) == [flat[a] + (min(k, len(flat) - a),) for a in range(0, len(flat), k)]
    cuts2 = S.host_chunks(data, seg, decode_batch=2)
    assert (0, 2, 2) in cuts2                    # starts at stream 0's second P picture and runs into stream 1: a cut inside a chain, a size change inside
    assert (1, 1, 2) in cuts2                    # between the I and the P picture of the 64 x 64 stream
    assert (0, 0, 3) in S.host_chunks(data, seg, decode_batch=3)      # ends at a stream boundary where the size changes
    assert S.host_chunks(data, seg) == [(0, 0, 69)]                  # the default: the 256 MiB of levels hold all of it, no 256-picture ceiling either
    # the default's bound counts each picture's own macroblocks: 4 a picture, then 16 a picture (one picture at least)
    assert S.host_chunks(data, seg, level_bytes=768 * 10)[:3] == [(0, 0, 2), (0, 2, 1), (1, 0, 1)]
    data, seg = S.place(B["many"], b"")
    assert S.host_chunks(data, seg) == [(0, 0, 4096)]


def test_chunks_and_caps_do_not_change_the_answer():
    for k in (1, 2, 3, 5):
        run("chunks", "i420", "module", decode_batch=k)
        run("verdicts", "nv12", "iso", decode_batch=k)
    run("chunks", "yv12", "iso", level_bytes=768 * 10)
    run("two_bad", "i420", "iso", decode_batch=7)               # the refused stream lies in ten chunks, its first bad slice in the second: none of its room is written
    total = S.expected(S.batches()["three"])["total"]
    rooms = [w["out_offset"] for w in S.expected(S.batches()["three"])["records"]]
    for cap, stages in ((total, [None, None, None]), (total - 1, [None, None, "cap"]), ((rooms[1] + rooms[2]) // 2, [None, "cap", "cap"]), (0, ["cap"] * 3)):
        assert [w["stage"] for w in S.expected(S.batches()["three"], cap=cap)["records"]] == stages
        run("three", "i420", "iso", cap=cap)


# ---- check() rejects, and names, single alterations ----
def _verdicts():
    batch = S.batches()["verdicts"]
    data, seg = S.place(batch, GAP, lead=1)
    recs, buf = S.host_decode_streams(data, seg)
    want = S.expected(batch)
    S.check(recs, buf, want, base=S.GUARD, segments=seg)
    return recs, buf, want, seg


def test_check_rejects_a_byte_in_a_refused_room():
    recs, buf, want, seg = _verdicts()
    w = want["records"][3]
    assert w["stage"] == "slice" and w["pictures"] * w["frame_bytes"] > 0
    buf = buf.copy()
    buf[S.GUARD + w["out_offset"] + 5] = 0
    with pytest.raises(AssertionError, match=r"stream 3 \(slice\): byte 5 of its room was written"):
        S.check(recs, buf, want, base=S.GUARD, segments=seg)


def test_check_rejects_an_out_offset_off_by_one():
    recs, buf, want, seg = _verdicts()
    recs = [dict(r) for r in recs]
    recs[4]["out_offset"] += 1
    with pytest.raises(AssertionError, match=r"stream 4: out_offset"):
        S.check(recs, buf, want, base=S.GUARD, segments=seg)


def test_check_rejects_an_absolute_err_offset():
    recs, buf, want, seg = _verdicts()
    recs = [dict(r) for r in recs]
    assert recs[3]["err_offset"] > 0 and seg[3][0] > 0
    recs[3]["err_offset"] += seg[3][0]
    with pytest.raises(AssertionError, match=r"stream 3 \(slice\): err_offset"):
        S.check(recs, buf, want, base=S.GUARD, segments=seg)


def test_check_rejects_two_records_swapped():
    recs, buf, want, seg = _verdicts()
    recs = list(recs)
    recs[0], recs[2] = recs[2], recs[0]
    with pytest.raises(AssertionError, match=r"stream 0: es_offset"):
        S.check(recs, buf, want, base=S.GUARD, segments=seg)
    with pytest.raises(AssertionError, match=r"stream 0: out_offset"):
        S.check(recs, buf, want, base=S.GUARD)


# ---- one textual change at a time in a copy of csrc/m2v_decode_kernels.hpp: each is caught by a named batch ----
# (the batch is the one whose first stream is the widest: with the change every read stays inside the chunk's buffer, so the altered
# library answers wrongly instead of faulting inside the test process)
MUTANTS = (
    ("locator_first_width", "r.at = out_locate(r.q, t[a].w, t[a].h, layout);", "r.at = out_locate(r.q, t[0].w, t[a].h, layout);", "mixed_reversed", "smallest"),
)


@pytest.mark.parametrize("name,old,new,caught_by,passes", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_batches_catch_mutants(tmp_path, name, old, new, caught_by, passes):
    text = open(os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc", "m2v_decode_kernels.hpp")).read()
    assert text.count(old) == 1, "the line this mutant changes is not there (once)"
    (tmp_path / "m2v_decode_kernels.hpp").write_text(text.replace(old, new))
    lib = S.build_host(str(tmp_path))
    run(caught_by, "i420", "iso")
    with pytest.raises(AssertionError):
        run(caught_by, "i420", "iso", lib=lib)
    if passes:                                  # ... and only by a batch that has what the change is about
        run(passes, "i420", "iso", lib=lib)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    B = S.batches()
    items = []
    for k, name in enumerate(sorted(B)):
        items.append((B[name], D.LAYOUTS[k & 3], ("iso", "module")[k & 1], None, 0))
    items += [(B["chunks"], "nv21", "iso", None, k) for k in (1, 2, 3, 5)]
    items += [(B["verdicts"], "nv12", "module", None, 2), (B["two_bad"], "i420", "iso", None, 7)]
    total = S.expected(B["three"])["total"]
    items += [(B["three"], "i420", "iso", cap, 0) for cap in (total, total - 1, total // 2, 0)]
    items += [([b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64)], "i420", "iso", None, 0)]
    path = tmp_path / "batches.bin"
    path.write_bytes(S.pack_batches(items))
    exe = str(tmp_path / "dec_host_streams_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    # the sanitizers' runtimes linked in: the program starts with whatever environment the test has
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-o", exe, os.path.join(D.ROOT, "tools", "dec_host_streams_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == sum(len(it[0]) + 1 for it in items)
    # the program's verdicts are the model's
    at = 0
    for k, (streams, layout, mode, cap, db) in enumerate(items):
        want = S.expected(streams, layout, mode, cap=cap)
        for b, w in enumerate(want["records"]):
            got = [int(v) for v in lines[at + b].split()]
            assert got[:4] == [k, b, w["status"], w["err_offset"]] and got[5] == w["out_offset"], (k, b, got, w)
        room = want["total"] if cap is None else cap
        if room <= 1 << 16:                      # ... and the small outputs' checksums (the output is exactly cap bytes, FILL where untouched)
            out = np.full(room, S.FILL, np.uint8)
            m = min(room, want["total"])
            out[:m] = want["out"][:m]
            total = 0
            for v in out.tolist():
                total = (total * 31 + v) & 0xFFFFFFFF
            assert lines[at + len(streams)] == "%d sum %08x" % (k, total), k
        at += len(streams) + 1
