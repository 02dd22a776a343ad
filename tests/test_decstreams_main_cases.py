"""A batch of main-syntax streams per call on the CPU: tools/dec_streams_main_host.hpp's decode_streams - the serial run of what
m2v_decode_streams_main.hip runs, plan_streams_main included - against the model of tests/decstreams_main_cases.py on every batch:
records, bytes and every byte that must stay untouched; plan_streams_main against hand-stated tables for the carried slots; every batch
asserted, from the writers' logs and the model, to hold what its name says; the host build once more under AddressSanitizer and UBSan
as a stand-alone program; the header and EXPORTS.  tests/test_gpu_decode_streams_main.py runs the same batches on the device."""
import os
import subprocess

import numpy as np
import pytest

import dec_cases as D
import decstreams_main_cases as X

M = D.M
GAP = b"\x00\x00\x01"                      # between the segments: a prefix that would make a start code with a segment's first byte


def run(batch, flags=3, layout="i420", cap=None, decode_batch=0, level_bytes=0, placed=None):
    data, seg = placed or X.place(batch, GAP, lead=1)
    recs, buf = X.host_decode_streams(data, seg, flags, layout, cap=cap, decode_batch=decode_batch, level_bytes=level_bytes)
    want = X.expected(batch, flags, layout, cap=cap)
    X.check(recs, buf, want, base=X.GUARD, segments=seg)
    out = buf[X.GUARD:X.GUARD + want["total"]]
    assert ((out != X.FILL) <= want["written"]).all(), "a byte outside the rooms of OK streams was written"
    return recs, buf


def test_the_entry_is_declared_and_exported():
    hdr = open(os.path.join(D.ROOT, "include", "m2v_mi355x.h")).read()
    for word in ("m2v_decode_streams_main_device", "M2V_DECS_B_PICTURES = 1", "M2V_DECS_INTERLACED = 2"):
        assert word in hdr
    assert "m2v_decode_streams_main_device" in M.EXPORTS
    assert (M.DECS_B_PICTURES, M.DECS_INTERLACED) == (1, 2)
    import inspect
    p = inspect.signature(M.Mpeg2Encoder.decode_streams).parameters
    assert (p["syntax"].default, p["b_pictures"].default, p["interlaced"].default) == ("module", False, False)
    build = open(os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "build.py")).read()
    assert '"m2v_decode_streams_main.hip"' in build and '"m2v_decode_streams_main.hpp"' in build


@pytest.mark.parametrize("name", X.NAMES)
def test_host_build_equals_the_model(name):
    assert set(X.batches()) == set(X.NAMES)
    batch, flags = X.batches()[name]
    for layout in D.LAYOUTS if len(batch) < 100 else ("i420",):
        run(batch, flags, layout)
    # the probe call reports the layout the decode has
    data, seg = X.place(batch, GAP, lead=1)
    recs, _ = X.host_decode_streams(data, seg, flags, probe=True)
    want = X.expected(batch, flags, probe=True)["records"]
    assert [(r["out_offset"], r["out_bytes"], r["status"]) for r in recs] == [(w["out_offset"], w["out_bytes"], w["status"]) for w in want]


def test_batches_hold_what_they_say():
    mixed = X.mixed()
    want = X.expected(mixed, 3)["records"]
    assert [w["stage"] for w in want] == [None] * len(mixed)
    sizes = [(w["width"], w["height"]) for w in want]
    assert sizes[:6] == [(1, 1), (17, 33), (32, 32), (48, 48), (16, 16), (64, 64)]
    assert want[0]["frame_bytes"] == 3 and want[1]["out_offset"] % 2 == 1          # the next stream starts at an odd output address
    assert X.ipbbpbb()[1]["pictures"] == [1, 2, 3, 3, 2, 3, 3]
    # 48 x 48 not progressive: four slices a picture, and every macroblock of the P picture field-predicted with field DCT
    L = X.field48()[1]
    assert len(L["qcodes"][0]) == 4 and X.decoder.sequence_headers(X.field48()[0])[:2] == (48, 48)
    assert all(m["dct"] == 1 for m in L["ilmbs"]) and all(m["motion"] == "field" and m["dct"] == 1 for m in L["ilmbs"] if m["type"] == 2)
    assert sum(m["type"] == 2 for m in L["ilmbs"]) == 12
    assert len(X.I.cases()["ipb_16"][1]["qcodes"][0]) == 2                          # 16 lines, two slices
    P = X.params_streams()
    assert {p[3] for p in P["alternate_scan"][1]["params"]} == {1} and {p[2] for p in P["q_scale_type"][1]["params"]} == {1}
    assert [p[1] for p in P["precisions"][1]["params"]] == [0, 3]
    assert any(k > 1 for k in P["f_code_3"][1]["incrs"]) and P["f_code_3"][1]["params"][1][0][:2] == (3, 3)
    assert want[12]["repeated_headers"] == 1
    a, b = (X.alone(bytes(P[k][0]), 3)["decoded"].sequence for k in ("matrix_a", "matrix_b"))
    assert list(a["intra_matrix"]) != list(b["intra_matrix"]) and list(a["non_intra_matrix"]) != list(b["non_intra_matrix"])
    # the flags: a B picture / frame_pred_frame_dct 0 is a probe-stage refusal without its flag, and the offsets behind shift
    for f in X.ALL_FLAGS:
        refused = {k for k in range(len(mixed)) if (k in X.MIXED_B and not f & 1) or (k in X.MIXED_FIELD and not f & 2)}
        st = X.stages(mixed, f)
        assert {k for k, s in enumerate(st) if s == "probe"} == refused and set(st) <= {None, "probe"}, f
    offs = {f: [w["out_offset"] for w in X.expected(mixed, f)["records"]] for f in X.ALL_FLAGS}
    assert len({tuple(v) for v in offs.values()}) == 4
    # the verdicts
    for (what, s), w in zip(X.verdicts(), X.expected([s for _, s in X.verdicts()], 3)["records"]):
        if what in X.VERDICT_STAGES:
            assert w["stage"] == X.VERDICT_STAGES[what], what
        else:
            assert w["stage"] in ("probe", "slice"), what
    assert X.alone(bytes(X.B.refusals()["backward_vector_outside"][0]), 3)["err_offset"] == X.B.refusals()["backward_vector_outside"][1]
    assert X.alone(bytes(X.I.refusals()["field_vector_left_0"][0]), 3)["err_offset"] == X.I.refusals()["field_vector_left_0"][2]
    # the altered streams: every kind of verdict in either batch
    for seed in X.ALTERED_SEEDS:
        assert len(X.altered(seed)) == 64 and set(X.stages(X.altered(seed), 3)) == {None, "probe", "slice"}
    # late: three chunks at "decode_batch" 2 and more, refused at its last slice
    (g1, x, g2), last = X.late()
    w = X.expected([g1, x, g2], 3)["records"][1]
    assert (w["stage"], w["err_offset"], w["pictures"]) == ("slice", last, 7)
    # events: more start codes than the first guess
    s = X.events()[0]
    assert len(X.decoder.start_codes(s)) > X.event_guess(len(s)) and X.alone(s, 0)["pictures"] == 300
    # many: every 64th stream has four pictures, I P B B
    many = X.many()
    assert len(many) == 4096 and [X.alone(many[k], 1)["pictures"] for k in (0, 62, 63, 64, 4095)] == [1, 1, 4, 1, 4]
    # alignment: the sixteen offsets, frame_bytes 3 and 384 in turn
    streams, data, seg = X.alignment()
    assert [a % 16 for a, _ in seg] == list(range(16))
    assert [w["frame_bytes"] for w in X.expected(streams, 3)["records"]] == [3, 384] * 8
    for a, n in seg:
        assert data[a - 3:a] == b"\x00\x00\x01" and data[a + n - 2:a + n + 2] == b"\x00\x00\x01\xb3"


# ---- plan_streams_main against hand-stated tables: (first stream, its picture, pictures, anchor steps, B pictures, carry0_from,
# carry1_from) per chunk - slots 0 and 1 are the carried ones, 2 + k the chunk's k-th picture - and (fwd, bwd, display) per picture ----
IPBBPBB = (1, 2, 3, 3, 2, 3, 3)
PLANS = {
    # two anchors in the first chunk, one in the second (slot 1 moves to slot 0, the new anchor to slot 1), none in the third
    "two_then_one": ([IPBBPBB], 3,
                     [(0, 0, 3, 2, 1, 2, 3), (0, 3, 3, 1, 2, 1, 3), (0, 6, 1, 0, 1, -1, -1)],
                     [(0, 0, 0), (2, 0, 3), (2, 3, 1), (0, 1, 2), (1, 0, 6), (1, 3, 4), (0, 1, 5)]),
    # a chunk of B pictures alone between its anchors and the next P picture: nothing moves behind it
    "zero_anchors": ([IPBBPBB], 2,
                     [(0, 0, 2, 2, 0, 2, 3), (0, 2, 2, 0, 2, -1, -1), (0, 4, 2, 1, 1, 1, 2), (0, 6, 1, 0, 1, -1, -1)],
                     [(0, 0, 0), (2, 0, 3), (0, 1, 1), (0, 1, 2), (1, 0, 6), (1, 2, 4), (0, 1, 5)]),
    # another stream behind the cut one in the same chunk: it starts without anchors, and only its own I picture is carried on
    "another_follows": ([(1, 2, 3), (1, 2)], 2,
                        [(0, 0, 2, 2, 0, 2, 3), (0, 2, 2, 1, 1, -1, 3), (1, 1, 1, 1, 0, -1, -1)],
                        [(0, 0, 0), (2, 0, 2), (0, 1, 1), (0, 0, 0), (1, 0, 1)]),
    # every picture a chunk of its own: anchors carried across two cuts
    "one_each": ([(1, 2, 3, 3)], 1,
                 [(0, 0, 1, 1, 0, -1, 2), (0, 1, 1, 1, 0, 1, 2), (0, 2, 1, 0, 1, -1, -1), (0, 3, 1, 0, 1, -1, -1)],
                 [(0, 0, 0), (1, 0, 3), (0, 1, 1), (0, 1, 2)]),
    # everything in one chunk: no carried slot is read
    "one_chunk": ([(1, 2, 3), (1, 2)], 0,
                  [(0, 0, 5, 2, 1, -1, -1)],
                  [(0, 0, 0), (2, 0, 2), (2, 3, 1), (0, 0, 0), (5, 0, 1)]),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_streams_main_carried_slots(name):
    types, decode_batch, chunks, refs = PLANS[name]
    assert X.host_plan(types, decode_batch) == (chunks, refs)


def test_plan_display_is_the_definitions():
    for letters in ("IPBBPBB", "IPBPBBBP", "IPPBIBBP", "IPBBI", "I", "IPP"):
        types = tuple(" IPB".index(c) for c in letters)
        assert [r[2] for r in X.host_plan([types], 0)[1]] == X.decoder.display_order(list(types))
    assert [r[2] for r in X.host_plan([(1, 2, 2)], 0, b_pictures=False)[1]] == [0, 1, 2]


def test_chunks_do_not_change_the_answer():
    """the chunks batch at "decode_batch" 1, 2, 3, 5 and the default: anchors carried across one and two cuts, a cut between an anchor and
    its B pictures, a chunk of B pictures alone, another stream behind a cut one - where each setting cuts is stated here"""
    types = list(X.CHUNK_TYPES)
    assert [tuple(q["type"] for q in X.alone(s, 3)["decoded"].pictures) for s in X.chunks()] == types
    flat = [(b, p) for b, t in enumerate(types) for p in range(len(t))]
    for k in (1, 2, 3, 5):
        got = X.host_plan(types, k)[0]
        assert [c[:3] for c in got] == [flat[a] + (min(k, len(flat) - a),) for a in range(0, len(flat), k)]
    two = X.host_plan(types, 2)[0]
    assert two[1][:5] == (0, 2, 2, 0, 2)           # B pictures alone, cut off from both anchors
    assert two[3][:3] == (0, 6, 2) and two[3][3:5] == (1, 1)      # the cut stream's last B picture, then another stream's I picture
    assert X.host_plan(types, 0)[0] == [(0, 0, 15, 3, 4, -1, -1)]
    results = []
    for k in X.DECODE_BATCHES:
        recs, buf = run(X.chunks(), 3, decode_batch=k)
        results.append(buf.tobytes())
    assert len(set(results)) == 1
    run(X.chunks(), 3, "nv12", decode_batch=3)
    run(X.chunks(), 3, "yv12", level_bytes=768 * 10)
    for k in (1, 2, 3):
        run([s for _, s in X.verdicts()], 3, "nv21", decode_batch=k)
        run(X.altered(X.ALTERED_SEEDS[0]), 3, decode_batch=k)


def test_late_refusal_writes_nothing():
    """the stream lies in four chunks at "decode_batch" 2 and is refused in its last slice: not one byte of its room is written"""
    (batch, last) = X.late()
    for k in (2, 1, 0):
        recs, buf = run(batch, 3, decode_batch=k)
        assert (recs[1]["status"], recs[1]["err_offset"], recs[1]["out_bytes"]) == (D.SYNTAX, last, 0)


def test_cap():
    """four streams; cap one byte short of the third's room: it and the one behind it are OVERFLOW, the two in front are written; the
    probe call reports the same layout"""
    batch = X.cap_batch()
    want = X.expected(batch, 3)
    total, offs = want["total"], [w["out_offset"] for w in want["records"]]
    for cap, st in ((total, [None] * 4), (offs[3] - 1, [None, None, "cap", "cap"]), (offs[3], [None, None, None, "cap"]), (offs[1], [None, "cap", "cap", "cap"]),
                    (0, ["cap"] * 4)):
        assert X.stages(batch, 3, cap=cap) == st
        recs, _ = run(batch, 3, cap=cap)
        assert [r["out_offset"] for r in recs] == offs


def test_alignment():
    streams, data, seg = X.alignment()
    for layout in D.LAYOUTS:
        run(streams, 3, layout, placed=(data, seg))
    run(streams, 0, placed=(data, seg))


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    Bt = X.batches()
    items = []
    for k, name in enumerate(sorted(Bt)):
        items.append((Bt[name][0], Bt[name][1], D.LAYOUTS[k & 3], None, 0))
    items += [(X.chunks(), 3, "nv21", None, k) for k in (1, 2, 3, 5)]
    items += [(Bt["verdicts"][0], 3, "nv12", None, 2), (X.late()[0], 3, "i420", None, 2), (X.altered(X.ALTERED_SEEDS[1]), 3, "yv12", None, 1)]
    want = X.expected(X.cap_batch(), 3)
    items += [(X.cap_batch(), 3, "i420", cap, 0) for cap in (want["total"], want["records"][3]["out_offset"] - 1, want["total"] // 2, 0)]
    items += [((b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64)), f, "i420", None, 0) for f in X.ALL_FLAGS]
    path = tmp_path / "batches.bin"
    path.write_bytes(X.pack_batches(items))
    exe = str(tmp_path / "dec_streams_main_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    # the sanitizers' runtimes linked in: the program starts with whatever environment the test has
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_streams_main_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == sum(len(it[0]) + 1 for it in items)
    at = 0
    for k, (streams, flags, layout, cap, db) in enumerate(items):
        want = X.expected(streams, flags, layout, cap=cap)
        for b, w in enumerate(want["records"]):
            got = [int(v) for v in lines[at + b].split()]
            assert got[:4] == [k, b, w["status"], w["err_offset"]] and got[5] == w["out_offset"], (k, b, got, w)
        room = want["total"] if cap is None else cap
        if room <= 1 << 16:                      # ... and the small outputs' checksums (the output is exactly cap bytes, FILL where untouched)
            out = np.full(room, X.FILL, np.uint8)
            m = min(room, want["total"])
            out[:m] = want["out"][:m]
            total = 0
            for v in out.tolist():
                total = (total * 31 + v) & 0xFFFFFFFF
            assert lines[at + len(streams)] == "%d sum %08x" % (k, total), k
        at += len(streams) + 1
