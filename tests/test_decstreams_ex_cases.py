"""A batch of main-syntax streams with the extended options per call, on the CPU: tools/dec_streams_ex_host.hpp's decode_streams - the
serial run of what m2v_decode_streams_ex.hip runs, plan_streams_main_ex included - against the model of tests/decstreams_ex_cases.py on
every batch: records, bytes and every byte that must stay untouched; plan_streams_main_ex against hand-stated tables for slice0,
pre_slices, the carried slots and bwd_off == fwd_off; every batch asserted, from the writers' logs and the model, to hold what its name
says; the host build once more under AddressSanitizer and UBSan as a stand-alone program; the header and EXPORTS.
tests/test_gpu_decode_streams_ex.py runs the same batches on the device."""
import os
import subprocess

import numpy as np
import pytest

import dec_cases as D
import decstreams_ex_cases as X

M = D.M
GAP = b"\x00\x00\x01"                      # between the segments: a prefix that would make a start code with a segment's first byte


def run(batch, flags=15, layout="i420", cap=None, decode_batch=0, level_bytes=0, placed=None):
    data, seg = placed or X.place(batch, GAP, lead=1)
    recs, buf = X.host_decode_streams(data, seg, flags, layout, cap=cap, decode_batch=decode_batch, level_bytes=level_bytes)
    want = X.expected(batch, flags, layout, cap=cap)
    X.check(recs, buf, want, base=X.GUARD, segments=seg)
    out = buf[X.GUARD:X.GUARD + want["total"]]
    assert ((out != X.FILL) <= want["written"]).all(), "a byte outside the rooms of OK streams was written"
    return recs, buf


def test_the_entry_is_declared_and_exported():
    hdr = open(os.path.join(D.ROOT, "include", "m2v_mi355x.h")).read()
    for word in ("m2v_decode_streams_main_ex_device", "M2V_DECS_EXTENDED = 4", "M2V_DECS_MB_TOOLS = 8"):
        assert word in hdr
    assert "m2v_decode_streams_main_ex_device" in M.EXPORTS
    assert (M.DECS_EXTENDED, M.DECS_MB_TOOLS) == (4, 8)
    import inspect
    p = inspect.signature(M.Mpeg2Encoder.decode_streams).parameters
    assert (p["extended"].default, p["mb_tools"].default) == (False, False)
    build = open(os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "build.py")).read()
    assert '"m2v_decode_streams_ex.hip"' in build and '"m2v_decode_streams_ex.hpp"' in build


@pytest.mark.parametrize("name", X.NAMES)
def test_host_build_equals_the_model(name):
    assert set(X.batches()) == set(X.NAMES)
    batch, flags = X.batches()[name]
    for layout in D.LAYOUTS if len(batch) < 40 else ("nv12",):
        run(batch, flags, layout)
    # the probe call reports the layout the decode has
    data, seg = X.place(batch, GAP, lead=1)
    recs, _ = X.host_decode_streams(data, seg, flags, probe=True)
    want = X.expected(batch, flags, probe=True)["records"]
    assert [(r["out_offset"], r["out_bytes"], r["status"]) for r in recs] == [(w["out_offset"], w["out_bytes"], w["status"]) for w in want]


def test_batches_hold_what_they_say():
    # tools: every valid case of both files is accepted under flags 15, beside plain streams of other sizes
    want = X.expected(X.tools(), 15)["records"]
    assert [w["stage"] for w in want] == [None] * len(X.tools()) and len(X.tools()) > len(X.XC.cases()) + len(X.TC.cases())
    assert len({(w["width"], w["height"]) for w in want}) >= 8 and (1, 1) in {(w["width"], w["height"]) for w in want}
    assert want[[w["frame_bytes"] for w in want].index(3) + 1]["out_offset"] % 2 == 1            # the stream behind a 1 x 1 one starts at an odd address
    # flags: under 4 .. 7 Table B-15, concealment vectors and dual prime's extension flags are probe refusals; the layouts differ
    mixed = X.mixed()
    st = {f: X.stages(mixed, f) for f in X.LEGAL_FLAGS}
    assert st[15] == [None] * len(mixed)
    for f in (4, 5, 6, 7):
        assert [st[f][k] for k in (7, 8, 10)] == ["probe"] * 3, f      # b15_mixed, cmv_ip, all_tools: at the coding extension
    assert st[7][9] == st[6][9] == "slice"                             # dual_flat: a motion type the option alone does not read, inside a slice
    offs = {f: tuple(w["out_offset"] for w in X.expected(mixed, f)["records"]) for f in X.LEGAL_FLAGS}
    assert len(set(offs.values())) >= 3 and len(set(offs.values())) == len(X.LEGAL_FLAGS)
    for f in (0, 1, 2, 3):                                             # below 4 the model is decstreams_main_cases'
        assert st[f] == X.X0.stages(mixed, f)
    # verdicts: the 30 + 24 hand-stated refusals, each between two good streams; both stages; continuity at the slice stage
    v = X.verdicts()
    assert len(X.XC.refusals()) == 30 and len(X.TC.refusals()) == 24 and len(v) == 2 * 54 + 1
    assert [what for what, _ in v][0::2] == ["good"] * 55
    got = dict(zip([what for what, _ in v], X.expected([s for _, s in v], 15)["records"]))
    assert got["good"]["stage"] is None
    for name, (s, b, i, at) in X.XC.refusals().items():
        w = got["ext_" + name]
        assert w["stage"] in ("probe", "slice") and w["err_offset"] == at, name
    for name, (s, b, i, t, at) in X.TC.refusals().items():
        w = got["mbt_" + name]
        if t:
            assert w["stage"] in ("probe", "slice") and w["err_offset"] == at, name
    for name in X.CONTINUITY:
        assert got[name]["stage"] == "slice", name
    assert {w["stage"] for w in got.values()} == {None, "probe", "slice"}
    got7 = dict(zip([what for what, _ in v], X.expected([s for _, s in v], 7)["records"]))
    for name in ("mbt_off_intra_vlc_format", "mbt_off_concealment", "mbt_off_both"):
        assert got7[name]["stage"] == "probe" and got7[name]["err_offset"] == X.TC.refusals()[name[4:]][4], name
    assert got7["mbt_off_dual_prime"]["stage"] == "slice" and got7["mbt_off_dual_prime"]["err_offset"] == X.TC.refusals()["off_dual_prime"][4]
    # chunks: one, two and three slices a row in turn - not rows x pictures -, a load, a reset, dual prime in every P picture
    s, L = X.chunk_stream()
    assert X.slices_of(s) == [3, 5, 4] * 3 and sum(X.slices_of(s)) != 2 * 9
    a = X.alone(s, 15)
    assert a["stage"] is None and [q["type"] for q in a["decoded"].pictures] == [" IPB".index(c) for c in X.CHUNK_LETTERS]
    assert a["repeated_headers"] == 1 and len([k for k, _ in L["units"] if k == "quant_matrix"]) == 1
    assert sorted({d[0] for d in L["duals"]}) == [1, 4, 7] and len(L["duals"]) == 12
    assert X.alone(s, 7)["stage"] == "slice"                           # (without the tools the first dual-prime macroblock is refused)
    # ... the matrices matter: the same stream without the extension, or without the reset, decodes to other frames
    frames = D.frames_of(a["decoded"], "i420")
    quant = [at for k, at in L["units"] if k == "quant_matrix"][0]
    nxt = [at for _, at in L["units"] if at > quant][0]
    twin = X.alone(s[:quant] + s[nxt:], 15)
    assert twin["stage"] is None
    other = D.frames_of(twin["decoded"], "i420")
    differs = [bool((frames[k] != other[k]).any()) for k in range(9)]
    assert differs[0] and any(differs[3:6]) and not any(differs[6:])   # in force five pictures on (display order), and gone behind the header
    # late: three pictures - three chunks at "decode_batch" 1 -, refused for continuity at the last slice
    (g1, x, g2), last = X.late()
    w = X.expected([g1, x, g2], 15)["records"]
    assert (w[1]["stage"], w[1]["err_offset"], w[1]["pictures"]) == ("slice", last, 3) and w[0]["stage"] is None and w[2]["stage"] is None
    assert X.slices_of(x) == [2, 2, 3]
    # long: 2 071 events, nine to a range
    for k in (1, 3):
        sl = X.long_batch()[k]
        assert len(X.decoder.start_codes(sl)) == 2071 and X.PC.per_of(2071) == 9
    assert X.stages(X.long_batch(), 15) == [None] * 5
    # many: one, two, three slices in turn
    many = X.many()
    assert len(many) == 1024 and [sum(X.slices_of(many[k])) for k in range(3)] == [1, 2, 3] and X.stages(many[:3], 13) == [None] * 3
    # alignment: the sixteen offsets, frame_bytes 3 and 1152 in turn, the second stream's row cut in two
    streams, data, seg = X.alignment()
    assert [a % 16 for a, _ in seg] == list(range(16))
    assert [w["frame_bytes"] for w in X.expected(streams, 15)["records"]] == [3, 1152] * 8 and X.slices_of(streams[1]) == [2, 2]
    for a, n in seg:
        assert data[a - 3:a] == b"\x00\x00\x01" and data[a + n - 2:a + n + 2] == b"\x00\x00\x01\xb3"
    # altered: on the model alone
    for kind, first in X.ALTERED:
        st = X.stages(X.altered(kind, first), 15)
        assert len(st) == 64 and st.count(None) >= 16 and st.count("slice") >= 16 and st.count("probe") >= 8, (kind, [st.count(k) for k in (None, "slice", "probe")])


# ---- plan_streams_main_ex against hand-stated tables: (first stream, its picture, pictures, slices, carry0_from, carry1_from) per chunk -
# slots 0 and 1 are the carried ones, 2 + k the chunk's k-th picture -, (slice0, fwd, bwd) per picture, slice0 per picture of the verdict
# pass, pre_slices ----
IPBBPBB = (1, 2, 3, 3, 2, 3, 3)
PLANS = {
    # two anchors in the first chunk, one in the second: its P picture is the chunk's first anchor and reads carried slot 1 TWICE
    "two_then_one": ([IPBBPBB], [(1, 2, 3, 1, 2, 3, 1)], 3,
                     [(0, 0, 3, 6, 2, 3), (0, 3, 3, 6, 1, 3), (0, 6, 1, 1, -1, -1)],
                     [(0, 0, 0), (1, 2, 2), (3, 2, 3), (0, 0, 1), (1, 1, 1), (3, 1, 3), (0, 0, 1)],
                     [0, 1, 3, 6, 7, 9, 12], 13),
    # every picture a chunk of its own: a chunk's slices are its picture's, and both B pictures have both anchors carried
    "one_each": ([(1, 2, 3, 3)], [(2, 3, 1, 2)], 1,
                 [(0, 0, 1, 2, -1, 2), (0, 1, 1, 3, 1, 2), (0, 2, 1, 1, -1, -1), (0, 3, 1, 2, -1, -1)],
                 [(0, 0, 0), (0, 1, 1), (0, 0, 1), (0, 0, 1)],
                 [0, 2, 5, 6], 8),
    # another stream behind the cut one in the same chunk
    "another_follows": ([(1, 2, 3), (1, 2)], [(2, 1, 3), (1, 2)], 2,
                        [(0, 0, 2, 3, 2, 3), (0, 2, 2, 4, -1, 3), (1, 1, 1, 2, -1, -1)],
                        [(0, 0, 0), (2, 2, 2), (0, 0, 1), (3, 0, 0), (0, 1, 1)],
                        [0, 2, 3, 6, 7], 9),
    # everything in one chunk: no verdict pass
    "one_chunk": ([(1, 2, 3), (1, 2)], [(1, 1, 1), (3, 3)], 0,
                  [(0, 0, 5, 9, -1, -1)],
                  [(0, 0, 0), (1, 2, 2), (2, 2, 3), (3, 0, 0), (6, 5, 5)],
                  [], 0),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_streams_main_ex_tables(name):
    types, nslices, decode_batch, chunks, refs, pre, pre_slices = PLANS[name]
    assert X.host_plan(types, nslices, decode_batch) == (chunks, refs, pre, pre_slices)
    # without the tools a P picture has no second reference: plan_streams_main's tables
    plain = X.host_plan(types, nslices, decode_batch, mb_tools=False)
    flat = [t for s in types for t in s]
    assert plain[0] == chunks and plain[2:] == (pre, pre_slices)
    assert plain[1] == [(s, f, 0 if t == 2 else b) for t, (s, f, b) in zip(flat, refs)]
    # one slice a picture: the references are plan_streams_main's (the existing entry's tables), but for a P picture's bwd
    import decstreams_main_cases as X0
    old = X0.host_plan(types, decode_batch)
    new = X.host_plan(types, [(1,) * len(s) for s in types], decode_batch, mb_tools=False)
    assert [(c[0], c[1], c[2], c[5], c[6]) for c in old[0]] == [(c[0], c[1], c[2], c[4], c[5]) for c in new[0]]
    assert [r[:2] for r in old[1]] == [r[1:] for r in new[1]]


def test_chunks_do_not_change_the_answer():
    """the chunks batch at "decode_batch" 1, 2, 3, 5 and the default.  Where the chunk stream's pictures fall is stated from the plan:
    at 1 every P picture is its chunk's first anchor with a carried reference and every B picture has both anchors carried; the
    matrices loaded at its first picture are used five chunks on"""
    types = [tuple(q["type"] for q in X.alone(s, 15)["decoded"].pictures) for s in X.chunks()]
    nsl = [tuple(X.slices_of(s)) for s in X.chunks()]
    assert types[1] == tuple(" IPB".index(c) for c in X.CHUNK_LETTERS)
    chunks, refs, pre, pre_slices = X.host_plan(types, nsl, 1)
    assert len(chunks) == sum(len(t) for t in types) and [c[3] for c in chunks[7:16]] == [3, 5, 4] * 3
    mine = refs[7:16]
    assert [r[1:] for r, t in zip(mine, types[1]) if t == 2] == [(1, 1)] * 3          # dual prime: both predictions from carried slot 1
    assert [r[1:] for r, t in zip(mine, types[1]) if t == 3] == [(0, 1)] * 4          # both anchors carried
    assert pre_slices == sum(sum(n) for n, t in zip(nsl, types) if len(t) > 1)
    results = []
    for k in X.DECODE_BATCHES:
        recs, buf = run(X.chunks(), 15, decode_batch=k)
        results.append(buf.tobytes())
    assert len(set(results)) == 1
    run(X.chunks(), 15, "nv12", decode_batch=3)
    run(X.chunks(), 15, "yv12", level_bytes=768 * 10)
    for k in (1, 2, 3):
        run([s for _, s in X.verdicts()], 15, "nv21", decode_batch=k)
        run(X.altered(*X.ALTERED[0]), 15, decode_batch=k)
        run(X.altered(*X.ALTERED[1]), 15, decode_batch=k)
    run(X.long_batch(), 15, "nv12", decode_batch=5)


def test_late_refusal_writes_nothing():
    """the stream lies in three chunks at "decode_batch" 1 and its last chunk holds the discontinuous slice: not one byte of its room
    is written, its neighbours are whole"""
    (batch, last) = X.late()
    for k in (1, 2, 0):
        recs, buf = run(batch, 15, decode_batch=k)
        assert (recs[1]["status"], recs[1]["err_offset"], recs[1]["out_bytes"]) == (D.SYNTAX, last, 0)
        assert recs[0]["status"] == recs[2]["status"] == D.OK


def test_cap():
    """four streams; cap one byte short of the third's room: it and the one behind it are OVERFLOW, the two in front are written"""
    batch = X.cap_batch()
    want = X.expected(batch, 15)
    total, offs = want["total"], [w["out_offset"] for w in want["records"]]
    for cap, st in ((total, [None] * 4), (offs[3] - 1, [None, None, "cap", "cap"]), (offs[3], [None, None, None, "cap"]), (offs[1], [None, "cap", "cap", "cap"]),
                    (0, ["cap"] * 4)):
        assert X.stages(batch, 15, cap=cap) == st
        recs, _ = run(batch, 15, cap=cap)
        assert [r["out_offset"] for r in recs] == offs


def test_alignment():
    streams, data, seg = X.alignment()
    for layout in D.LAYOUTS:
        run(streams, 15, layout, placed=(data, seg))
    run(streams, 4, placed=(data, seg))


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    Bt = X.batches()
    items = []
    for k, name in enumerate(("verdicts", "verdicts_7", "altered_ext", "altered_mbt", "chunks", "late", "tools", "flags_5", "flags_14", "long")):
        items.append((Bt[name][0], Bt[name][1], D.LAYOUTS[k & 3], None, 0))
    items += [(X.chunks(), 15, "nv21", None, k) for k in (1, 2, 3, 5)]
    items += [(Bt["verdicts"][0], 15, "nv12", None, 2), (X.late()[0], 15, "i420", None, 1)]
    items += [(X.altered(*a), 15, "yv12", None, 1) for a in X.ALTERED]
    want = X.expected(X.cap_batch(), 15)
    items += [(X.cap_batch(), 15, "i420", cap, 0) for cap in (want["total"], want["records"][3]["out_offset"] - 1, want["total"] // 2, 0)]
    items += [((b"", b"\x00\x00\x01", b"\x00\x00\x01\xb3", bytes(64)), f, "i420", None, 0) for f in (4, 7, 12, 15)]
    path = tmp_path / "batches.bin"
    path.write_bytes(X.pack_batches(items))
    exe = str(tmp_path / "dec_streams_ex_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    # the sanitizers' runtimes linked in: the program starts with whatever environment the test has
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "dec_streams_ex_host_check.cpp")])
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
