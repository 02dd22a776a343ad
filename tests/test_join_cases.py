"""Streams cut from a broadcast (option "decode_join"), on the CPU: decoder.decode(..., join=) - the definition - and the g++ build of
the device's own functions (tools/dec_j_host.hpp over the j_ functions of csrc/m2v_decode_kernels.hpp) held to each other on every
stream of tests/join_cases.py - frames, record, join record, verdict and offset, planned in 256 ranges of events, in one, and in
numbers between - and both held to answers the new code did not make:
   I1  junk G without a sequence_header_code in front of S: join=1 on G + S is join=1 on S, every offset moved by len(G)
   I2  every stream the field-picture tests' option-off definition accepts: the same frames and record under join=1, join record (0, len, 0, 0)
   I3  S accepted without an end code, X a strict prefix of one further coded frame, cut at every byte: from the fourth byte of its
       picture start code on join=2 on S + X is option-off on S, tail_offset len(S); in front of that (the rule knows a frame by its
       picture start code: fewer bytes, or a GOP header alone, begin none) and on S itself it is option-off on S cut at its own T
   I4  with sequence_end_code, join=2 is option-off
   I5  join=1 on the part of A + S2 from S2's sequence header on: the frames option-off yields for A + S2 at the display positions of
       the kept pictures; dropped_leading stated as a literal
   I6  join=3 on full[c : len - d] for every c across one GOP and a dozen d: I1, I3 and I5 composed, from the writer's log
The refusals' offsets are stated by hand from the writer's log."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import join_cases as J

M, D, F = J.M, J.D, J.F
LANES = (256, 1, 2, 5, 37)


def frames_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for x, y in zip(a, b) for p, q in zip(x, y))


def agree(stream, b, join, lanes=(256,), layout="i420"):
    """the host build answers what the definition answers, planned in every number of ranges -> the definition's answer (None: refused)"""
    d, at = J.spec_cached(stream, b, join)
    for n in lanes:
        got, r, jr = J.host_decode(stream, b, join, layout, n)
        if d is None:
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at) and jr == (0, len(stream), 0, 0), (n, r, at, jr)
            continue
        assert got is not None, (n, r)
        want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
        assert got.shape == want.shape and np.array_equal(got, want), n
        rec = J.record_of(d, stream)
        assert {k: int(r[k]) for k in rec} == rec and jr == J.join_of(d, stream), (n, r, rec, jr)
    return d


def shifted(d, by):
    return (d.join_offset + by, d.tail_offset + by, d.dropped_leading, d.dropped_trailing)


def test_keyword_rules():
    s = J.open_cases()["i_p"][0]
    kw = dict(quirks=False, syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True)
    for missing in ("interlaced", "extended", "mb_tools", "field_pictures"):
        with pytest.raises(ValueError):
            M.decoder.decode(s, join=1, **dict(kw, **{missing: False}))
    with pytest.raises(ValueError):
        M.decoder.decode(s, join=4, **kw)
    with pytest.raises(ValueError):
        M.decoder.decode(s, join=1, **dict(kw, syntax="module", quirks=True))
    d = M.decoder.decode(s, join=0, **kw)
    assert not hasattr(d, "join_offset") and frames_equal(d.frames, F.spec_cached(s, True)[0].frames)


@pytest.mark.parametrize("name", sorted(J.junk()))
def test_i1_junk_in_front(name):
    g = J.junk()[name]
    for case in ("b_pair", "ip_anchor"):
        s, L, c, na, letters, dropped = J.open_cases()[case]
        s = s[c:]
        want = agree(s, True, 1, LANES)
        got = agree(g + s, True, 1, LANES)
        assert want is not None and frames_equal(got.frames, want.frames) and J.join_of(got, g + s) == shifted(want, len(g))
        assert got.dropped_leading == dropped and got.join_offset == len(g)
    # a refusal moves as well
    s, b, join, at = J.refusals()["dropped_b_same_parity"]
    base = len(J.junk()["random"])
    assert J.spec_cached(g + s[base:], b, join) == (None, at - base + len(g))
    agree(g + s[base:], b, join, LANES)


def test_i2_accepted_streams_keep_their_answer():
    for name, s, b in F.all_streams():
        d, at = F.spec_cached(s, b)
        if d is None:
            continue
        got = agree(s, b, 1, (256, 3) if len(s) < 20000 else (256,))
        assert got is not None and frames_equal(got.frames, d.frames) and J.record_of(got, s) == F.record_of(d, s) and J.join_of(got, s) == (0, len(s), 0, 0), name


@pytest.mark.parametrize("name", sorted(J.tail_base()[2]))
def test_i3_cut_at_every_byte(name):
    s, L, more = J.tail_base()
    x = more[name]
    want, _ = F.spec_cached(s, True)
    assert want is not None
    whole = x.find(b"\x00\x00\x01\x00") + 4                         # the frame's picture start code is whole from here on
    t = J.units(L, "picture")[2]
    cut, _ = F.spec_cached(s[:t], True)
    for n in range(1, whole):                                       # no picture start code yet (a GOP header alone begins no frame): the rule takes S's own last frame
        got = agree(s + x[:n], True, 2, (256, 2))
        assert frames_equal(got.frames, cut.frames) and J.join_of(got, s) == (0, t, 0, 1), n
    for n in range(whole, len(x)):                                  # every strict prefix that holds the picture start code
        got = agree(s + x[:n], True, 2, (256, 2))
        assert got is not None and frames_equal(got.frames, want.frames) and J.join_of(got, s) == (0, len(s), 0, 1), n
        assert J.record_of(got, s) == F.record_of(want, s)
    both = agree(J.junk()["lone_prefix"] + s + x[:len(x) // 2], True, 3, LANES)
    assert frames_equal(both.frames, want.frames) and J.join_of(both, s) == (3, 3 + len(s), 0, 1)


def test_i3_a_picture_header_cut_after_two_bytes():
    s, L, more = J.tail_base()
    want, _ = F.spec_cached(s, True)
    got = agree(s + more["frame_picture"][:6], True, 2, LANES)
    assert frames_equal(got.frames, want.frames) and J.join_of(got, s) == (0, len(s), 0, 1)
    # the stream itself under bit 2: option-off on the stream cut at its own T - the start of its last frame
    t = J.units(L, "picture")[2]
    cut, _ = F.spec_cached(s[:t], True)
    got = agree(s, True, 2, LANES)
    assert cut is not None and frames_equal(got.frames, cut.frames) and J.join_of(got, s) == (0, t, 0, 1) and len(got.frames) == 2


def test_i4_with_an_end_code_the_tail_is_kept():
    for name, (s, L, b) in sorted(F.cases().items()):
        assert s.endswith(b"\x00\x00\x01\xb7")
        d, _ = F.spec_cached(s, b)
        for join in (2, 3):
            got = agree(s, b, join, (256, 5))
            assert frames_equal(got.frames, d.frames) and J.join_of(got, s) == (0, len(s), 0, 0), (name, join)
    s, L, c, na, letters, dropped = J.open_cases()["b_pair"]
    got = agree(s[c:] + bytes(9), True, 3, LANES)                   # zeros behind the end code
    assert J.join_of(got, s) == (0, len(s) - c + 9, dropped, 0)


@pytest.mark.parametrize("name", sorted(J.open_cases()))
def test_i5_leading_b_pictures(name):
    s, L, c, na, letters, dropped = J.open_cases()[name]
    full, _ = F.spec_cached(s, True)
    assert [" IPB"[p["type"]] for p in full.pictures[na:]] == list(letters)
    got = agree(s[c:], True, 1, LANES)
    keep = J.kept_frames(letters)
    assert got is not None and got.dropped_leading == dropped == len(letters) - len(keep)
    want = [full.frames[k] for k in sorted(full.display[na + k] for k in keep)]
    assert frames_equal(got.frames, want) and J.join_of(got, s[c:]) == (0, len(s) - c, dropped, 0)
    # with the option 0 the stream is refused at the unit the parent names: its first leading B picture (or accepted: there is none)
    off, at = F.spec_cached(s[c:], True)
    first_b = [a - c for a, f in zip(J.units(L, "picture"), L["fields"]) if a >= c and f["type"] == 3][:1]
    assert (off is None and at == first_b[0]) if dropped else (off is not None and frames_equal(off.frames, got.frames))
    assert J.spec_cached(s[c:], True, 0)[1] == at
    # without "decode_b_pictures" a B picture is refused at its header as ever
    if "B" in letters:
        assert J.spec_cached(s[c:], False, 1) == (None, first_b[0]) and agree(s[c:], False, 1) is None


def test_i5_the_matrix_of_a_dropped_picture_holds():
    s, L, c, na, letters, dropped = J.open_cases()["matrix_in_a_dropped_b"]
    with_it, other = agree(s[c:], True, 1), agree(J.without_matrix(), True, 1)
    assert len(with_it.frames) == len(other.frames) == 3 and not frames_equal(with_it.frames[1:], other.frames[1:])


def test_i6_every_cut_across_a_gop():
    """full[c : len - d]: J is the first sequence header at or behind c, the leading B frames of its GOP go, and so does the frame the
    cut end lies in - all read off the writer's log, the frames off the option-off decode of the whole"""
    s, L, letters = J.three_gops()
    full, _ = F.spec_cached(s, True)
    seqs, pics = J.units(L, "sequence"), J.units(L, "picture")
    begins = [a for a, f in zip(pics, L["fields"]) if not f["second"]]           # the picture that begins each frame
    assert len(begins) == len(letters) == len(full.frames)
    heads = sorted(J.units(L, "gop") + pics)
    slices = J.units(L, "slice")
    ds = [1, 2, 3, 5, 17, 40, 41, 42, 43, 44, 90, 131]
    for c in list(range(seqs[0] + 1, seqs[1] + 1)) + [seqs[1] + 1, seqs[2] - 2]:
        j = min(a for a in seqs if a >= c)
        for d in ds if c % 9 == 0 or c in (seqs[1], seqs[1] + 1) else ds[c % 12:c % 12 + 1]:
            end = len(s) - d
            f = max(k for k, a in enumerate(begins) if a + 4 <= end)             # F: the last frame whose picture start code is whole
            last_slice = max(a for a in slices if a < begins[f])
            t = min(a for a in heads if a > last_slice)
            first = min(k for k, a in enumerate(begins) if a >= j)
            keep = [first + k for k in J.kept_frames(letters[first:f])]
            got = agree(s[c:end], True, 3, (256, 3))
            assert got is not None, (c, d)
            want = [full.frames[k] for k in sorted(full.display[k] for k in keep)]
            assert frames_equal(got.frames, want), (c, d)
            assert J.join_of(got, s) == (j - c, t - c, (f - first) - len(keep), 1), (c, d)


def test_refusals():
    cases = J.refusals()
    assert len(cases) >= 20
    for name, (s, b, join, want) in sorted(cases.items()):
        d = agree(s, b, join, LANES)
        if want is None:
            assert d is not None, name
        else:
            assert d is None and J.spec_cached(s, b, join)[1] == want, (name, J.spec_cached(s, b, join)[1], want)


@pytest.mark.parametrize("name", sorted(J.plan_streams()))
def test_plan_streams(name):
    s, b, join = J.plan_streams()[name]
    d = agree(s, b, join, LANES)
    assert d is not None and d.dropped_leading >= 2 and d.join_offset > 0
    if name == "long":
        assert len(d.frames) > 256
    if name.startswith("shift"):
        assert d.dropped_trailing == 1 and d.tail_offset < len(s)


def test_plan_streams_reach_every_position():
    """what the plan carries across range edges falls at every position of a range: from the start codes alone (join_cases.reached)"""
    R = {name: J.reached(*v) for name, v in J.plan_streams().items()}
    shift = [R["shift_%d" % k] for k in range(7)]
    assert all(r["per"] == 2 and r["per0"] == 2 for r in shift)
    for what in ("J", "E1", "E2", "F", "T"):
        assert {r[what] for r in shift} == {0, 1}, what
    wide = [R["wide_%d" % k] for k in range(3)]
    assert all(r["per"] == 3 for r in wide)
    for what in ("E1", "E2", "F", "T"):
        assert {r[what] for r in wide} == {0, 1, 2}, what
    assert all(r["dropped_pair_straddles"] for r in shift + wide)          # a field is three events: its partner lies in another range
    assert R["long"]["per"] == 7 and R["long"]["dropped_pair_inside"] and (R["long"]["E1"], R["long"]["E2"]) == (4, 5)
    assert R["long_junk"]["per0"] == 14 and R["long_junk"]["per"] == 3 and R["long_junk"]["J"] == 4      # J is searched in ranges of the whole list


def test_altered_streams():
    cases = J.altered()
    assert len(cases) == 300
    refused = sum(agree(x, True, 3, (256, 4)) is None for _, x in cases)
    assert 30 <= refused <= 270, refused


def test_sanitizers():
    """every stream of join_cases.all_streams() through tools/dec_j_host_check.cpp built with AddressSanitizer and UBSan: a stand-alone
    program, each stream in an allocation of exactly its size; its verdicts are the definition's"""
    streams = J.all_streams()
    root = D.ROOT
    d = tempfile.mkdtemp(prefix="m2v_dec_j_check_")
    exe, path = os.path.join(d, "dec_j_host_check"), os.path.join(d, "streams.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "fpga-mpeg2-encoder_amd", "csrc"),
                           "-I", os.path.join(root, "tools"), os.path.join(root, "tools", "dec_j_host_check.cpp"), "-o", exe])
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for name, s, b, join in streams:
            f.write(struct.pack("<IQ", int(bool(b)) | join << 1, len(s)) + bytes(s))
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == len(streams)
    for line, (name, s, b, join) in zip(lines[::5], streams[::5]):
        k, status, err, pictures, jo, to, dl, dt, _ = line.split()
        d_, at = J.spec_cached(s, b, join)
        if d_ is None:
            assert (int(status), int(err)) == (D.SYNTAX, at), name
        else:
            assert (int(status), int(pictures), int(jo), int(to), int(dl), int(dt)) == (D.OK, len(d_.frames)) + J.join_of(d_, s), name
