"""-m gpu: m2v_decode_device with option "decode_join" = 0 .. 3 (on "decode_syntax" = main and "decode_interlaced", "decode_extended",
"decode_mb_tools", "decode_field_pictures" = 1, "decode_b_pictures" 0 or 1 as the case says) against decoder.decode(..., field_pictures=True,
join=...) - byte for byte, record for record, join record for join record, err_offset for err_offset; no tolerance anywhere.  The
streams are those of tests/join_cases.py at their smallest shapes; tests/test_join_cases.py runs them through the host build of the same
functions and shows by identities that the definition's answers are right.  Every decode writes into a buffer of FILL with guards
around the frames and a capacity of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM = -1
MAIN = 1
NEEDS = ("decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures")


@pytest.fixture(scope="module")
def env():
    import join_cases
    return join_cases.M, join_cases.D, join_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, J = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    for name in NEEDS:
        e.set_option(name, 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def join_record(enc):
    r = enc.decode_join_report()
    assert not r["reserved"].any()
    return tuple(int(r[k]) for k in ("join_offset", "tail_offset", "dropped_leading", "dropped_trailing"))


def decode(M, D, enc, stream, b, join, layout="i420", es_off=0, dst_off=0):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record,
    join record); asserts the guards, that the probe's layout is the decode's, and with a status other than OK that nothing was written"""
    import torch
    enc.set_option("decode_b_pictures", int(bool(b)))
    enc.set_option("decode_join", int(join))
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    torch.cuda.synchronize()                                        # (the stream is in place before the handle's own HIP stream reads it)
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES["iso"], None) == 0
    r0, j0 = enc.decode_report(), join_record(enc)
    room = int(r0["pictures"]) * int(r0["frame_bytes"]) if r0["status"] == D.OK else 4096
    buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES["iso"], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r, j = enc.decode_report(), join_record(enc)
    assert not r["reserved"].any()
    got = buf.cpu().numpy()
    a, b_ = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    assert (got[:a] == D.FILL).all() and (got[b_:] == D.FILL).all(), "bytes outside the frames were written"
    assert (r0["status"], r0["err_offset"]) == (r["status"], r["err_offset"]) or r0["status"] == D.OK      # (the probe stops behind the plan)
    if r0["status"] == D.OK:
        assert (int(r0["pictures"]), int(r0["frame_bytes"]), int(r0["out_bytes"])) == (int(r["pictures"]), int(r["frame_bytes"]), room)
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0 and j == (0, len(stream), 0, 0)
        return None, r, j
    assert j0 == j
    return got[a:b_].reshape(int(r["pictures"]), int(r["frame_bytes"])), r, j


def agree(env, enc, stream, b, join, layout="i420", **kw):
    """the device answers what the definition answers"""
    M, D, J = env
    d, at = J.spec_cached(bytes(stream), b, join) if join else J.F.spec_cached(bytes(stream), b)
    got, r, j = decode(M, D, enc, stream, b, join, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = J.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    assert j == J.join_of(d, stream), (j, J.join_of(d, stream))
    return d


def open_names():
    import join_cases
    return sorted(join_cases.open_cases())


@pytest.mark.parametrize("name", open_names())
def test_open_gops(env, enc, name):
    """I5's streams under all four values of the option, the layouts going round, at a source and a destination that are not aligned;
    the option-off call on the same handle in front and behind gives the parent's answer"""
    M, D, J = env
    k = open_names().index(name)
    s, L, c, na, letters, dropped = J.open_cases()[name]
    cut = s[c:]
    off = agree(env, enc, cut, True, 0)
    assert (off is None) == (dropped > 0)
    for join in (1, 2, 3):
        d = agree(env, enc, cut, True, join, D.LAYOUTS[(k + join) & 3], es_off=(k + join) % 5, dst_off=(3 * k + join) % 7)
        if join == 2 and dropped:
            assert d is None                                        # the tail alone: the leading B pictures stay refused
        else:
            assert d is not None and d.dropped_leading == (dropped if join & 1 else 0)
    assert agree(env, enc, s, True, 3, D.LAYOUTS[k & 3], es_off=1) is not None      # the whole: J is 0, A's frames are there
    if "B" in letters:
        assert agree(env, enc, cut, False, 1) is None                # without "decode_b_pictures" a B picture is refused as ever
    assert (agree(env, enc, cut, True, 0) is None) == (dropped > 0)


def test_junk_in_front(env, enc):
    """I1's junk in front of an open GOP: bit 1 and both bits; the slices' junk makes a fresh handle's event list grow"""
    M, D, J = env
    s, L, c, na, letters, dropped = J.open_cases()["b_pair"]
    for k, (name, g) in enumerate(sorted(J.junk().items())):
        d = agree(env, enc, g + s[c:], True, 1 + 2 * (k & 1), D.LAYOUTS[k & 3], es_off=k % 3, dst_off=k % 5)
        assert d is not None and d.join_offset == len(g) and d.dropped_leading == dropped, name
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        e.set_option("decode_syntax", MAIN)
        for n in NEEDS:
            e.set_option(n, 1)
        stream, b, join = J.plan_streams()["long_junk"]
        assert len(M.decoder.start_codes(stream)) > max(1024, len(stream) // 16 + 64)      # more events than the list's first size
        assert agree(env, e, stream, b, join) is not None
    finally:
        e.close()


def test_tails(env, enc):
    """I3 at a few cuts of each further frame (a picture header cut after two bytes among them); I2 and I4 on every valid stream of
    the field-picture tests"""
    M, D, J = env
    s, L, more = J.tail_base()
    for k, (name, x) in enumerate(sorted(more.items())):
        first = x.find(b"\x00\x00\x01\x00") + 4
        for n in sorted({4, first, first + 2, len(x) // 2, len(x) - 1}):
            d = agree(env, enc, s + x[:n], True, 2, D.LAYOUTS[(k + n) & 3], dst_off=n % 7)
            assert d is not None and d.dropped_trailing == 1
            assert d.tail_offset == (len(s) if n >= first else J.units(L, "picture")[2])
    assert agree(env, enc, s, True, 2).tail_offset == J.units(L, "picture")[2]
    for k, (name, (t, tl, b)) in enumerate(sorted(J.F.cases().items())):      # I2 and I4: the field-picture tests' streams keep their answer
        want = J.F.spec_cached(t, b)[0]
        for join in (1, 2, 3):
            d = agree(env, enc, t, b, join, D.LAYOUTS[(k + join) & 3])
            assert d is not None and len(d.frames) == len(want.frames) and J.join_of(d, t) == (0, len(t), 0, 0), (name, join)


def test_every_cut_across_a_gop(env, enc):
    """I6 at every seventh cut in front and four behind"""
    M, D, J = env
    s, L, letters = J.three_gops()
    seqs = J.units(L, "sequence")
    for c in list(range(seqs[0] + 1, seqs[1] + 1, 7)) + [seqs[1], seqs[1] + 1]:
        for d in (1, 17, 43, 131)[c % 4:c % 4 + 2]:
            assert agree(env, enc, s[c:len(s) - d], True, 3, D.LAYOUTS[c & 3], es_off=c % 3) is not None


def test_refusals(env, enc):
    """the status, the offset stated by hand, nothing written, the join record 0, es_bytes, 0, 0"""
    M, D, J = env
    for name, (s, b, join, want) in sorted(J.refusals().items()):
        d = agree(env, enc, s, b, join)
        if want is None:
            assert d is not None, name
        else:
            got, r, j = decode(M, D, enc, s, b, join)
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def plan_names():
    import join_cases
    return sorted(join_cases.plan_streams())


@pytest.mark.parametrize("name", plan_names())
def test_plan_streams(env, enc, name):
    """more than 256 events behind J, J, F, T, the anchors and the dropped pairs at every position of a range; more than 256 kept
    frames; junk longer than the event list's first size"""
    M, D, J = env
    s, b, join = J.plan_streams()[name]
    assert agree(env, enc, s, b, join, es_off=len(name) % 4) is not None


def test_altered_streams(env, enc):
    """every altered stream: the definition's verdict, its earliest offset, its frames where it accepts - never a fault"""
    M, D, J = env
    cases = J.altered()
    assert len(cases) == 300
    refused = sum(agree(env, enc, x, True, 3) is None for _, x in cases)
    assert 30 <= refused <= 270


def test_decode_batch(env, enc):
    """"decode_batch" 1, 2 and 3 (frames): the kept frames alone fill the chunks"""
    M, D, J = env
    try:
        for batch in (1, 2, 3):
            enc.set_option("decode_batch", batch)
            for name in ("b_pair", "cut_rows", "matrix_in_a_dropped_b", "ip_anchor"):
                s, L, c, na, letters, dropped = J.open_cases()[name]
                assert agree(env, enc, s[c:], True, 3, "nv12" if batch & 1 else "yv12", dst_off=batch) is not None
            s, b, join = J.plan_streams()["shift_%d" % batch]
            assert agree(env, enc, s, b, join) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_rules_of_the_option(env):
    """a value outside 0 .. 3 is M2V_E_PARAM; the option without one of the four options it needs, with the module syntax or with the
    module's mode is M2V_E_PARAM, names the option and writes nothing"""
    import torch
    M, D, J = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_join", 4) == E_PARAM and L.m2v_set_option(h, b"decode_join", -1) == E_PARAM
        s, log, c, na, letters, dropped = J.open_cases()["b_pair"]
        es = dev(s[c:])
        buf = torch.full((1 << 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
        e.set_option("decode_join", 3)
        call = lambda mode: L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES[mode], None)
        assert call("iso") == E_PARAM and b"decode_join" in L.m2v_last_error(h)                    # the module syntax
        e.set_option("decode_syntax", MAIN)
        e.set_option("decode_b_pictures", 1)
        for missing in NEEDS + (None,):
            for n in NEEDS:
                e.set_option(n, int(n != missing))
            if missing is not None:
                assert call("iso") == E_PARAM and b"decode_join" in L.m2v_last_error(h), missing
        assert call("module") == E_PARAM and b"decode_join" in L.m2v_last_error(h)                 # the module's mode
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all()
        assert call("iso") == 0 and e.decode_report()["status"] == D.OK and join_record(e) == (0, len(s) - c, dropped, 0)
        e.set_option("decode_join", 0)
        assert call("iso") == 0
        r = e.decode_report()
        first_b = [a - c for a, f in zip(J.units(log, "picture"), log["fields"]) if a >= c and f["type"] == 3][0]
        assert (r["status"], r["err_offset"]) == (D.SYNTAX, first_b) and join_record(e) == (0, len(s) - c, 0, 0)
    finally:
        e.close()


def test_decode_device_keyword(env):
    """decode_device(..., join=) takes 0 .. 3 or a name, puts the option back, and raises ValueError without field_pictures"""
    M, D, J = env
    s, L, c, na, letters, dropped = J.open_cases()["cut_rows"]
    cut = s[c:]
    d, _ = J.spec_cached(cut, True, 3)
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        kw = dict(syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True)
        for join in ("both", 3):
            got, r = e.decode_device(dev(cut), join=join, **kw)
            assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames) and join_record(e) == J.join_of(d, cut)
            assert e._set.get("decode_join", 0) == 0
        got, r = e.decode_device(dev(cut), join="head", **kw)
        assert r["pictures"] == len(J.spec_cached(cut, True, 1)[0].frames)
        with pytest.raises(M.M2VError, match="M2V_DEC_SYNTAX"):               # the option is back: the parent's answer
            e.decode_device(dev(cut), **kw)
        with pytest.raises(ValueError):
            e.decode_device(dev(cut), join="both", **dict(kw, field_pictures=False))
        with pytest.raises(ValueError):
            e.decode_device(dev(cut), join="middle", **kw)
        e.set_option("decode_join", 1)
        with pytest.raises(M.M2VError, match="M2V_DEC_SYNTAX"):               # join=0 decodes without it, whatever the handle holds
            e.decode_device(dev(cut), **kw)
        assert e._set["decode_join"] == 1                                      # and puts it back
    finally:
        e.close()


def test_from_a_recorded_transport_stream(env):
    """end to end: a transport stream from tests/demux_writer.py around an open-GOP stream, cut at packet boundaries in front and
    behind, through decode_device(container="ts", join="both") against decoder.decode(..., join=3) on the stream the CPU
    demultiplexer extracts (handed on with the zero padding to a whole 32-byte word, as decode_device hands it on)"""
    M, D, J = env
    import demux_writer as X
    s, L, letters = J.three_gops()
    w = X.TsWriter(11, video_pid=0x120)
    w.psi(0, X.pat_section([(1, 0x1000)]))
    w.psi(0x1000, X.pmt_section(1, 0x120, [(0x02, 0x120, b"")]))
    for n, at in enumerate(range(0, len(s), 100)):                  # a PES packet every 100 bytes: none begins where a picture does
        head = X.pes_header(0xE0, 0, pts=9000 + 3600 * n, dts=None)
        w.video(head + s[at:at + 100], pusi=1, head=len(head), stamp=(9000 + 3600 * n, X.ABSENT))
        if n % 3 == 0:
            w.null()
    ts = w.bytes()
    assert len(ts) % 188 == 0 and w.expect()["es"] == s
    packets = len(ts) // 188
    cut = ts[:2 * 188] + ts[4 * 188:(packets - 1) * 188]            # the tables, then the recording: it begins and ends inside a picture
    es = M.container.demux_ts(cut)[0]
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        assert es != s and es in s and not s.startswith(es) and not s.endswith(es)
        padded = es + bytes(-len(es) % 32)
        d, at = J.spec_cached(padded, True, 3)
        assert d is not None and d.join_offset == J.units(L, "sequence")[1] - s.find(es) > 0 and d.dropped_leading == 2 and d.dropped_trailing == 1 and len(d.frames) >= 4
        got, r = e.decode_device(dev(cut), container="ts", syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True, join="both")
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames) and join_record(e) == J.join_of(d, padded)
    finally:
        e.close()
