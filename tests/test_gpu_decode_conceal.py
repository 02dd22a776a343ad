"""-m gpu: m2v_decode_device with option "decode_conceal" = 1 (on "decode_syntax" = main and "decode_interlaced", "decode_extended",
"decode_mb_tools", "decode_field_pictures" = 1, "decode_b_pictures" 0 or 1 as the case says, "decode_join" 0 .. 3) against
decoder.decode(..., field_pictures=True, join=..., conceal=True) - byte for byte, record for record, report for report; no tolerance
anywhere.  The streams are those of tests/conceal_cases.py at their smallest shapes; tests/test_conceal_cases.py runs them through the
host build of the same functions and shows by twins, a numpy splice and literals that the definition's answers are right.  Every
decode writes into a buffer of FILL with guards around the frames and a capacity of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM = -1
MAIN = 1
NEEDS = ("decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures")
FIELDS = ("first_offset", "bad_slices", "concealed_rows", "grey_rows", "damaged_pictures")


@pytest.fixture(scope="module")
def env():
    import conceal_cases
    return conceal_cases.M, conceal_cases.D, conceal_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, C = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    for name in NEEDS:
        e.set_option(name, 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def report(enc):
    r = enc.decode_conceal_report()
    assert not r["reserved"].any()
    return tuple(int(r[k]) for k in FIELDS)


def join_record(enc):
    r = enc.decode_join_report()
    return tuple(int(r[k]) for k in ("join_offset", "tail_offset", "dropped_leading", "dropped_trailing"))


def decode(M, D, enc, stream, b, join, conceal, layout="i420", es_off=0, dst_off=0, batch=0):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record,
    join record, report); asserts the guards, and with a status other than OK that nothing was written and the report is of zeros"""
    import torch
    enc.set_option("decode_b_pictures", int(bool(b)))
    enc.set_option("decode_join", int(join))
    enc.set_option("decode_conceal", int(conceal))
    enc.set_option("decode_batch", int(batch))
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    torch.cuda.synchronize()                                        # (the stream is in place before the handle's own HIP stream reads it)
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES["iso"], None) == 0
    r0 = enc.decode_report()
    assert report(enc) == (len(stream), 0, 0, 0, 0)                 # (a probe walks nothing)
    room = int(r0["pictures"]) * int(r0["frame_bytes"]) if r0["status"] == D.OK else 4096
    buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES["iso"], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r, j, c = enc.decode_report(), join_record(enc), report(enc)
    assert not r["reserved"].any()
    got = buf.cpu().numpy()
    a, b_ = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    assert (got[:a] == D.FILL).all() and (got[b_:] == D.FILL).all(), "bytes outside the frames were written"
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0 and c == (len(stream), 0, 0, 0, 0)
        return None, r, j, c
    return got[a:b_].reshape(int(r["pictures"]), int(r["frame_bytes"])), r, j, c


def agree(env, enc, stream, b, join=0, conceal=1, layout="i420", **kw):
    """the device answers what the definition answers"""
    M, D, C = env
    d, at = C.spec_cached(bytes(stream), b, join, bool(conceal))
    got, r, j, c = decode(M, D, enc, stream, b, join, conceal, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = C.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    assert c == C.report_of(d, stream), (c, C.report_of(d, stream))
    assert j == C.J.join_of(d, stream), (j, C.J.join_of(d, stream))
    return d


def case_names():
    import conceal_cases
    return conceal_cases.gpu_subset()


@pytest.mark.parametrize("name", case_names())
def test_damaged_streams(env, enc, name):
    """every kind of damage: refused with the option off, concealed with it on - the report the literal of the case -, refused again; the
    layouts going round, a source and a destination that are not aligned, "decode_batch" 1, 2, 3 and the default"""
    M, D, C = env
    c = C.cases()[name]
    k = case_names().index(name)
    off = agree(env, enc, c["stream"], c["b"], 0, 0)
    assert off is None                                              # the parent's answer: M2V_DEC_SYNTAX at the unit the definition names
    d = agree(env, enc, c["stream"], c["b"], 0, 1, D.LAYOUTS[k & 3], es_off=k % 5, dst_off=(3 * k) % 7, batch=k % 4)
    assert d is not None and C.report_of(d, c["stream"]) == c["report"]
    assert agree(env, enc, c["stream"], c["b"], 0, 0) is None


def test_chunks(env, enc):
    """damaged pictures whose reference lies in the chunk in front ("decode_batch" 1), beside them (2, 3) and anywhere (the default): an I
    picture among them - it waits for the frame it is patched from"""
    M, D, C = env
    names = [n for n in sorted(C.cases()) if n.startswith(("i48", "s80")) and n.endswith(("_no_slices", "_unreadable"))]
    names += [n for n in sorted(C.cases()) if n.startswith("c48") and n.endswith("_one_of_three")]
    assert len(names) >= 12
    for name in names:
        c = C.cases()[name]
        for batch in (1, 2, 3):
            assert agree(env, enc, c["stream"], c["b"], 0, 1, batch=batch) is not None, (name, batch)
    for name, c in sorted(C.chains().items()):
        for batch in (0, 1, 2, 3):
            d = agree(env, enc, c["stream"], c["b"], c["join"], 1, D.LAYOUTS[batch], batch=batch, dst_off=batch)
            assert d is not None and C.report_of(d, c["stream"]) == c["report"]


def test_every_i_picture_damaged(env, enc):
    """the stream of I pictures alone with a row gone in every picture: each frame is patched from the patched one in front, whatever
    the chunks are"""
    M, D, C = env
    s, L = C.base_stream("i48")
    x = s
    for pic in range(len(L["fields"]) - 1, -1, -1):
        x = C.unreadable(x, pic, 0)
    for batch in (0, 1, 2, 3):
        d = agree(env, enc, x, False, 0, 1, batch=batch)
        assert d is not None and d.conceal["damaged_pictures"] == len(L["fields"]) and d.conceal["grey_rows"] == 1


def test_accepted_streams_keep_their_answer(env, enc):
    """every valid stream of the field-picture tests, and the join's open GOPs under "decode_join" 3: the same bytes and record, a report
    of zeros"""
    M, D, C = env
    for k, (name, (s, L, b)) in enumerate(sorted(C.F.cases().items())):
        want = C.F.spec_cached(s, b)[0]
        d = agree(env, enc, s, b, 0, 1, D.LAYOUTS[k & 3], batch=k % 3)
        assert d is not None and len(d.frames) == len(want.frames) and C.report_of(d, s) == (len(s), 0, 0, 0, 0), name
    for name, (s, L, c, na, letters, dropped) in sorted(C.J.open_cases().items()):
        want = C.J.spec_cached(s[c:], True, 3)[0]
        d = agree(env, enc, s[c:], True, 3, 1)
        assert d is not None and C.J.join_of(d, s[c:]) == C.J.join_of(want, s[c:]) and C.report_of(d, s[c:]) == (len(s) - c, 0, 0, 0, 0), name


def test_join_and_damage(env, enc):
    """a damaged stream behind junk, cut in its last frame, under "decode_join" 3: offsets count from the first byte of the input"""
    M, D, C = env
    g = C.J.junk()["random"]
    c = C.cases()["c48_2Pf_unreadable"]
    x = g + c["stream"][:-4]                                        # no sequence_end_code: the tail drops the last frame
    d = agree(env, enc, x, True, 3, 1, "nv12", es_off=3, dst_off=5)
    assert d is not None and d.join_offset == len(g) and d.dropped_trailing == 1
    assert C.report_of(d, x) == (c["report"][0] + len(g),) + c["report"][1:]


def test_refusals_stay(env, enc):
    M, D, C = env
    for name, (s, b, join, want) in sorted(C.refusals().items()):
        got, r, j, c = decode(M, D, enc, s, b, join, 1)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)
        assert agree(env, enc, s, b, join, 1) is None


def test_plan_streams(env, enc):
    """more than 256 events: pictures without a slice and damaged ones at every position of a range of two and of three events"""
    M, D, C = env
    for name, (s, b, join) in sorted(C.plan_streams().items()):
        if name == "long":
            continue
        d = agree(env, enc, s, b, join, 1, batch=(0, 3)[len(name) & 1])
        assert d is not None and d.conceal["damaged_pictures"] > 10, name


def test_a_fresh_handle_and_many_pictures(env):
    """more than 256 frames on a handle whose tables are sized by this call: a picture without a slice is two events"""
    M, D, C = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        e.set_option("decode_syntax", MAIN)
        for n in NEEDS:
            e.set_option(n, 1)
        s, b, join = C.plan_streams()["long"]
        d = agree(env, e, s, b, join, 1)
        assert d is not None and len(d.frames) > 256
    finally:
        e.close()


def test_option_rules(env, enc):
    """2 is no value; with a needed option missing m2v_decode_device answers M2V_E_PARAM, names the option and writes nothing; the batch
    entries do not read it"""
    import torch
    M, D, C = env
    with pytest.raises(M.M2VError):
        enc.set_option("decode_conceal", 2)
    s = C.cases()["f16_1Pt_unreadable"]["stream"]
    es = dev(s)
    buf = torch.full((1 << 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    enc.set_option("decode_conceal", 1)
    enc.set_option("decode_join", 0)
    try:
        for missing in NEEDS + ("decode_syntax",):
            enc.set_option(missing, 0)
            rc = enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(s), buf.data_ptr(), buf.numel(), M.LAYOUTS_420["i420"], D.MODES["iso"], None)
            assert rc == E_PARAM and b"decode_conceal" in enc._L.m2v_last_error(enc._h), missing
            enc.set_option(missing, 1)
        rc = enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(s), buf.data_ptr(), buf.numel(), M.LAYOUTS_420["i420"], D.MODES["module"], None)
        assert rc == E_PARAM and b"decode_conceal" in enc._L.m2v_last_error(enc._h)
        torch.cuda.synchronize()
        assert bool((buf == D.FILL).all())
    finally:
        enc.set_option("decode_conceal", 0)


def test_decode_device_keyword(env):
    """Mpeg2Encoder.decode_device(container="ts", join="both", conceal=True): a damaged stream in a transport stream from
    tests/demux_writer.py, cut at packet boundaries in front and behind, against the definition on the stream the CPU demultiplexer
    extracts (handed on with the zero padding to a whole 32-byte word, as decode_device hands it on); the option is put back"""
    M, D, C = env
    import demux_writer as X
    s0, L, letters = C.J.three_gops()
    npics = len(C.pictures_of(C.units(s0)))
    s = s0
    for pic in range(npics - 3, 2, -3):                             # a slice in every third picture cannot be read
        s = C.unreadable(s, pic, 0)
    w = X.TsWriter(11, video_pid=0x120)
    w.psi(0, X.pat_section([(1, 0x1000)]))
    w.psi(0x1000, X.pmt_section(1, 0x120, [(0x02, 0x120, b"")]))
    for n, at in enumerate(range(0, len(s), 100)):
        head = X.pes_header(0xE0, 0, pts=9000 + 3600 * n, dts=None)
        w.video(head + s[at:at + 100], pusi=1, head=len(head), stamp=(9000 + 3600 * n, X.ABSENT))
    ts = w.bytes()
    packets = len(ts) // 188
    cut = ts[:2 * 188] + ts[4 * 188:(packets - 1) * 188]
    es = M.container.demux_ts(cut)[0]
    padded = es + bytes(-len(es) % 32)
    d, at = C.spec_cached(padded, True, 3, True)
    assert d is not None and d.join_offset > 0 and d.dropped_trailing == 1 and d.conceal["damaged_pictures"] >= 2 and d.conceal["first_offset"] > d.join_offset
    assert C.spec_cached(padded, True, 3, False)[0] is None         # without the option the recording is refused
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        kw = dict(syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=True)
        with pytest.raises(M.M2VError):
            e.decode_device(dev(cut), container="ts", join="both", **kw)
        got, r = e.decode_device(dev(cut), container="ts", join="both", conceal=True, **kw)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        assert report(e) == C.report_of(d, padded) and join_record(e) == C.J.join_of(d, padded)
        assert e._set.get("decode_conceal", 0) == 0
        with pytest.raises(ValueError):
            e.decode_device(dev(s), conceal=True, syntax="main")
    finally:
        e.close()
