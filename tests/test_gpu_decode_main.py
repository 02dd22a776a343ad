"""-m gpu: m2v_decode_device with option "decode_syntax" = M2V_SYNTAX_MAIN against decoder.decode(..., syntax="main") - byte for
byte, record for record, err_offset for err_offset; no tolerance anywhere.  The streams are those of tests/main_cases.py at their
smallest shapes (48 x 32, 160 x 96, 1088 x 16); tests/test_main_cases.py runs them through the host build of the same arithmetic and
shows from the writer's log what they reach.  Every decode writes into a buffer of FILL with guards around the frames and a capacity
of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4
MAIN, MODULE = 1, 0


@pytest.fixture(scope="module")
def env():
    import main_cases
    return main_cases.M, main_cases.D, main_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, C = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, layout="i420", es_off=0, dst_off=0, mode="iso"):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written"""
    import torch
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES[mode], None) == 0
    r0 = enc.decode_report()
    room = int(r0["pictures"]) * int(r0["frame_bytes"]) if r0["status"] == D.OK else 4096
    buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES[mode], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r = enc.decode_report()
    got = buf.cpu().numpy()
    a, b = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    assert (got[:a] == D.FILL).all() and (got[b:] == D.FILL).all(), "bytes outside the frames were written"
    assert (r0["status"], r0["err_offset"]) == (r["status"], r["err_offset"]) or r0["status"] == D.OK      # (the probe stops behind the plan)
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0
        return None, r
    return got[a:b].reshape(int(r["pictures"]), int(r["frame_bytes"])), r      # (no picture at all: an empty array)


def agree(env, enc, stream, layout="i420", **kw):
    """the device answers what the definition answers"""
    M, D, C = env
    d, at = C.spec_cached(bytes(stream))
    got, r = decode(M, D, enc, stream, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = C.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import main_cases
    return sorted(main_cases.cases())


@pytest.mark.parametrize("name", case_names())
def test_cases(env, enc, name):
    """every valid stream of main_cases.cases(): types, precisions, scales, scans, matrices, f_codes with residuals and wraps, address
    increments with one and two escapes, optional units missing, transparent units, repeated headers, parameters that change from
    picture to picture; each in one layout, the four layouts going round, at a source and a destination that are not aligned"""
    M, D, C = env
    k = case_names().index(name)
    assert agree(env, enc, C.cases()[name][0], D.LAYOUTS[k & 3], es_off=k % 5, dst_off=(3 * k) % 7) is not None


def test_every_layout(env, enc):
    M, D, C = env
    for layout in D.LAYOUTS:
        for name in ("types", "odd_size"):
            agree(env, enc, C.cases()[name][0], layout)


def test_refusals(env, enc):
    """one stream per line of the header's list of what is still M2V_DEC_SYNTAX: the status, the definition's offset, nothing written"""
    M, D, C = env
    for name, (s, want) in sorted(C.refusals().items()):
        got, r = decode(M, D, enc, s)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_altered_streams(env, enc):
    """200 of the altered streams - 70 header flips, 80 seeded flips in slice data, 25 cuts and 25 insertions there, each group sampled
    evenly: the definition's verdict, its earliest offset, its frames where it accepts - never a fault"""
    M, D, C = env
    groups = {p: [c for c in C.altered() if c[0].startswith(p)] for p in ("bit", "flip", "cut", "ins")}
    assert [len(groups[p]) for p in ("bit", "flip", "cut", "ins")] == [887, 400, 50, 50]
    cases = groups["bit"][::12][:70] + groups["flip"][::5] + groups["cut"][::2] + groups["ins"][::2]
    assert len(cases) == 200
    refused = sum(agree(env, enc, x) is None for _, x in cases)
    assert 40 <= refused <= 190


def test_units_at_the_scan_tile(env, enc):
    """start codes of every kind - transparent units among them - three bytes in front of a multiple of the scan's tile, two, one, and on it"""
    M, D, C = env
    import main_writer as MW
    T = M.decode_scan_tile()
    rng = np.random.RandomState(17)
    pics = [C.intra_picture(rng, 3, 2, gop_extras=[MW.USER], extras=[MW.COPYRIGHT, MW.USER, MW.PICTURE_DISPLAY]), C.random_p(rng, 3, 2, extras=[MW.USER])]
    kinds = [k for k, _ in MW.stream(48, 32, pics, seq=dict(extras=[MW.USER]))[1]["units"]]
    for shift in (-3, -2, -1, 0):
        aimed = {kind: max(j for j, k in enumerate(kinds) if k == kind) for kind in set(kinds)}

        def stuff(k, kind, at):
            if aimed[kind] != k:
                return 0
            return -(-(at - shift) // T) * T + shift - at
        s, L = MW.stream(48, 32, pics, seq=dict(extras=[MW.USER]), stuff=stuff)
        assert all((a - shift) % T == 0 for j, (k, a) in enumerate(L["units"]) if aimed[k] == j)
        assert agree(env, enc, s) is not None


def test_headers_and_no_picture(env, enc):
    """sequence headers, user_data behind them and no picture: OK with no frames and nothing written, with and without an end code"""
    M, D, C = env
    t, L = C.cases()["transparent"]
    cut = [a for k, a in L["units"] if k == "gop"][0]
    for x in (t[:cut], t[:cut] + b"\x00\x00\x01\xb7"):
        d = agree(env, enc, x)
        assert d is not None and d.frames == []
        r = enc.decode_report()
        assert (r["status"], r["pictures"], r["out_bytes"], r["width"], r["height"]) == (D.OK, 0, 0, 48, 32)


def test_decode_batch(env, enc):
    """"decode_batch" 1 and 3 over the stream whose parameters change with every picture: the chunks' pictures carry their own"""
    M, D, C = env
    s = C.cases()["changing"][0]
    try:
        for batch in (1, 3):
            enc.set_option("decode_batch", batch)
            assert agree(env, enc, s, "nv12") is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_from_a_transport_stream(env):
    """a transport stream from tests/demux_writer.py - PAT, PMT, another PID, null packets - around a main-syntax stream: demultiplexed
    and decoded on the device through decode_device(container="ts", syntax="main"), which puts the option back"""
    M, D, C = env
    import demux_writer as X
    s = C.cases()["transparent"][0]
    d, _ = C.spec_cached(s)
    w = X.TsWriter(5, video_pid=0x120)
    w.psi(0, X.pat_section([(1, 0x1000)]))
    w.psi(0x1000, X.pmt_section(1, 0x120, [(0x02, 0x120, b""), (0x03, 0x121, b"")]))
    head = X.pes_header(0xE0, 0, pts=9000, dts=None)
    data = head + s
    w.video(data[:150], pusi=1, head=len(head), stamp=(9000, X.ABSENT))
    at = 150
    while at < len(data):
        if (at // 184) % 3 == 0:
            w.other(0x121)
            w.null()
        w.video(data[at:at + 184])
        at += 184
    assert w.expect()["es"] == s
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        got, r = e.decode_device(dev(w.bytes()), container="ts", syntax="main")
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        # the option is back: the module syntax refuses the stream at its first unit that is not the module's
        with pytest.raises(M.M2VError, match="M2V_DEC_SYNTAX"):
            e.decode_device(dev(s))
        with pytest.raises(ValueError):
            e.decode_device(dev(s), syntax="other")
    finally:
        e.close()


def test_rules_of_the_option(env):
    """mode "module" with the main syntax is M2V_E_PARAM; decode_streams with the option on is M2V_E_STATE and writes nothing, and the
    next legal call is right; a value other than 0 and 1 is M2V_E_PARAM; with the option off again the module syntax answers what it
    answered before, record and bytes"""
    import torch
    M, D, C = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        small = D.small()
        before, r_before = e.decode_device(dev(small), mode="module")
        before = before.cpu().numpy().copy()
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_syntax", 2) == E_PARAM and L.m2v_set_option(h, b"decode_syntax", -1) == E_PARAM
        e.set_option("decode_syntax", MAIN)
        es = dev(small)
        buf = torch.full((1 << 14,), D.FILL, dtype=torch.uint8, device="cuda:0")
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM
        assert b"decode_syntax" in L.m2v_last_error(h)
        off, nb = (np.array([0], np.uint64), np.array([len(small)], np.uint64))
        rc = L.m2v_decode_streams_device(h, es.data_ptr(), off.ctypes.data, nb.ctypes.data, 1, buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None)
        assert rc == E_STATE
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all() and len(e.decode_streams_report()) == 0
        # the next legal call: the main syntax on a stream of its own, then on the module's stream (the invariant)
        s = C.cases()["types"][0]
        got, r = e.decode_device(dev(s), syntax="main")
        assert np.array_equal(got.cpu().numpy(), D.frames_of(C.spec_cached(s)[0]))
        got, r = e.decode_device(dev(small), mode="iso", syntax="main")
        assert np.array_equal(got.cpu().numpy(), D.frames_of(M.decoder.decode(small, quirks=False)))
        # decode_device(syntax=) puts the option back to what set_option left - here main, which the C entry shows: mode "module" is refused
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM
        # ... and syntax="module", the default, decodes with the module syntax on such a handle, and leaves main behind
        got, r = e.decode_device(dev(small), mode="module")
        assert np.array_equal(got.cpu().numpy(), before)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM
        e.set_option("decode_syntax", MODULE)
        after, r_after = e.decode_device(dev(small), mode="module")
        assert np.array_equal(after.cpu().numpy(), before) and r_after.tobytes() == r_before.tobytes()
        frames, recs = e.decode_streams(dev(small), [(0, len(small))], mode="module")
        assert recs["rec"]["status"][0] == D.OK and np.array_equal(frames.cpu().numpy(), before.reshape(-1))
    finally:
        e.close()
