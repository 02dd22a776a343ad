"""-m gpu: m2v_decode_device with option "decode_b_pictures" = 1 (on "decode_syntax" = main) against
decoder.decode(..., syntax="main", b_pictures=True) - byte for byte in display order, record for record, err_offset for err_offset; no
tolerance anywhere.  The streams are those of tests/bpic_cases.py at their smallest shapes; tests/test_bpic_cases.py runs them through
the host build of the same arithmetic and shows from the writer's log what they reach.  Every decode writes into a buffer of FILL with
guards around the frames and a capacity of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4
MAIN, MODULE = 1, 0


@pytest.fixture(scope="module")
def env():
    import bpic_cases
    return bpic_cases.M, bpic_cases.D, bpic_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, B = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    e.set_option("decode_b_pictures", 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, layout="i420", es_off=0, dst_off=0):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written"""
    import torch
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES["iso"], None) == 0
    r0 = enc.decode_report()
    room = int(r0["pictures"]) * int(r0["frame_bytes"]) if r0["status"] == D.OK else 4096
    buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES["iso"], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r = enc.decode_report()
    got = buf.cpu().numpy()
    a, b = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    assert (got[:a] == D.FILL).all() and (got[b:] == D.FILL).all(), "bytes outside the frames were written"
    assert (r0["status"], r0["err_offset"]) == (r["status"], r["err_offset"]) or r0["status"] == D.OK      # (the probe stops behind the plan)
    if r0["status"] == D.OK:
        assert (int(r0["pictures"]), int(r0["frame_bytes"]), int(r0["out_bytes"])) == (int(r["pictures"]), int(r["frame_bytes"]), room)
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0
        return None, r
    return got[a:b].reshape(int(r["pictures"]), int(r["frame_bytes"])), r


def agree(env, enc, stream, layout="i420", **kw):
    """the device answers what the definition answers"""
    M, D, B = env
    d, at = B.spec_cached(bytes(stream))
    got, r = decode(M, D, enc, stream, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = B.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import bpic_cases
    return sorted(bpic_cases.cases())


@pytest.mark.parametrize("name", case_names())
def test_cases(env, enc, name):
    """every valid stream of bpic_cases.cases(): each in one layout, the four going round, at a source and a destination (an odd byte
    address among them) that are not aligned"""
    M, D, B = env
    k = case_names().index(name)
    assert agree(env, enc, B.cases()[name][0], D.LAYOUTS[k & 3], es_off=k % 5, dst_off=(3 * k + 1) % 7) is not None


def test_every_layout_and_the_crop(env, enc):
    M, D, B = env
    for layout in D.LAYOUTS:
        for name in ("types", "size_40x24", "size_17x17"):
            assert agree(env, enc, B.cases()[name][0], layout, dst_off=1) is not None


def test_refusals(env, enc):
    """the status, the definition's offset, nothing written"""
    M, D, B = env
    for name, (s, want) in sorted(B.refusals().items()):
        got, r = decode(M, D, enc, s)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_superset_of_the_option_off(env, enc):
    """streams without B pictures: with the option on, the bytes and the record of the option off (the definition's, which
    tests/test_bpic_cases.py holds equal for both values)"""
    M, D, B = env
    for name in ("types", "changing", "transparent", "escapes", "no_end_tail", "repeats"):
        s = B.C.cases()[name][0]
        d = agree(env, enc, s)
        assert d is not None and np.array_equal(D.frames_of(d), D.frames_of(B.C.spec_cached(s)[0]))
    for name, (s, want) in sorted(B.C.refusals().items()):
        if name not in ("b_picture",):
            got, r = decode(M, D, enc, s)
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_altered_streams(env, enc):
    """about 300 of the altered streams, each group sampled evenly: the definition's verdict, its earliest offset, its frames where it
    accepts - never a fault"""
    M, D, B = env
    groups = {p: [c for c in B.altered() if c[0].startswith(p)] for p in ("bit", "flip", "cut", "ins")}
    cases = groups["bit"][::2] + groups["flip"][::2][:120] + groups["cut"] + groups["ins"]
    assert 270 <= len(cases) <= 330
    refused = sum(agree(env, enc, x) is None for _, x in cases)
    assert 50 <= refused <= len(cases) - 50


def test_decode_batch(env, enc):
    """"decode_batch" 0, 1, 2, 3 and 5 on the order streams: chunks that end between an anchor and its B pictures, anchors carried over
    one and two chunks - identical bytes and records"""
    M, D, B = env
    try:
        for batch in (0, 1, 2, 3, 5):
            enc.set_option("decode_batch", batch)
            for letters in B.ORDERS:
                assert agree(env, enc, B.cases()["order_" + letters][0], "nv12" if batch & 1 else "i420", dst_off=batch) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_overflow_writes_nothing(env, enc):
    import torch
    M, D, B = env
    s = B.cases()["order_IPBBPBB"][0]
    es = dev(s)
    cap = 7 * 2304
    buf = torch.full((cap + 64,), D.FILL, dtype=torch.uint8, device="cuda:0")
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(s), buf.data_ptr(), cap - 1, 0, D.MODES["iso"], None) == 0
    r = enc.decode_report()
    assert (r["status"], r["out_bytes"], r["pictures"]) == (D.OVERFLOW, 0, 7) and (buf.cpu().numpy() == D.FILL).all()
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(s), buf.data_ptr(), cap, 0, D.MODES["iso"], None) == 0
    assert enc.decode_report()["status"] == D.OK and (buf.cpu().numpy()[cap:] == D.FILL).all()


def test_refused_in_a_late_b_slice_of_the_last_chunk(env, enc):
    """I P B B P B B in chunks of three, the last B picture's last slice made unreadable: the record names that slice, and of the
    output only what the chunks in front wrote is touched"""
    import torch
    M, D, B = env
    s, L = B.cases()["order_IPBBPBB"]
    at = [a for k, a in L["units"] if k == "slice"][-1]
    bad = s[:at + 4] + bytes([s[at + 4] | 0x04]) + s[at + 5:]           # extra_bit_slice 1
    d, want = B.spec_cached(bad)
    assert d is None and want == at
    good = D.frames_of(B.spec_cached(s)[0])
    es = dev(bad)
    try:
        enc.set_option("decode_batch", 3)
        buf = torch.full((7 * 2304 + 64,), D.FILL, dtype=torch.uint8, device="cuda:0")
        assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(bad), buf.data_ptr(), 7 * 2304, 0, D.MODES["iso"], None) == 0
        r = enc.decode_report()
        assert (r["status"], r["err_offset"], r["out_bytes"], r["pictures"]) == (D.SYNTAX, at, 0, 7)
        got = buf.cpu().numpy()[:7 * 2304].reshape(7, 2304)
        # chunks [I P B], [B P B], [B] in coded order, display indices [0 3 1], [2 6 4], [5]: the first two chunks are written before the
        # third's slices are judged, as the header allows; the last chunk's picture, display index 5, is not
        for k in (0, 1, 2, 3, 4, 6):
            assert np.array_equal(got[k], good[k]), k
        assert (got[5] == D.FILL).all()
    finally:
        enc.set_option("decode_batch", 0)


def test_one_size_above_the_small_ones(env, enc):
    """336 x 64, eighteen pictures: mbw over 16, 72 slices in one launch (more than a wavefront), sixteen B pictures in one launch; then
    in chunks of five"""
    M, D, B = env
    s = B.wide()[0]
    assert agree(env, enc, s, "nv21", dst_off=3) is not None
    try:
        enc.set_option("decode_batch", 5)
        assert agree(env, enc, s) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_from_a_transport_stream(env):
    """decode_device(container="ts", syntax="main", b_pictures=True) puts both options back"""
    M, D, B = env
    import demux_writer as X
    s = B.cases()["order_IPBPBBBP"][0]
    d, _ = B.spec_cached(s)
    w = X.TsWriter(5, video_pid=0x120)
    w.psi(0, X.pat_section([(1, 0x1000)]))
    w.psi(0x1000, X.pmt_section(1, 0x120, [(0x02, 0x120, b"")]))
    head = X.pes_header(0xE0, 0, pts=9000, dts=None)
    data = head + s
    w.video(data[:150], pusi=1, head=len(head), stamp=(9000, X.ABSENT))
    for at in range(150, len(data), 184):
        w.video(data[at:at + 184])
    assert w.expect()["es"] == s
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        got, r = e.decode_device(dev(w.bytes()), container="ts", syntax="main", b_pictures=True)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        # both options are back: the main syntax without B pictures refuses the stream at its first B picture header ...
        first_b = [a for k, a in B.cases()["order_IPBPBBBP"][1]["units"] if k == "picture"][2]
        with pytest.raises(M.M2VError, match="err_offset %d" % first_b):
            e.decode_device(dev(s), syntax="main")
        with pytest.raises(M.M2VError, match="M2V_DEC_SYNTAX"):      # ... and the module syntax at a unit of its own
            e.decode_device(dev(s))
        with pytest.raises(ValueError):
            e.decode_device(dev(s), b_pictures=True)
        # set_option leaves it on the handle, decode_device(b_pictures=False) decodes without it and puts it back
        e.set_option("decode_syntax", MAIN)
        e.set_option("decode_b_pictures", 1)
        with pytest.raises(M.M2VError, match="err_offset %d" % first_b):
            e.decode_device(dev(s), syntax="main")
        got, r = e.decode_device(dev(s), syntax="main", b_pictures=True)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d))
        es = dev(s)
        assert e._L.m2v_decode_device(e._h, es.data_ptr(), es.numel(), None, 0, 0, D.MODES["iso"], None) == 0 and e.decode_report()["status"] == D.OK
    finally:
        e.close()


def test_rules_of_the_option(env):
    """a value other than 0 and 1 is M2V_E_PARAM; the option with the module syntax or the module's mode is M2V_E_PARAM, names the
    option and writes nothing; m2v_decode_streams_device with the main syntax is still M2V_E_STATE; with the option off again the
    B picture is refused where it was"""
    import torch
    M, D, B = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_b_pictures", 2) == E_PARAM and L.m2v_set_option(h, b"decode_b_pictures", -1) == E_PARAM
        s = B.cases()["types"][0]
        es = dev(s)
        buf = torch.full((1 << 14,), D.FILL, dtype=torch.uint8, device="cuda:0")
        e.set_option("decode_b_pictures", 1)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == E_PARAM      # the module syntax
        assert b"decode_b_pictures" in L.m2v_last_error(h)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM
        e.set_option("decode_syntax", MAIN)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM   # the module's mode
        assert b"decode_b_pictures" in L.m2v_last_error(h)
        off, nb = (np.array([0], np.uint64), np.array([len(s)], np.uint64))
        assert L.m2v_decode_streams_device(h, es.data_ptr(), off.ctypes.data, nb.ctypes.data, 1, buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == E_STATE
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all()
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == 0
        assert e.decode_report()["status"] == D.OK
        e.set_option("decode_b_pictures", 0)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), None, 0, 0, D.MODES["iso"], None) == 0
        r = e.decode_report()
        assert (r["status"], r["err_offset"]) == (D.SYNTAX, [a for k, a in B.cases()["types"][1]["units"] if k == "picture"][2])
    finally:
        e.close()
