"""-m gpu: m2v_decode_device with option "decode_interlaced" = 1 (on "decode_syntax" = main, "decode_b_pictures" 0 or 1 as the case
says) against decoder.decode(..., syntax="main", b_pictures=..., interlaced=True) - byte for byte, record for record, err_offset for
err_offset; no tolerance anywhere.  The streams are those of tests/ilace_cases.py at their smallest shapes; tests/test_ilace_cases.py
runs them through the host build of the same arithmetic and shows from the writer's log what they reach.  Every decode writes into a
buffer of FILL with guards around the frames and a capacity of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM = -1
MAIN, MODULE = 1, 0


@pytest.fixture(scope="module")
def env():
    import ilace_cases
    return ilace_cases.M, ilace_cases.D, ilace_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, I = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    e.set_option("decode_interlaced", 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, b_pictures, layout="i420", es_off=0, dst_off=0):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written"""
    import torch
    enc.set_option("decode_b_pictures", int(bool(b_pictures)))
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


def agree(env, enc, stream, b_pictures, layout="i420", **kw):
    """the device answers what the definition answers"""
    M, D, I = env
    d, at = I.spec_cached(bytes(stream), b_pictures)
    got, r = decode(M, D, enc, stream, b_pictures, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = I.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import ilace_cases
    return sorted(ilace_cases.cases())


@pytest.mark.parametrize("name", case_names())
def test_cases(env, enc, name):
    """every valid stream of ilace_cases.cases(): each in one layout, the four going round, at a source and a destination (an odd byte
    address among them) that are not aligned"""
    M, D, I = env
    k = case_names().index(name)
    s, L = I.cases()[name]
    assert agree(env, enc, s, I.b_flag(name, L), D.LAYOUTS[k & 3], es_off=k % 5, dst_off=(3 * k + 1) % 7) is not None


def test_known_answers_against_their_literal_pictures(env, enc):
    """the device against pictures no decoder made"""
    M, D, I = env
    for name, (s, L, want) in sorted(I.known().items()):
        got, r = decode(M, D, enc, s, I.b_flag(name, L), dst_off=1)
        assert got is not None and len(got) == len(want), (name, r)
        for k, planes in enumerate(want):
            assert np.array_equal(got[k], np.concatenate([p.reshape(-1) for p in planes])), (name, k)


def test_every_layout_and_the_crop(env, enc):
    M, D, I = env
    for layout in D.LAYOUTS:
        for name in ("ipb_16", "crop_40", "mixed"):
            assert agree(env, enc, I.cases()[name][0], True, layout, dst_off=1) is not None


def test_both_settings_of_b_pictures(env, enc):
    """a stream without B pictures decodes to the same bytes with "decode_b_pictures" 0 and 1"""
    M, D, I = env
    for name in ("ip_32", "ip_48", "vector_scale"):
        s = I.cases()[name][0]
        a, b = agree(env, enc, s, False), agree(env, enc, s, True)
        assert a is not None and b is not None and np.array_equal(D.frames_of(a), D.frames_of(b))


def test_refusals(env, enc):
    """the status, the definition's offset, nothing written"""
    M, D, I = env
    for name, (s, b, want) in sorted(I.refusals().items()):
        got, r = decode(M, D, enc, s, b)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_altered_streams(env, enc):
    """a seeded sample of the altered streams, every group sampled evenly: the definition's verdict, its earliest offset, its frames
    where it accepts - never a fault"""
    M, D, I = env
    cases = I.altered()[::2]
    assert len(cases) == 150
    refused = sum(agree(env, enc, x, True) is None for _, x in cases)
    assert 40 <= refused <= len(cases) - 10


def test_invariant_on_streams_of_the_main_syntax(env, enc):
    """streams the main syntax accepts with the option off: with it on, the bytes and the record of the option off"""
    M, D, I = env
    import bpic_cases as B
    import main_cases as C
    for name in ("types", "changing", "transparent", "escapes", "no_end_tail", "repeats"):
        s = C.cases()[name][0]
        for b in (False, True):
            d = agree(env, enc, s, b)
            assert d is not None and np.array_equal(D.frames_of(d), D.frames_of(C.spec_cached(s)[0]))
    for name in ("types", "skips", "half_pel", "order_IPBBPBB", "size_17x17", "params"):
        s = B.cases()[name][0]
        d = agree(env, enc, s, True)
        assert d is not None and np.array_equal(D.frames_of(d), D.frames_of(B.spec_cached(s)[0]))
    for name, (s, want) in sorted(B.refusals().items())[::3]:
        got, r = decode(M, D, enc, s, True)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_decode_batch(env, enc):
    """"decode_batch" 0, 1, 2, 3 and 5: the B pictures' field predictions read anchors carried between chunks - identical bytes"""
    M, D, I = env
    try:
        for batch in (0, 1, 2, 3, 5):
            enc.set_option("decode_batch", batch)
            for name in ("ipbb", "ipb_48", "b_skip"):
                assert agree(env, enc, I.cases()[name][0], True, "nv12" if batch & 1 else "i420", dst_off=batch) is not None
            assert agree(env, enc, I.cases()["ip_48"][0], False) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_more_than_one_wavefront_of_slices(env, enc):
    """32 x 128, nine pictures: 72 slices in one launch; then in chunks of four"""
    M, D, I = env
    s = I.cases()["wide"][0]
    assert agree(env, enc, s, True, "nv21", dst_off=3) is not None
    try:
        enc.set_option("decode_batch", 4)
        assert agree(env, enc, s, True) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_decode_device_keyword(env):
    """decode_device(syntax="main", interlaced=True) puts the option back"""
    M, D, I = env
    s, L = I.cases()["ipb_32"]
    d, _ = I.spec_cached(s, True)
    first = [a for k, a in L["units"] if k == "picture_ext"][0]
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        got, r = e.decode_device(dev(s), syntax="main", b_pictures=True, interlaced=True)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        with pytest.raises(M.M2VError, match="err_offset %d" % first):      # the option is back: the parent's answer
            e.decode_device(dev(s), syntax="main", b_pictures=True)
        with pytest.raises(ValueError):
            e.decode_device(dev(s), interlaced=True)
        e.set_option("decode_syntax", MAIN)
        e.set_option("decode_interlaced", 1)
        with pytest.raises(M.M2VError, match="err_offset %d" % first):      # interlaced=False decodes without it, whatever the handle holds
            e.decode_device(dev(s), syntax="main", b_pictures=True)
        es = dev(I.cases()["ip_32"][0])                                     # and puts it back
        assert e._L.m2v_decode_device(e._h, es.data_ptr(), es.numel(), None, 0, 0, D.MODES["iso"], None) == 0 and e.decode_report()["status"] == D.OK
    finally:
        e.close()


def test_rules_of_the_option(env):
    """a value other than 0 and 1 is M2V_E_PARAM; the option with the module syntax or the module's mode is M2V_E_PARAM, names the
    option and writes nothing; with the option off again the stream is refused where the parent refuses it: at the first picture
    coding extension"""
    import torch
    M, D, I = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_interlaced", 2) == E_PARAM and L.m2v_set_option(h, b"decode_interlaced", -1) == E_PARAM
        s, log = I.cases()["ip_32"]
        es = dev(s)
        buf = torch.full((1 << 14,), D.FILL, dtype=torch.uint8, device="cuda:0")
        e.set_option("decode_interlaced", 1)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == E_PARAM      # the module syntax
        assert b"decode_interlaced" in L.m2v_last_error(h)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM
        e.set_option("decode_syntax", MAIN)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM   # the module's mode
        assert b"decode_interlaced" in L.m2v_last_error(h)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all()
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == 0
        assert e.decode_report()["status"] == D.OK
        e.set_option("decode_interlaced", 0)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), None, 0, 0, D.MODES["iso"], None) == 0
        r = e.decode_report()
        assert (r["status"], r["err_offset"]) == (D.SYNTAX, [a for k, a in log["units"] if k == "picture_ext"][0])
    finally:
        e.close()
