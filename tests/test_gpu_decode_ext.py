"""-m gpu: m2v_decode_device with option "decode_extended" = 1 (on "decode_syntax" = main, "decode_b_pictures" and "decode_interlaced" 0 or
1 as the case says) against decoder.decode(..., syntax="main", b_pictures=..., interlaced=..., extended=True) - byte for byte, record
for record, err_offset for err_offset; no tolerance anywhere.  The streams are those of tests/ext_cases.py at their smallest shapes;
tests/test_ext_cases.py runs them through the host build of the same functions and shows from the writer's log what they reach.
Every decode writes into a buffer of FILL with guards around the frames and a capacity of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM = -1
MAIN, MODULE = 1, 0


@pytest.fixture(scope="module")
def env():
    import ext_cases
    return ext_cases.M, ext_cases.D, ext_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, X = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    e.set_option("decode_extended", 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, b, i, layout="i420", es_off=0, dst_off=0):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written"""
    import torch
    enc.set_option("decode_b_pictures", int(bool(b)))
    enc.set_option("decode_interlaced", int(bool(i)))
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
    a, b_ = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    assert (got[:a] == D.FILL).all() and (got[b_:] == D.FILL).all(), "bytes outside the frames were written"
    assert (r0["status"], r0["err_offset"]) == (r["status"], r["err_offset"]) or r0["status"] == D.OK      # (the probe stops behind the plan)
    if r0["status"] == D.OK:
        assert (int(r0["pictures"]), int(r0["frame_bytes"]), int(r0["out_bytes"])) == (int(r["pictures"]), int(r["frame_bytes"]), room)
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0
        return None, r
    return got[a:b_].reshape(int(r["pictures"]), int(r["frame_bytes"])), r


def agree(env, enc, stream, b, i, layout="i420", **kw):
    """the device answers what the definition answers"""
    M, D, X = env
    d, at = X.spec_cached(bytes(stream), b, i)
    got, r = decode(M, D, enc, stream, b, i, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = X.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import ext_cases
    return sorted(ext_cases.cases())


@pytest.mark.parametrize("name", case_names())
def test_cases(env, enc, name):
    """every valid stream of ext_cases.cases(): each in one layout, the four going round, at a source and a destination (an odd byte
    address among them) that are not aligned"""
    M, D, X = env
    k = case_names().index(name)
    s, L, b, i = X.cases()[name]
    assert agree(env, enc, s, b, i, D.LAYOUTS[k & 3], es_off=k % 5, dst_off=(3 * k + 1) % 7) is not None


def test_known_answers(env, enc):
    """the device against frames the new code did not make: the option-off definition on the twin streams, and literal pictures"""
    M, D, X = env
    for name, (s, b, i, want) in sorted(X.known().items()):
        got, r = decode(M, D, enc, s, b, i, dst_off=1)
        assert got is not None and len(got) == len(want), (name, r)
        for k, planes in enumerate(want):
            assert np.array_equal(got[k], np.concatenate([p.reshape(-1) for p in planes])), (name, k)


def test_refusals(env, enc):
    """the status, the offset stated by hand, nothing written"""
    M, D, X = env
    for name, (s, b, i, want) in sorted(X.refusals().items()):
        got, r = decode(M, D, enc, s, b, i)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_refusals_of_the_older_options_stay(env, enc):
    M, D, X = env
    for name, (s, b, i, want) in sorted(X.older_refusals().items()):
        got, r = decode(M, D, enc, s, b, i)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_altered_streams(env, enc):
    """the evenly sampled half of the altered streams: the definition's verdict, its earliest offset, its frames where it accepts - never
    a fault.  By decoder.py, counted on the CPU before the bound was written: 54 of the 150 accepted, 96 refused"""
    M, D, X = env
    cases = X.altered_sample()
    assert len(cases) == 150
    refused = sum(agree(env, enc, x, True, False) is None for _, x in cases)
    assert 15 <= refused <= len(cases) - 15


def test_all_four_settings_of_the_other_two_options(env, enc):
    """a cut stream of progressive I / P pictures decodes to the same bytes under all four; B pictures with "decode_b_pictures" off are
    refused at the first B picture's header"""
    M, D, X = env
    s = X.cases()["ip_cut"][0]
    frames = [D.frames_of(agree(env, enc, s, b, i)) for b in (False, True) for i in (False, True)]
    assert all(np.array_equal(frames[0], f) for f in frames[1:])
    for i in (False, True):
        assert agree(env, enc, X.cases()["ipbb_cut"][0], False, i) is None
        assert agree(env, enc, X.cases()["fields_ip_cut"][0], i, True) is not None
    assert agree(env, enc, X.cases()["fields_ip_cut"][0], False, False) is None


def test_decode_batch(env, enc):
    """"decode_batch" 0, 1, 2, 3 and 5 on the B streams: the matrices change from picture to picture across every chunk's edge, the
    slices of a chunk are counted from the plan's table - identical bytes"""
    M, D, X = env
    try:
        for batch in (0, 1, 2, 3, 5):
            enc.set_option("decode_batch", batch)
            for name in ("quant_bbb", "ipbb_cut", "fields_cut", "quant_coded_order"):
                s, L, b, i = X.cases()[name]
                assert agree(env, enc, s, b, i, "nv12" if batch & 1 else "i420", dst_off=batch) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_288_slices(env, enc):
    """64 x 128, nine pictures, one macroblock per slice: more than one wavefront of slices, the binary search across pictures; whole
    and in chunks of four"""
    M, D, X = env
    s, L, b, i = X.cases()["many"]
    assert len(L["cuts"]) == 288
    assert agree(env, enc, s, b, i, "nv21", dst_off=3) is not None
    try:
        enc.set_option("decode_batch", 4)
        assert agree(env, enc, s, b, i) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_invariant_on_older_cases(env, enc):
    """streams the main syntax accepts with the option off: with it on, the bytes and the record of the option off"""
    M, D, X = env
    valid = X.older_valid()
    for name in ("main_types", "main_transparent", "main_escapes", "main_repeats", "main_no_end_tail", "bpic_types", "bpic_skips", "bpic_order_IPBBPBB",
                 "ilace_mixed", "ilace_ipbb", "ilace_b_skip", "ilace_crop_40"):
        s, b, i = valid[name]
        d = agree(env, enc, s, b, i)
        off, _ = X.spec_cached(s, b, i, False)
        assert d is not None and np.array_equal(D.frames_of(d), D.frames_of(off)) and X.record_of(d, s) == X.record_of(off, s)


def test_decode_device_keyword(env):
    """decode_device(syntax="main", extended=True) puts the option back"""
    M, D, X = env
    s, L, b, i = X.cases()["ipbb_cut"]
    d, _ = X.spec_cached(s, True, False)
    off = X.spec_cached(s, True, False, False)[1]
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        got, r = e.decode_device(dev(s), syntax="main", b_pictures=True, extended=True)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        assert e._set.get("decode_extended", 0) == 0
        with pytest.raises(M.M2VError, match="err_offset %d" % off):        # the option is back: the parent's answer
            e.decode_device(dev(s), syntax="main", b_pictures=True)
        with pytest.raises(ValueError):
            e.decode_device(dev(s), extended=True)
        e.set_option("decode_syntax", MAIN)
        e.set_option("decode_extended", 1)
        with pytest.raises(M.M2VError, match="err_offset %d" % off):        # extended=False decodes without it, whatever the handle holds
            e.decode_device(dev(s), syntax="main", b_pictures=True)
        assert e._set["decode_extended"] == 1                               # and puts it back
        es = dev(X.cases()["ip_cut"][0])
        assert e._L.m2v_decode_device(e._h, es.data_ptr(), es.numel(), None, 0, 0, D.MODES["iso"], None) == 0 and e.decode_report()["status"] == D.OK
    finally:
        e.close()


def test_rules_of_the_option(env):
    """a value other than 0 and 1 is M2V_E_PARAM; the option with the module syntax or the module's mode is M2V_E_PARAM, names the
    option and writes nothing; with the option off again the stream is refused where the parent refuses it: at the first slice that
    is a row's second"""
    import torch
    M, D, X = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_extended", 2) == E_PARAM and L.m2v_set_option(h, b"decode_extended", -1) == E_PARAM
        s, log, b, i = X.cases()["ip_cut"]
        es = dev(s)
        buf = torch.full((1 << 14,), D.FILL, dtype=torch.uint8, device="cuda:0")
        e.set_option("decode_extended", 1)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == E_PARAM      # the module syntax
        assert b"decode_extended" in L.m2v_last_error(h)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM
        e.set_option("decode_syntax", MAIN)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["module"], None) == E_PARAM   # the module's mode
        assert b"decode_extended" in L.m2v_last_error(h)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all()
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES["iso"], None) == 0
        assert e.decode_report()["status"] == D.OK
        e.set_option("decode_extended", 0)
        assert L.m2v_decode_device(h, es.data_ptr(), es.numel(), None, 0, 0, D.MODES["iso"], None) == 0
        r = e.decode_report()
        assert (r["status"], r["err_offset"]) == (D.SYNTAX, X.spec_cached(s, False, False, False)[1])
        assert r["err_offset"] in [a for k, a in log["units"] if k == "slice"][1:]
    finally:
        e.close()
