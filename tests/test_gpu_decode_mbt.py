"""-m gpu: m2v_decode_device with option "decode_mb_tools" = 1 (on "decode_syntax" = main and "decode_extended" = 1, "decode_b_pictures"
and "decode_interlaced" 0 or 1 as the case says) against decoder.decode(..., syntax="main", b_pictures=..., interlaced=..., extended=True,
mb_tools=True) - byte for byte, record for record, err_offset for err_offset; no tolerance anywhere.  The streams are those of
tests/mbt_cases.py at their smallest shapes; tests/test_mbt_cases.py runs them through the host build of the same functions and shows
from the writer's log what they reach.  Every decode writes into a buffer of FILL with guards around the frames and a capacity of
exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM = -1
MAIN, MODULE = 1, 0


@pytest.fixture(scope="module")
def env():
    import mbt_cases
    return mbt_cases.M, mbt_cases.D, mbt_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, T = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    e.set_option("decode_extended", 1)
    e.set_option("decode_mb_tools", 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, b, i, layout="i420", es_off=0, dst_off=0, tools=1):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written"""
    import torch
    enc.set_option("decode_b_pictures", int(bool(b)))
    enc.set_option("decode_interlaced", int(bool(i)))
    enc.set_option("decode_mb_tools", int(tools))
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


def agree(env, enc, stream, b, i, layout="i420", tools=1, **kw):
    """the device answers what the definition answers"""
    M, D, T = env
    d, at = T.spec_cached(bytes(stream), b, i, bool(tools))
    got, r = decode(M, D, enc, stream, b, i, layout, tools=tools, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = T.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import mbt_cases
    return sorted(mbt_cases.cases())


@pytest.mark.parametrize("name", case_names())
def test_cases(env, enc, name):
    """every valid stream of mbt_cases.cases() under every setting of the other two options that accepts it: the layouts going round,
    at a source and a destination (an odd byte address among them) that are not aligned; the option-off call on the same handle in
    front and behind gives the parent's answer - the refusal at the unit the option-off definition names"""
    M, D, T = env
    k = case_names().index(name)
    s, L, b, i = T.cases()[name]
    assert agree(env, enc, s, b, i, tools=0) is None
    for n, (bb, ii) in enumerate(T.settings(b, i)):
        assert agree(env, enc, s, bb, ii, D.LAYOUTS[(k + n) & 3], es_off=(k + n) % 5, dst_off=(3 * k + n + 1) % 7) is not None
    assert agree(env, enc, s, b, i, tools=0) is None


def test_known_answers(env, enc):
    """the device against frames the new code did not make: the option-off definition on the twin streams, the numpy reference of dual
    prime, and the literal picture"""
    M, D, T = env
    for name, (s, b, i, want) in sorted(T.known().items()):
        got, r = decode(M, D, enc, s, b, i, dst_off=1)
        assert got is not None and len(got) == len(want), (name, r)
        for k, planes in enumerate(want):
            assert np.array_equal(got[k], np.concatenate([p.reshape(-1) for p in planes])), (name, k)


def test_refusals(env, enc):
    """the status, the offset stated by hand, nothing written"""
    M, D, T = env
    for name, (s, b, i, t, want) in sorted(T.refusals().items()):
        got, r = decode(M, D, enc, s, b, i, tools=int(t))
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_altered_streams(env, enc):
    """every altered stream: the definition's verdict, its earliest offset, its frames where it accepts - never a fault"""
    M, D, T = env
    cases = T.altered()
    assert len(cases) == 300
    refused = sum(agree(env, enc, x, False, True) is None for _, x in cases)
    assert 30 <= refused <= 270


def test_option_off_is_the_parent(env, enc):
    """streams of the extended option on the same handle with the option off, on, and off again: the same bytes each time"""
    M, D, T = env
    import ext_cases as X
    for name in ("ipbb_cut", "fields_cut", "headers", "quant_bbb"):
        s, L, b, i = X.cases()[name]
        want = D.frames_of(X.spec_cached(s, b, i)[0])
        for tools in (0, 1, 0):
            got, r = decode(M, D, enc, s, b, i, tools=tools)
            assert got is not None and np.array_equal(got, want), (name, tools)
    for name in ("gap", "quant_weight_0", "closing_bit_missing"):
        s, b, i, want = X.refusals()[name]
        for tools in (0, 1):
            got, r = decode(M, D, enc, s, b, i, tools=tools)
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, tools)


def test_decode_batch(env, enc):
    """"decode_batch" 1 and 2 on streams whose P pictures read their reference twice: a dual-prime macroblock's second prediction finds
    the reference in the chunk, in the slot carried over, and behind a carried copy - identical bytes"""
    M, D, T = env
    try:
        for batch in (1, 2):
            enc.set_option("decode_batch", batch)
            for name in ("all_tools", "dual_vectors", "b15_fields", "cmv_b"):
                s, L, b, i = T.cases()[name]
                assert agree(env, enc, s, b, i, "nv12" if batch & 1 else "i420", dst_off=batch) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_decode_device_keyword(env):
    """decode_device(syntax="main", extended=True, mb_tools=True) puts the option back"""
    M, D, T = env
    s, L, b, i = T.cases()["all_tools"]
    d, _ = T.spec_cached(s, b, i)
    off = T.spec_cached(s, b, i, False)[1]
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        got, r = e.decode_device(dev(s), syntax="main", interlaced=True, extended=True, mb_tools=True)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        assert e._set.get("decode_mb_tools", 0) == 0 and e._set.get("decode_extended", 0) == 0
        with pytest.raises(M.M2VError, match="err_offset %d" % off):        # the option is back: the parent's answer
            e.decode_device(dev(s), syntax="main", interlaced=True, extended=True)
        with pytest.raises(ValueError):
            e.decode_device(dev(s), syntax="main", interlaced=True, mb_tools=True)
        e.set_option("decode_mb_tools", 1)
        with pytest.raises(M.M2VError, match="err_offset %d" % off):        # mb_tools=False decodes without it, whatever the handle holds
            e.decode_device(dev(s), syntax="main", interlaced=True, extended=True)
        assert e._set["decode_mb_tools"] == 1                               # and puts it back
    finally:
        e.close()


def test_rules_of_the_option(env):
    """a value other than 0 and 1 is M2V_E_PARAM; the option without "decode_extended", with the module syntax or with the module's mode
    is M2V_E_PARAM, names the option and writes nothing"""
    import torch
    M, D, T = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_mb_tools", 2) == E_PARAM and L.m2v_set_option(h, b"decode_mb_tools", -1) == E_PARAM
        s, log, b, i = T.cases()["cmv_ip"]
        es = dev(s)
        buf = torch.full((1 << 14,), D.FILL, dtype=torch.uint8, device="cuda:0")
        e.set_option("decode_mb_tools", 1)
        call = lambda mode: L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES[mode], None)
        assert call("iso") == E_PARAM and b"decode_mb_tools" in L.m2v_last_error(h)          # the module syntax
        e.set_option("decode_syntax", MAIN)
        assert call("iso") == E_PARAM and b"decode_mb_tools" in L.m2v_last_error(h)          # without "decode_extended"
        e.set_option("decode_extended", 1)
        assert call("module") == E_PARAM                                                     # the module's mode
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all()
        assert call("iso") == 0 and e.decode_report()["status"] == D.OK
        e.set_option("decode_mb_tools", 0)
        assert call("iso") == 0
        r = e.decode_report()
        assert (r["status"], r["err_offset"]) == (D.SYNTAX, [a for k, a in log["units"] if k == "picture_ext"][0])
    finally:
        e.close()
