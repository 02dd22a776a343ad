"""-m gpu: m2v_decode_device with option "decode_field_pictures" = 1 (on "decode_syntax" = main and "decode_interlaced", "decode_extended",
"decode_mb_tools" = 1, "decode_b_pictures" 0 or 1 as the case says) against decoder.decode(..., syntax="main", b_pictures=...,
interlaced=True, extended=True, mb_tools=True, field_pictures=True) - byte for byte, record for record, err_offset for err_offset; no
tolerance anywhere.  The streams are those of tests/fld_cases.py at their smallest shapes; tests/test_fld_cases.py runs them through the
host build of the same functions and shows from the writer's log what they reach.  Every decode writes into a buffer of FILL with guards
around the frames and a capacity of exactly the frames' bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM = -1
MAIN, MODULE = 1, 0


@pytest.fixture(scope="module")
def env():
    import fld_cases
    return fld_cases.M, fld_cases.D, fld_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, F = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    for name in ("decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures"):
        e.set_option(name, 1)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, b, layout="i420", es_off=0, dst_off=0, fields=1):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written"""
    import torch
    enc.set_option("decode_b_pictures", int(bool(b)))
    enc.set_option("decode_field_pictures", int(fields))
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    torch.cuda.synchronize()                                        # (the stream is in place before the handle's own HIP stream reads it)
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


def agree(env, enc, stream, b, layout="i420", fields=1, **kw):
    """the device answers what the definition answers"""
    M, D, F = env
    d, at = F.spec_cached(bytes(stream), b, bool(fields))
    got, r = decode(M, D, enc, stream, b, layout, fields=fields, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout) if d.frames else np.zeros((0, int(r["frame_bytes"])), np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = F.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import fld_cases
    return sorted(fld_cases.cases())


@pytest.mark.parametrize("name", case_names())
def test_cases(env, enc, name):
    """every valid stream of fld_cases.cases() under every setting of "decode_b_pictures" that accepts it: the layouts going round, at a
    source and a destination (an odd byte address among them) that are not aligned; the option-off call on the same handle in front and
    behind gives the parent's answer - the refusal at the unit the option-off definition names"""
    M, D, F = env
    k = case_names().index(name)
    s, L, b = F.cases()[name]
    assert agree(env, enc, s, b, fields=0) is None
    for n, bb in enumerate(F.settings(b)):
        assert agree(env, enc, s, bb, D.LAYOUTS[(k + n) & 3], es_off=(k + n) % 5, dst_off=(3 * k + n + 1) % 7) is not None
    assert agree(env, enc, s, b, fields=0) is None


def test_known_answers(env, enc):
    """the device against frames the new code did not make: the option-off definition on the two progressive twins woven, the numpy
    reference on the case of each of its switches, and the literal picture"""
    M, D, F = env
    for name, (s, b, want) in sorted(F.known().items()):
        got, r = decode(M, D, enc, s, b, dst_off=1)
        assert got is not None and len(got) == len(want), (name, r)
        for k, planes in enumerate(want):
            assert np.array_equal(got[k], np.concatenate([p.reshape(-1) for p in planes])), (name, k)


def test_refusals(env, enc):
    """the status, the offset stated by hand, nothing written"""
    M, D, F = env
    for name, (s, b, f, want) in sorted(F.refusals().items()):
        got, r = decode(M, D, enc, s, b, fields=int(f))
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)


def test_altered_streams(env, enc):
    """every altered stream: the definition's verdict, its earliest offset, its frames where it accepts - never a fault"""
    M, D, F = env
    cases = F.altered()
    assert len(cases) == 300
    refused = sum(agree(env, enc, x, True) is None for _, x in cases)
    assert 30 <= refused <= 270


def plan_names():
    import fld_cases
    return sorted(fld_cases.plan_streams())


@pytest.mark.parametrize("name", plan_names())
def test_plan_streams(env, enc, name):
    """streams longer than a lane's range, a range's edge at every position of a pair; more than 256 frames"""
    M, D, F = env
    s, L, b = F.plan_streams()[name]
    assert agree(env, enc, s, b) is not None


def test_decode_batch(env, enc):
    """"decode_batch" 1, 2 and 3 (frames): every chunk's edge falls on a frame, with an I + P pair and a P + P pair at each edge - a
    second field finds its first field in the chunk, the field of its own parity in the slot carried over"""
    M, D, F = env
    try:
        for batch in (1, 2, 3):
            enc.set_option("decode_batch", batch)
            for name in ("batch_edges", "mixed", "cut_rows", "tools"):
                s, L, b = (F.cases()[name] if name != "batch_edges" else F.batch_edges())
                assert agree(env, enc, s, b, "nv12" if batch & 1 else "i420", dst_off=batch) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_decode_device_keyword(env):
    """decode_device(..., field_pictures=True) puts the option back, and raises ValueError without the three options it needs"""
    M, D, F = env
    s, L, b = F.cases()["cut_rows"]
    d, _ = F.spec_cached(s, b)
    off = F.spec_cached(s, b, False)[1]
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        kw = dict(syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True)
        got, r = e.decode_device(dev(s), field_pictures=True, **kw)
        assert np.array_equal(got.cpu().numpy(), D.frames_of(d)) and r["pictures"] == len(d.frames)
        assert all(e._set.get(n, 0) == 0 for n in ("decode_field_pictures", "decode_mb_tools", "decode_extended", "decode_interlaced"))
        with pytest.raises(M.M2VError, match="err_offset %d" % off):        # the option is back: the parent's answer
            e.decode_device(dev(s), **kw)
        for missing in ("interlaced", "extended", "mb_tools"):
            with pytest.raises(ValueError):
                e.decode_device(dev(s), field_pictures=True, **dict(kw, **{missing: False}))
        e.set_option("decode_field_pictures", 1)
        with pytest.raises(M.M2VError, match="err_offset %d" % off):        # field_pictures=False decodes without it, whatever the handle holds
            e.decode_device(dev(s), **kw)
        assert e._set["decode_field_pictures"] == 1                         # and puts it back
    finally:
        e.close()


def test_rules_of_the_option(env):
    """a value other than 0 and 1 is M2V_E_PARAM; the option without one of the three options it needs, with the module syntax or with
    the module's mode is M2V_E_PARAM, names the option and writes nothing"""
    import torch
    M, D, F = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        L, h = e._L, e._h
        assert L.m2v_set_option(h, b"decode_field_pictures", 2) == E_PARAM and L.m2v_set_option(h, b"decode_field_pictures", -1) == E_PARAM
        s, log, b = F.cases()["ip_only"]
        es = dev(s)
        buf = torch.full((1 << 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
        e.set_option("decode_field_pictures", 1)
        call = lambda mode: L.m2v_decode_device(h, es.data_ptr(), es.numel(), buf.data_ptr(), buf.numel(), 0, D.MODES[mode], None)
        names = ("decode_interlaced", "decode_extended", "decode_mb_tools")
        assert call("iso") == E_PARAM and b"decode_field_pictures" in L.m2v_last_error(h)          # the module syntax
        e.set_option("decode_syntax", MAIN)
        for missing in names + (None,):
            for n in names:
                e.set_option(n, int(n != missing))
            if missing is not None:
                assert call("iso") == E_PARAM and b"decode_field_pictures" in L.m2v_last_error(h), missing
        assert call("module") == E_PARAM and b"decode_field_pictures" in L.m2v_last_error(h)       # the module's mode
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == D.FILL).all()
        assert call("iso") == 0 and e.decode_report()["status"] == D.OK
        e.set_option("decode_field_pictures", 0)
        assert call("iso") == 0
        r = e.decode_report()
        assert (r["status"], r["err_offset"]) == (D.SYNTAX, [a for k, a in log["units"] if k == "picture_ext"][0])
    finally:
        e.close()


def test_option_off_is_the_parent(env, enc):
    """streams of the older options on the same handle with the option off, on, and off again: the same bytes, the same refusals"""
    M, D, F = env
    import mbt_cases as T
    for name in ("b15_fields", "cmv_fields", "dual_vectors", "all_tools"):
        s, L, b, i = T.cases()[name]
        want = D.frames_of(T.spec_cached(s, b, True)[0])
        for fields in (0, 1, 0):
            got, r = decode(M, D, enc, s, b, fields=fields)
            assert got is not None and np.array_equal(got, want), (name, fields)
    for name in ("marker_0", "dual_in_b_picture", "derived_outside_top", "motion_type_0"):
        s, b, i, t, want = T.refusals()[name]
        for fields in (0, 1):
            got, r = decode(M, D, enc, s, b, fields=fields)
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, fields)
