"""-m gpu: the streams of tests/vec_cases.py - motion vectors at every f_code, with wraps, residuals, negative odd predictors, far reads
at the largest width - through m2v_decode_device on "decode_syntax" = main under the least capable option set that accepts each stream
and under every more capable one: "decode_interlaced" alone (dec_i), with "decode_extended" (dec_x), with "decode_mb_tools" (dec_x with
its tools), with "decode_field_pictures" (dec_f) and with "decode_join" = 3 on a whole stream (dec_j), "decode_b_pictures" either way
where the stream has no B picture.  The expectation is decoder.decode(...) with the same options - byte for byte, record for record,
err_offset for err_offset, no tolerance anywhere; tests/test_vec_cases.py shows on the CPU that tests/vec_ref.py, which reads only the
codes the writer logged, gives the same frames, and what the streams reach.  Every decode writes into a buffer of FILL with guards
around the frames and a capacity of exactly the frames' bytes, at a source and a destination that are not aligned."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MAIN = 1
OPTIONS = ("decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures")
KEYS = ("b_pictures", "interlaced", "extended", "mb_tools", "field_pictures")
GAP = b"\x00\x00\x01"


@pytest.fixture(scope="module")
def env():
    import vec_cases
    return vec_cases.M, vec_cases.D, vec_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D, V = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, o, join=0, layout="i420", es_off=0, dst_off=0, batch=0):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written.  The handle's options are put back"""
    import torch
    try:
        for name, key in zip(OPTIONS, KEYS):
            enc.set_option(name, int(bool(o[key])))
        enc.set_option("decode_join", int(join))
        enc.set_option("decode_batch", int(batch))
        es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
        torch.cuda.synchronize()                                    # (the stream is in place before the handle's own HIP stream reads it)
        assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES["iso"], None) == 0, enc._L.m2v_last_error(enc._h)
        r0 = enc.decode_report()
        room = int(r0["pictures"]) * int(r0["frame_bytes"]) if r0["status"] == D.OK else 4096
        buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES["iso"], None)
        assert rc == 0, enc._L.m2v_last_error(enc._h)
        r = enc.decode_report()
    finally:
        enc.set_option("decode_join", 0)
        enc.set_option("decode_batch", 0)
        for name in OPTIONS[::-1]:
            enc.set_option(name, 0)
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


def agree(env, enc, stream, o, join=0, layout="i420", **kw):
    """the device answers what the definition answers under the same options"""
    M, D, V = env
    d, at = V.spec_cached(bytes(stream), o, join)
    got, r = decode(M, D, enc, stream, o, join, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8]
    rec = V.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def case_names():
    import vec_cases
    return vec_cases.NAMES


@pytest.mark.parametrize("name", case_names())
def test_streams(env, enc, name):
    """every stream under every option set of its ladder, the layouts going round, unaligned source and destination"""
    M, D, V = env
    k = case_names().index(name)
    c = V.get(name)
    for n, (unit, o, join) in enumerate(V.ladder(c)):
        assert agree(env, enc, c["stream"], o, join, D.LAYOUTS[(k + n) & 3], es_off=(k + n) % 5, dst_off=(3 * k + n + 1) % 7) is not None, unit


def batch_names():
    import vec_cases
    return vec_cases.BATCH_NAMES


@pytest.mark.parametrize("name", batch_names())
def test_decode_batch(env, enc, name):
    """"decode_batch" 1 and 2 on the streams with B pictures and on the field pictures: a vector's read crosses the chunk's edge into the
    anchors carried over"""
    M, D, V = env
    c = V.get(name)
    ladder = V.ladder(c)
    for batch in (1, 2):
        for unit, o, join in (ladder[0], [x for x in ladder if x[0] == "dec_j"][0]):      # the least capable unit and dec_j
            assert agree(env, enc, c["stream"], o, join, "nv12" if batch & 1 else "i420", dst_off=batch, batch=batch) is not None, (unit, batch)


def test_known_answers(env, enc):
    """the device against pictures typed by hand: the halved negative odd predictor, the dual-prime factors with top_field_first 0, the
    far read at 2048 samples"""
    M, D, V = env
    for name, k in sorted(V.known().items()):
        want = np.stack([np.concatenate([p.reshape(-1) for p in f]) for f in k["frames"]])
        for unit, o, join in V.ladder(k):
            got, r = decode(M, D, enc, k["stream"], o, join, dst_off=1)
            assert got is not None and np.array_equal(got, want), (name, unit, r)


def test_refusals(env, enc):
    """a component inside its f_code's range whose read is not inside the picture - a field vector, a derived dual-prime vector, a lower
    16 x 8 vector: the status, the offset stated by hand, nothing written, under every option set"""
    M, D, V = env
    for name, c in sorted(V.refusals().items()):
        for unit, o, join in V.ladder(c):
            got, r = decode(M, D, enc, c["stream"], o, join)
            assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, c["offset"]), (name, unit, r)


def test_three_streams_of_one_call(env):
    """il_fcodes, dual_far and conceal_fcodes as three streams of one m2v_decode_streams_main_ex_device call with the b_pictures,
    interlaced, extended and mb_tools flags: the verdicts and the frames of the single-stream calls"""
    import torch
    import decstreams_ex_cases as X
    M, D, V = env
    batch = [V.get(n)["stream"] for n in ("il_fcodes", "dual_far", "conceal_fcodes")]
    o = dict(b_pictures=True, interlaced=True, extended=True, mb_tools=True, field_pictures=False)
    data, seg = X.place(batch, GAP, lead=1)
    e = M.Mpeg2Encoder(XL=6, YL=6)
    try:
        es = dev(data)
        off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
        nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
        call = lambda dst, cap: e._L.m2v_decode_streams_main_ex_device(e._h, es.data_ptr(), off, nb, len(seg), dst, cap, M.LAYOUTS_420["i420"], 15, None)
        torch.cuda.synchronize()
        assert call(None, 0) == 0, e._L.m2v_last_error(e._h)
        r0 = X.records_of(e.decode_streams_report())
        total = max(r["out_offset"] + r["out_bytes"] for r in r0)
        buf = torch.full((2 * X.GUARD + total,), X.FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert call(buf.data_ptr() + X.GUARD, total) == 0, e._L.m2v_last_error(e._h)
        recs = X.records_of(e.decode_streams_report())
        got = buf.cpu().numpy()
        assert (got[:X.GUARD] == X.FILL).all() and (got[X.GUARD + total:] == X.FILL).all()
        e.set_option("decode_syntax", MAIN)
        for b, s in enumerate(batch):
            d, at = V.spec_cached(s, o)
            assert d is not None and recs[b]["status"] == D.OK, (b, recs[b])
            want = D.frames_of(d)
            a = X.GUARD + recs[b]["out_offset"]
            assert recs[b]["out_bytes"] == want.size and np.array_equal(got[a:a + want.size], want.reshape(-1)), b
            one, r = decode(M, D, e, s, o)
            assert np.array_equal(one.reshape(-1), got[a:a + want.size]) and {k: int(r[k]) for k in D.STAT_FIELDS} == {k: int(recs[b][k]) for k in D.STAT_FIELDS}, b
    finally:
        e.close()
