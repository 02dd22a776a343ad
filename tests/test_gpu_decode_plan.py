"""-m gpu: the main-syntax decode plans - k_dm_plan, k_db_plan, k_di_plan, k_dx_plan, k_dt_plan through m2v_decode_device, k_dsm_plan
through m2v_decode_streams_main_device - on the streams of tests/plan_cases.py, whose event lists give every lane a range of 1 to 13
events: several pictures a range, ranges cut at every position of a picture's units, empty trailing lanes, an event list that is
grown and a plan that runs twice.  Against decoder.decode(..., syntax="main", ...) with the options the case names - byte for byte,
record for record, err_offset for err_offset; no tolerance anywhere.  tests/test_plan_cases.py runs the same streams through the
host builds (which plan serially) and shows what every stream reaches.  Every decode is a probe, then a decode into exactly the room:
a buffer of FILL with guards around the frames, the source and the destination at byte offsets that are not aligned, the layouts going
round."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MAIN = 1
OPTIONS = ("decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools")


@pytest.fixture(scope="module")
def env():
    import plan_cases as P
    return P.M, P.D, P


def new_handle(M):
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    return e


@pytest.fixture(scope="module")
def enc(env):
    e = new_handle(env[0])
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, opt, layout="i420", es_off=0, dst_off=0, late=False):
    """one m2v_decode_device through the C-ABI (a probe for the size, then the decode into exactly that much) -> (frames or None, record);
    asserts the guards, and with a status other than OK that nothing was written (late: a refusal found behind the first chunk, whose
    pictures the call has written by then - nothing outside the room)"""
    import torch
    for name, v in zip(OPTIONS, opt):
        enc.set_option(name, int(bool(v)))
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    torch.cuda.synchronize()                                            # (the handle reads on a stream of its own: the source is whole before it does)
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES["iso"], None) == 0, enc._L.m2v_last_error(enc._h)
    r0 = enc.decode_report()
    room = int(r0["pictures"]) * int(r0["frame_bytes"]) if r0["status"] == D.OK else 4096
    buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES["iso"], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r = enc.decode_report()
    got = buf.cpu().numpy()
    a, b_ = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    if late and r["status"] != D.OK:
        b_ = a + room
    assert (got[:a] == D.FILL).all() and (got[b_:] == D.FILL).all(), "bytes outside the frames were written"
    assert (r0["status"], r0["err_offset"]) == (r["status"], r["err_offset"]) or r0["status"] == D.OK      # (the probe stops behind the plan)
    if r0["status"] == D.OK:
        assert (int(r0["pictures"]), int(r0["frame_bytes"]), int(r0["out_bytes"])) == (int(r["pictures"]), int(r["frame_bytes"]), room)
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0
        return None, r
    return got[a:b_].reshape(int(r["pictures"]), int(r["frame_bytes"])), r


def agree(env, enc, stream, opt, layout="i420", **kw):
    """the device answers what the definition answers -> the definition's Decoded, or None where both refuse at the same offset"""
    M, D, P = env
    d, at = P.spec_cached(stream, opt)
    got, r = decode(M, D, enc, stream, opt, layout, **kw)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), "pictures (display order) that differ: %s" % np.nonzero((got != want).any(axis=1))[0][:12]
    rec = P.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    return d


def test_edges(env, enc):
    """I B B P padded to 255 .. 769 start codes under k_db_plan: per 1, 2, 3 and 4, all lanes full, one event too few, half the lanes
    empty; 257 and 513 under the other four plans too (k_dm_plan refuses them at the first B picture)"""
    M, D, P = env
    for k, n in enumerate(P.EDGES):
        s = P.cases()["edge_%d" % n][0]
        assert agree(env, enc, s, P.B_, D.LAYOUTS[k & 3], es_off=1 + k % 5, dst_off=(3 * k + 1) % 7) is not None
    for k, n in enumerate((257, 513)):
        s = P.cases()["edge_%d" % n][0]
        others = [P.M_] + P.later_options(P.B_)
        assert [P.PLAN_OF[o] for o in others] == ["k_dm_plan", "k_di_plan", "k_dx_plan", "k_dt_plan"]
        for j, opt in enumerate(others):
            assert (agree(env, enc, s, opt, D.LAYOUTS[(k + j) & 3], es_off=3, dst_off=j + 1) is None) == (opt == P.M_)


@pytest.mark.parametrize("k", range(7))
def test_shift(env, enc, k):
    """k user_data units behind every sequence header: the ranges' edges pass through every position of a picture's units; with
    "decode_b_pictures" (k_db_plan), and with "decode_interlaced" at 16 x 32, progressive_sequence 0, two slices (k_di_plan)"""
    M, D, P = env
    assert k < P.SHIFT_PER
    for j, name in enumerate(("shift_%d" % k, "shift_%d_interlaced" % k)):
        s, L, opt, letters = P.cases()[name]
        assert agree(env, enc, s, opt, D.LAYOUTS[(k + j) & 3], es_off=1 + (k + j) % 4, dst_off=1 + (2 * k + j) % 6) is not None


@pytest.mark.parametrize("name", ("long_b", "long_m", "long_t", "long_x"))
def test_long(env, enc, name):
    """per 7 .. 13, three or four pictures a range, under the plan the case's options select and under every later option set that
    accepts it: all five single-stream plans meet long_b"""
    M, D, P = env
    s, L, opt, letters = P.cases()[name]
    for j, o in enumerate([opt] + P.later_options(opt)):
        assert agree(env, enc, s, o, D.LAYOUTS[j & 3], es_off=1 + j, dst_off=5 - j) is not None, o
    if name == "long_b":
        assert agree(env, enc, s, P.M_) is None                         # k_dm_plan: refused at the first B picture


def test_refusals(env, enc):
    """the status, the offset stated by hand, nothing written"""
    M, D, P = env
    for name, (s, opt, want) in sorted(P.refusals().items()):
        late = name == "gap_behind_first_chunk"                         # (found by the slice walk of the second chunk)
        if want is None:
            assert agree(env, enc, s, opt, es_off=1, dst_off=3) is not None, name
            continue
        got, r = decode(M, D, enc, s, opt, es_off=1, dst_off=3, late=late)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r, want)
        assert agree(env, enc, s, opt, late=late) is None


@pytest.mark.parametrize("part", range(4))
def test_altered(env, enc, part):
    """every altered stream (a quarter of the 120 per case): the definition's verdict, its earliest offset, its frames where it
    accepts - never a fault"""
    M, D, P = env
    cases = P.altered()
    assert len(cases) == 120
    for _, x in cases[30 * part:30 * part + 30]:
        agree(env, enc, x, P.B_, es_off=part, dst_off=1)


def test_decode_batch(env, enc):
    """"decode_batch" 0 (256 pictures a chunk), 7 and 100 on long_b and long_x: a chunk's edge between B pictures, identical bytes"""
    M, D, P = env
    try:
        for k, batch in enumerate((0, 7, 100)):
            enc.set_option("decode_batch", batch)
            for name in ("long_b", "long_x"):
                s, L, opt, letters = P.cases()[name]
                assert agree(env, enc, s, opt, D.LAYOUTS[k + 1], dst_off=k + 1) is not None
    finally:
        enc.set_option("decode_batch", 0)


def test_event_list_regrow(env):
    """long_b holds more start codes than the first guess of the event list: on a fresh handle the first call already answers right (the
    plan ran twice), and a second call on the same handle gives the same bytes"""
    M, D, P = env
    s, L, opt, letters = P.cases()["long_b"]
    assert len(M.decoder.start_codes(s)) > P.first_guess(len(s))
    e = new_handle(M)
    try:
        first, r1 = decode(M, D, e, s, opt)
        want = D.frames_of(P.spec_cached(s, opt)[0])
        assert first is not None and np.array_equal(first, want)
        second, r2 = decode(M, D, e, s, opt, dst_off=1)
        assert np.array_equal(second, want) and {k: int(r1[k]) for k in D.STAT_FIELDS} == {k: int(r2[k]) for k in D.STAT_FIELDS}
    finally:
        e.close()


def streams_call(M, X, enc, data, seg, flags, layout="i420"):
    """one m2v_decode_streams_main_device through the C-ABI: a probe, then into exactly the rooms -> ([record per stream], the output)"""
    import torch
    off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
    nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
    es = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda:0"), dev(data)])
    torch.cuda.synchronize()
    call = lambda dst, cap: enc._L.m2v_decode_streams_main_device(enc._h, es.data_ptr() + 1, off, nb, len(seg), dst, cap, M.LAYOUTS_420[layout], flags, None)
    assert call(None, 0) == 0, enc._L.m2v_last_error(enc._h)
    r0 = X.records_of(enc.decode_streams_report())
    total = max(r["out_offset"] + r["out_bytes"] for r in r0)
    buf = torch.full((2 * X.GUARD + 1 + total + 16,), X.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert call(buf.data_ptr() + X.GUARD + 1, total) == 0, enc._L.m2v_last_error(enc._h)
    recs = X.records_of(enc.decode_streams_report())
    got = buf.cpu().numpy()
    assert (got[:X.GUARD + 1] == X.FILL).all() and (got[X.GUARD + 1 + total:] == X.FILL).all(), "bytes outside the rooms were written"
    return recs, got[X.GUARD + 1:X.GUARD + 1 + total]


@pytest.mark.parametrize("flags", (3, 0))
def test_batch_entry(env, enc, flags):
    """k_dsm_plan with per >= 2 and B pictures: [short, long_b, short, shift_3 interlaced, edge_257] under flags 3 and, with long_m in
    long_b's place, flags 0 (which refuses what holds a B picture).  Each record is the stream's own m2v_decode_device record with the
    options as the flags say, the frames are packed one behind the other, and long_b's / long_m's are the definition's"""
    import decstreams_main_cases as X
    M, D, P = env
    c = P.cases()
    short = P._xw(16, 16, P.pictures("IPBB" if flags else "IPP", seed=51))[0]
    long_ = c["long_b" if flags else "long_m"][0]
    batch = [short, long_, short, c["shift_3_interlaced"][0], c["edge_257"][0]]
    data, seg = X.place(batch, b"\x00\x00\x01", lead=1)
    recs, out = streams_call(M, X, enc, data, seg, flags)
    opt = (flags & 1, flags >> 1 & 1, 0, 0)
    at = 0
    for b, s in enumerate(batch):
        frames, r1 = decode(M, D, enc, s, opt)
        assert {k: recs[b][k] for k in D.STAT_FIELDS} == {k: int(r1[k]) for k in D.STAT_FIELDS}, b
        assert recs[b]["es_offset"] == seg[b][0] and recs[b]["out_offset"] == at, b
        if frames is not None:
            assert np.array_equal(out[at:at + frames.size], frames.reshape(-1)), b
        at += recs[b]["out_bytes"]
    assert at == out.size
    assert [r["status"] for r in recs] == ([D.OK] * 5 if flags else [D.OK, D.OK, D.OK, D.SYNTAX, D.SYNTAX])
    want = D.frames_of(P.spec_cached(long_, opt)[0]).reshape(-1)
    assert np.array_equal(out[recs[1]["out_offset"]:recs[1]["out_offset"] + want.size], want)
