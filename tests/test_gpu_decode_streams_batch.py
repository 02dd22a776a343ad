"""-m gpu: m2v_decode_streams_device - a batch of streams of any sizes in one call, a verdict per stream - against the model of
tests/decstreams_cases.py (decoder.py composed stream by stream) and, where stated, against m2v_decode_device on the same stream:
byte for byte and integer for integer, no tolerance anywhere.  Every decode writes into a buffer filled with 0xA5 with GUARD bytes in
front of and behind the rooms, and every room that must stay untouched is looked at byte by byte.  tests/test_decstreams_cases.py
runs the same batches through the host build of the same arithmetic and shows that they hold what their names say.  Small shapes;
what each case is for is in its docstring."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4


@pytest.fixture(scope="module")
def env():
    import decstreams_cases as S
    return S.M, S.D, S


@pytest.fixture(scope="module")
def enc(env):
    M, D, S = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def raw(M, D, enc, es_ptr, seg, dst_ptr, cap, layout, mode):
    """the C entry itself -> its answer"""
    off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
    nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
    return enc._L.m2v_decode_streams_device(enc._h, es_ptr, off, nb, len(seg), dst_ptr, cap, M.LAYOUTS_420[layout], D.MODES[mode], None)


def decode(env, enc, data, seg, layout="i420", mode="iso", es_off=0, dst_off=0, cap=None, probe=False):
    """one m2v_decode_streams_device through the C-ABI: the data es_off bytes behind an aligned address, the output dst_off bytes behind
    one, GUARD bytes of FILL around the rooms.  -> ([dict per stream], the destination from its first GUARD byte on, the index of output
    byte 0 in it); cap None: exactly the rooms a probe reports"""
    import torch
    M, D, S = env
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(data)])
    ptr = es.data_ptr() + es_off
    assert raw(M, D, enc, ptr, seg, None, 0, layout, mode) == 0, enc._L.m2v_last_error(enc._h)
    r0 = S.records_of(enc.decode_streams_report())
    if probe:
        return r0, None, 0
    total = max(r["out_offset"] + r["out_bytes"] for r in r0)
    cap = total if cap is None else cap
    buf = torch.full((2 * S.GUARD + dst_off + max(cap, total) + 16,), S.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert raw(M, D, enc, ptr, seg, buf.data_ptr() + S.GUARD + dst_off, cap, layout, mode) == 0, enc._L.m2v_last_error(enc._h)
    assert enc._L.m2v_decode_streams_report(enc._h, None, 0) == len(seg)
    recs = S.records_of(enc.decode_streams_report())
    assert enc._L.m2v_decode_streams_report(enc._h, None, 0) == 0
    got = buf.cpu().numpy()
    assert (got[S.GUARD + dst_off + max(cap, total):] == S.FILL).all(), "bytes behind the destination were written"
    return recs, got[:S.GUARD + dst_off + max(cap, total)], S.GUARD + dst_off


def run(env, enc, batch, layout="i420", mode="iso", gap=b"\x00\x00\x01", lead=1, cap=None, **kw):
    M, D, S = env
    data, seg = S.place(batch, gap, lead=lead)
    recs, buf, base = decode(env, enc, data, seg, layout, mode, cap=cap, **kw)
    S.check(recs, buf, S.expected(batch, layout, mode, cap=cap), base=base, segments=seg)
    return recs


def single(env, enc, stream, layout, mode):
    """m2v_decode_device on one stream -> (frames bytes or None, its record as a dict)"""
    import torch
    M, D, S = env
    es = dev(stream) if len(stream) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES[mode], None) == 0
    r = enc.decode_report()
    if r["status"] != D.OK:
        return None, {k: int(r[k]) for k in D.STAT_FIELDS}
    out = torch.empty(int(r["out_bytes"]), dtype=torch.uint8, device="cuda:0")
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(stream), out.data_ptr(), out.numel(), M.LAYOUTS_420[layout], D.MODES[mode], None) == 0
    r = enc.decode_report()
    return (out.cpu().numpy() if r["status"] == D.OK else None), {k: int(r[k]) for k in D.STAT_FIELDS}


def recon_names():
    import dec_cases
    return dec_cases.recon_names()


@pytest.mark.parametrize("name", recon_names())
def test_batch_of_one_equals_the_single_call(env, enc, name):
    """every stream of dec_cases.recon_streams() as a batch of one: bytes and rec are m2v_decode_device's"""
    M, D, S = env
    c = D.recon_streams()[name]
    mode = "iso" if c["conformant"] else "module"
    want, r1 = single(env, enc, c["stream"], "i420", mode)
    recs, buf, base = decode(env, enc, c["stream"], [(0, len(c["stream"]))], "i420", mode)
    assert {k: recs[0][k] for k in D.STAT_FIELDS} == r1 and recs[0]["out_offset"] == 0 and recs[0]["es_offset"] == 0
    assert np.array_equal(buf[base:base + want.size], want) and (buf[:base] == S.FILL).all() and (buf[base + want.size:] == S.FILL).all()
    assert np.array_equal(want.reshape(r1["pictures"], -1), D.expected_from_dump(c, "i420"))


def test_smallest_batch(env, enc):
    """small(7) and small(8), 32 x 32, I + P: all four layouts, both modes"""
    M, D, S = env
    for mode, _ in S.BOTH:
        for layout in D.LAYOUTS:
            run(env, enc, S.batches()["smallest"], layout, mode)


@pytest.mark.parametrize("name", ("mixed", "mixed_reversed"))
def test_mixed_sizes(env, enc, name):
    """1 x 1 (frame_bytes 3: the next stream starts at an odd output address), 32 x 32, 17 x 33, 64 x 64 and 80 x 112 (40-byte chroma
    rows) in one call, both orders, the destination at every misalignment"""
    M, D, S = env
    for dst_off in range(16):
        run(env, enc, S.batches()[name], D.LAYOUTS[dst_off & 3], ("iso", "module")[(dst_off >> 2) & 1], dst_off=dst_off)


def test_segment_edges(env, enc):
    """the source at every misalignment; gaps filled with start codes placed so that each would straddle either edge of a segment;
    segments touching; a segment that ends exactly at a scan-tile edge; one that starts 1 .. 3 bytes before one"""
    M, D, S = env
    T = M.decode_scan_tile()
    batch = S.batches()["three"]
    for es_off in range(16):
        run(env, enc, batch, es_off=es_off)
    for code in (b"\x00\x00\x01\xb3", b"\x00\x00\x01\x00", b"\x00\x00\x01\xb7"):
        for k in (1, 2, 3):                      # the gap ends with the code's first k bytes and begins with its last 4 - k
            run(env, enc, batch, gap=code[k:] + b"\xff" * 5 + code[:k])
        run(env, enc, batch, gap=code)
    run(env, enc, batch, gap=b"")                # touching
    # small + zeros to a multiple of 32 is still the stream: pad the first so that it ends exactly at a tile's edge
    first = batch[0] + bytes(T - len(batch[0]))
    assert len(first) == T
    run(env, enc, [first, batch[1]], gap=b"", lead=0)
    for k in (1, 2, 3):                          # the first segment starts k bytes before a multiple of the tile in the tensor
        run(env, enc, batch, gap=b"", lead=T - k)


def test_verdicts_are_independent(env, enc):
    """[small, picture_type_3, small(8), a slice-stage refusal, sized(17, 33), cut_in_header, b"", small]: each record equals the single
    call's, OK streams are byte-exact, the slice-stage room is untouched, probe-stage refusals take no room, the probe reports the same
    layout; and two_bad_slices() between two good streams: err_offset is the earlier slice, relative to the stream"""
    M, D, S = env
    for name in ("verdicts", "two_bad"):
        batch = S.batches()[name]
        for mode in ("iso", "module"):
            recs = run(env, enc, batch, "i420", mode)
            for b, s in enumerate(batch):
                _, r1 = single(env, enc, s, "i420", mode)
                assert {k: recs[b][k] for k in D.STAT_FIELDS} == r1, (name, mode, b)
            data, seg = S.place(batch, b"\x00\x00\x01", lead=1)
            probe, _, _ = decode(env, enc, data, seg, "i420", mode, probe=True)
            assert [r["out_offset"] for r in probe] == [r["out_offset"] for r in recs]
            want = S.expected(batch, "i420", mode, probe=True)["records"]
            assert [(r["out_bytes"], r["status"]) for r in probe] == [(w["out_bytes"], w["status"]) for w in want]
    recs = run(env, enc, S.batches()["two_bad"])
    assert (recs[1]["status"], recs[1]["err_offset"], recs[1]["out_bytes"]) == (D.SYNTAX, D.two_bad_slices()[1], 0)
    stages = [w["stage"] for w in S.expected(S.batches()["verdicts"])["records"]]
    assert stages == [None, "probe", None, "slice", None, "probe", "probe", None]


def test_cap(env, enc):
    """three streams; cap of exactly the total, total - 1, the middle of stream 1's room, 0: OVERFLOW exactly where the rule says, the
    streams that fit are written, nothing at or past cap"""
    M, D, S = env
    batch = S.batches()["three"]
    want = S.expected(batch)
    total, rooms = want["total"], [w["out_offset"] for w in want["records"]]
    for cap, stages in ((total, [None, None, None]), (total - 1, [None, None, "cap"]), ((rooms[1] + rooms[2]) // 2, [None, "cap", "cap"]), (0, ["cap"] * 3)):
        assert [w["stage"] for w in S.expected(batch, cap=cap)["records"]] == stages
        recs = run(env, enc, batch, cap=cap, dst_off=3)
        assert [r["status"] for r in recs] == [D.OVERFLOW if st else D.OK for st in stages]


def test_chunk_cuts(env, enc):
    """[I P P of 32 x 32, I P of 64 x 64, 62 I pictures of 64 x 64, small] with "decode_batch" 1, 2, 3, 5 and the default: cuts between an
    I picture and its P picture, at a stream boundary where the size changes, inside a run of chains (test_decstreams_cases.py shows
    where each option cuts); and the batch with refusals, whose slice-stage one then lies in two chunks"""
    M, D, S = env
    try:
        for k in (1, 2, 3, 5, 0):
            enc.set_option("decode_batch", k)
            run(env, enc, S.batches()["chunks"], ("i420", "nv12")[k & 1], ("module", "iso")[k & 1])
        enc.set_option("decode_batch", 1)
        run(env, enc, S.batches()["verdicts"])
        enc.set_option("decode_batch", 7)
        run(env, enc, S.batches()["two_bad"])
    finally:
        enc.set_option("decode_batch", 0)


def test_event_list_too_small_beside_others(env, enc):
    """dec_writer.many_pictures() - 400 pictures in 11 KB, more start codes than its list is guessed to hold - between two small
    streams: the scan runs a second time, for all three"""
    M, D, S = env
    batch = S.batches()["events"]
    assert D.prefixes(batch[1]) > max(256, len(batch[1]) // 16 + 64)
    run(env, enc, batch, "i420", "iso")
    run(env, enc, batch, "nv21", "module")


def test_many_streams_and_the_entry_rules(env, enc):
    """4096 copies of one one-picture 16 x 16 stream in one call: the tiling of one decode, every out_offset; nstreams 0 and 65536 are
    M2V_E_PARAM; a call while a resident _begin is open is M2V_E_STATE with no output byte changed, and the next legal call is right"""
    import torch
    M, D, S = env
    batch = S.batches()["many"]
    recs = run(env, enc, batch, gap=b"", lead=0)
    assert [r["out_offset"] for r in recs] == [384 * b for b in range(4096)]
    one = (ctypes.c_uint64 * 1)(0)
    es = dev(batch[0])
    for n in (0, 65536):
        assert enc._L.m2v_decode_streams_device(enc._h, es.data_ptr(), one, one, n, None, 0, 0, 0, None) == E_PARAM
    e = M.Mpeg2Encoder(XL=4, YL=4)
    try:
        data, seg = S.place(S.batches()["smallest"], b"", lead=0)
        d = dev(data)
        out = torch.full((2 * 6144,), S.FILL, dtype=torch.uint8, device="cuda:0")
        f444 = M.synth.clip(64, 64, 2, clip_index=3)
        d_in = torch.from_numpy(f444.reshape(2, -1).copy()).to("cuda:0")
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        e.encode_resident_begin(d_in.data_ptr(), 2, d_out.data_ptr(), d_out.numel(), 4, 4, 1)
        assert raw(M, D, e, d.data_ptr(), seg, out.data_ptr(), 6144, "i420", "iso") == E_STATE
        e.encode_resident_end()
        assert (out.cpu().numpy() == S.FILL).all()
        frames, recs = e.decode_streams(d, seg, out=out[:6144])
        want = S.expected(S.batches()["smallest"])
        S.check(S.records_of(recs), out.cpu().numpy()[:6144], want, segments=seg)
        assert (out.cpu().numpy()[6144:] == S.FILL).all()
        assert torch.equal(M.frames_of_stream(frames, recs[1]).reshape(-1), frames[3072:6144])
        with pytest.raises(ValueError):
            e.decode_streams(d, [])
        with pytest.raises(ValueError):
            e.decode_streams(d, [(0, d.numel() + 1)])
        with pytest.raises(ValueError):
            e.decode_streams(d, seg, stream=0x100)
    finally:
        e.close()


def test_the_loop_closed(env):
    """encode_batch of 3 clips x 3 frames of 64 x 64, "conformant", recon "i420" -> decode_streams(mode "iso"): the frames are the
    reconstruction buffer, a [B, N, frame_bytes] tensor.  The same through container "ts" and "ps", with one container altered so that
    the demultiplexer refuses it: its record is SYNTAX with no pictures, the others' frames are still the reconstruction"""
    import torch
    M, D, S = env
    e = M.Mpeg2Encoder(XL=4, YL=4)
    try:
        e.set_option("conformant", 1)
        x = torch.from_numpy(np.random.RandomState(21).randint(0, 256, size=(3, 3, 64, 64, 3)).astype(np.uint8)).to("cuda:0")
        stream, offsets, recon = e.encode_batch(x, 2, recon="i420")
        seg = [(offsets[b], offsets[b + 1] - offsets[b]) for b in range(3)]
        frames, recs = e.decode_streams(stream, seg, mode="iso")
        assert (recs["rec"]["status"] == D.OK).all() and list(recs["out_offset"]) == [0, 3 * 6144, 6 * 6144] and list(recs["es_offset"]) == [a for a, _ in seg]
        assert torch.equal(frames.reshape(3, 3, 6144), recon.reshape(3, 3, 6144))
        for b in range(3):
            assert torch.equal(M.frames_of_stream(frames, recs[b]), recon.reshape(3, 3, 6144)[b])
        for kind in ("ts", "ps"):
            box, where, recon = e.encode_batch(x, 2, recon="i420", container=kind)
            frames, recs = e.decode_streams(box, where, mode="iso", container=kind)
            assert (recs["rec"]["status"] == D.OK).all() and torch.equal(frames.reshape(3, 3, 6144), recon.reshape(3, 3, 6144)), kind
            bad = box.clone()
            bad[where[1][0]] = 0xFF              # neither a transport packet's sync byte nor the first byte of a pack start code
            frames, recs = e.decode_streams(bad, where, mode="iso", container=kind)
            assert [int(v) for v in recs["rec"]["status"]] == [D.OK, D.SYNTAX, D.OK] and int(recs["rec"]["pictures"][1]) == 0, kind
            assert list(recs["out_offset"]) == [0, 3 * 6144, 3 * 6144] and frames.numel() == 6 * 6144
            assert torch.equal(frames.reshape(2, 3, 6144), recon.reshape(3, 3, 6144)[[0, 2]]), kind
    finally:
        e.close()
