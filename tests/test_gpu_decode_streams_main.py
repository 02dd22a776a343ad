"""-m gpu: m2v_decode_streams_main_device - a batch of main-syntax streams in one call, B pictures and interlaced frame pictures by the
call's flags, a verdict per stream - against the model of tests/decstreams_main_cases.py (decoder.py composed stream by stream) and,
where stated, against m2v_decode_device on the same stream with the options set as the flags say: byte for byte and integer for
integer, no tolerance anywhere.  Every decode writes into a buffer filled with 0xA5 with GUARD bytes in front of and behind the rooms,
and every room that must stay untouched is looked at byte by byte.  tests/test_decstreams_main_cases.py runs the same batches through
the host build of the same arithmetic and shows that they hold what their names say.  Small shapes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4
GAP = b"\x00\x00\x01"


@pytest.fixture(scope="module")
def env():
    import decstreams_main_cases as X
    return X.M, X.D, X


@pytest.fixture(scope="module")
def enc(env):
    M, D, X = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def raw(M, enc, es_ptr, seg, dst_ptr, cap, layout, flags):
    """the C entry itself -> its answer"""
    off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
    nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
    return enc._L.m2v_decode_streams_main_device(enc._h, es_ptr, off, nb, len(seg), dst_ptr, cap, M.LAYOUTS_420[layout], flags, None)


def decode(env, enc, data, seg, flags=3, layout="i420", es_off=0, dst_off=0, cap=None, probe=False):
    """one m2v_decode_streams_main_device through the C-ABI: the data es_off bytes behind an aligned address, the output dst_off bytes
    behind one, GUARD bytes of FILL around the rooms.  -> ([dict per stream], the destination from its first GUARD byte on, the index of
    output byte 0 in it); cap None: exactly the rooms a probe reports"""
    import torch
    M, D, X = env
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(data)])
    ptr = es.data_ptr() + es_off
    assert raw(M, enc, ptr, seg, None, 0, layout, flags) == 0, enc._L.m2v_last_error(enc._h)
    r0 = X.records_of(enc.decode_streams_report())
    if probe:
        return r0, None, 0
    total = max(r["out_offset"] + r["out_bytes"] for r in r0)
    cap = total if cap is None else cap
    buf = torch.full((2 * X.GUARD + dst_off + max(cap, total) + 16,), X.FILL, dtype=torch.uint8, device="cuda:0")
    assert (buf.data_ptr() + X.GUARD) % 16 == 0
    torch.cuda.synchronize()
    assert raw(M, enc, ptr, seg, buf.data_ptr() + X.GUARD + dst_off, cap, layout, flags) == 0, enc._L.m2v_last_error(enc._h)
    assert enc._L.m2v_decode_streams_report(enc._h, None, 0) == len(seg)
    recs = X.records_of(enc.decode_streams_report())
    assert enc._L.m2v_decode_streams_report(enc._h, None, 0) == 0
    got = buf.cpu().numpy()
    assert (got[X.GUARD + dst_off + max(cap, total):] == X.FILL).all(), "bytes behind the destination were written"
    return recs, got[:X.GUARD + dst_off + max(cap, total)], X.GUARD + dst_off


def run(env, enc, batch, flags=3, layout="i420", cap=None, placed=None, **kw):
    M, D, X = env
    data, seg = placed or X.place(batch, GAP, lead=1)
    recs, buf, base = decode(env, enc, data, seg, flags, layout, cap=cap, **kw)
    want = X.expected(batch, flags, layout, cap=cap)
    X.check(recs, buf, want, base=base, segments=seg)
    out = buf[base:base + want["total"]]
    assert ((out != X.FILL) <= want["written"]).all(), "a byte outside the rooms of OK streams was written"
    return recs, buf[base:]


def single(env, enc, stream, flags, layout="i420"):
    """m2v_decode_device on one stream with "decode_syntax" = main and the options as the flags say -> (frames bytes or None, its
    record as a dict); the handle's options are put back"""
    import torch
    M, D, X = env
    held = [(k, enc._set.get(k, 0)) for k in ("decode_syntax", "decode_b_pictures", "decode_interlaced")]
    es = dev(stream) if len(stream) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    try:
        enc.set_option("decode_syntax", 1)
        enc.set_option("decode_b_pictures", flags & 1)
        enc.set_option("decode_interlaced", flags >> 1 & 1)
        assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(stream), None, 0, M.LAYOUTS_420[layout], 0, None) == 0
        r = enc.decode_report()
        if r["status"] != D.OK:
            return None, {k: int(r[k]) for k in D.STAT_FIELDS}
        out = torch.empty(int(r["out_bytes"]), dtype=torch.uint8, device="cuda:0")
        assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), len(stream), out.data_ptr(), out.numel(), M.LAYOUTS_420[layout], 0, None) == 0
        r = enc.decode_report()
        return (out.cpu().numpy() if r["status"] == D.OK else None), {k: int(r[k]) for k in D.STAT_FIELDS}
    finally:
        for k, v in held:
            enc.set_option(k, v)


def equals_single(env, enc, batch, recs, out, flags, layout="i420"):
    M, D, X = env
    for b, s in enumerate(batch):
        frames, r1 = single(env, enc, s, flags, layout)
        assert {k: recs[b][k] for k in D.STAT_FIELDS} == r1, b
        if frames is not None:
            assert np.array_equal(out[recs[b]["out_offset"]:recs[b]["out_offset"] + frames.size], frames), b


@pytest.mark.parametrize("name", ("mixed", "mixed_reversed"))
def test_mixed(env, enc, name):
    """sizes 1 x 1 .. 64 x 64, B pictures, field pictures (four macroblock rows at 48 lines), the oracle's stream, two pairs of matrices
    side by side, both scans, both scale types, precisions, f_code 3, a repeated header: the lanes of one wavefront of the walk hold
    slices of different streams.  Every layout; each stream's record and frames are also m2v_decode_device's for it alone"""
    M, D, X = env
    batch, flags = X.batches()[name]
    for layout in D.LAYOUTS:
        recs, out = run(env, enc, batch, flags, layout, dst_off=D.LAYOUTS.index(layout) * 5)
    equals_single(env, enc, batch, recs, out, flags, D.LAYOUTS[-1])


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_flags(env, enc, flags):
    """the mixed batch under each flag combination: without its flag a B picture / frame_pred_frame_dct 0 is a probe-stage refusal that
    takes no room, and the offsets behind it shift; the probe reports the decode's layout"""
    M, D, X = env
    batch = X.mixed()
    recs, out = run(env, enc, batch, flags)
    equals_single(env, enc, batch, recs, out, flags)
    data, seg = X.place(batch, GAP, lead=1)
    probe, _, _ = decode(env, enc, data, seg, flags, probe=True)
    want = X.expected(batch, flags, probe=True)["records"]
    assert [(r["out_offset"], r["out_bytes"], r["status"]) for r in probe] == [(w["out_offset"], w["out_bytes"], w["status"]) for w in want]


def test_verdicts_are_independent(env, enc):
    """OK, a grammar refusal, a leading B picture, slice refusals in an anchor, in a B picture and in a field macroblock, an empty and a
    3-byte segment, a truncated stream - each between good streams: the neighbours' bytes are right, the refused rooms untouched"""
    M, D, X = env
    batch = [s for _, s in X.verdicts()]
    for layout in ("i420", "nv12"):
        recs, out = run(env, enc, batch, 3, layout, dst_off=3)
    equals_single(env, enc, batch, recs, out, 3, "nv12")


@pytest.mark.parametrize("seed", (31, 32))
def test_altered(env, enc, seed):
    """64 seeded alterations of a small interlaced I P B B stream as one batch: every verdict and err_offset is the definition's"""
    M, D, X = env
    batch = X.altered(seed)
    assert len(batch) == 64
    run(env, enc, batch, 3)


def test_chunks(env, enc):
    """I P B B P B B, an I-only stream and two I / P streams at "decode_batch" 1, 2, 3, 5 and the default: anchors carried across one
    and two cuts, B pictures cut off from their anchors, another stream behind a cut one - identical results, each the single call's"""
    M, D, X = env
    batch = X.chunks()
    results = []
    try:
        for k in X.DECODE_BATCHES:
            enc.set_option("decode_batch", k)
            recs, out = run(env, enc, batch, 3)
            results.append(out.tobytes())
        assert len(set(results)) == 1
        enc.set_option("decode_batch", 2)
        run(env, enc, batch, 3, "nv21", dst_off=7)
        run(env, enc, [s for _, s in X.verdicts()], 3)
    finally:
        enc.set_option("decode_batch", 0)
    equals_single(env, enc, batch, recs, out, 3)


def test_late_refusal_writes_nothing(env, enc):
    """a stream lying in several chunks ("decode_batch" 2) is refused in its last slice: nothing of it is written"""
    M, D, X = env
    batch, last = X.late()
    try:
        enc.set_option("decode_batch", 2)
        recs, _ = run(env, enc, batch, 3)
    finally:
        enc.set_option("decode_batch", 0)
    assert (recs[1]["status"], recs[1]["err_offset"], recs[1]["out_bytes"]) == (D.SYNTAX, last, 0)
    run(env, enc, batch, 3)


def test_cap(env, enc):
    """cap one byte short of the third stream's room: it and the one behind it are OVERFLOW, the two in front are written, nothing at
    or past cap; the probe reports the same layout"""
    M, D, X = env
    batch = X.cap_batch()
    want = X.expected(batch, 3)
    total, offs = want["total"], [w["out_offset"] for w in want["records"]]
    data, seg = X.place(batch, GAP, lead=1)
    probe, _, _ = decode(env, enc, data, seg, 3, probe=True)
    assert [r["out_offset"] for r in probe] == offs
    for cap, st in ((total, [None] * 4), (offs[3] - 1, [None, None, "cap", "cap"]), (offs[1], [None, "cap", "cap", "cap"]), (0, ["cap"] * 4)):
        recs, _ = run(env, enc, batch, 3, cap=cap, dst_off=1)
        assert [r["status"] for r in recs] == [D.OVERFLOW if s else D.OK for s in st] and [r["out_offset"] for r in recs] == offs


def test_alignment(env, enc):
    """sixteen streams at segment offsets 0 .. 15 mod 16 with start codes in the gaps and across both edges of every segment; the
    destination 1 and 7 bytes behind an aligned address with frame_bytes 3 and 384 in turn, all four layouts"""
    M, D, X = env
    streams, data, seg = X.alignment()
    for dst_off in (1, 7, 0):
        for layout in D.LAYOUTS:
            run(env, enc, streams, 3, layout, placed=(data, seg), dst_off=dst_off)
    run(env, enc, streams, 0, "i420", placed=(data, seg), es_off=5, dst_off=9)


def test_event_list_too_small_beside_others(env, enc):
    """300 pictures of 16 x 16 with user_data - more start codes than the list is guessed to hold - between two small streams: the scan
    runs a second time, for all three"""
    M, D, X = env
    batch, flags = X.batches()["events"]
    assert len(X.decoder.start_codes(batch[1])) > X.event_guess(len(batch[1]))
    run(env, enc, batch, flags)
    run(env, enc, batch, 3, "nv21")


def test_many_streams(env, enc):
    """4096 streams of 16 x 16 in one chunk, every 64th an I P B B stream: every out_offset, every frame at its display index"""
    M, D, X = env
    batch, flags = X.batches()["many"]
    recs, _ = run(env, enc, batch, flags, placed=X.place(batch, b"", lead=0))
    assert recs[64]["out_offset"] == 384 * (63 + 4)


def test_the_entry_rules(env, enc):
    """unknown flag bits, nstreams 0 and 65536: M2V_E_PARAM and nothing touched; M2V_E_STATE between encode_resident_begin and _end with
    no byte written and the next legal call right; the handle's three syntax options change nothing and are not changed; after each,
    m2v_decode_device and the module's batch entry answer as before"""
    import torch
    M, D, X = env
    import decstreams_cases as S
    batch = X.chunks()
    data, seg = X.place(batch, GAP, lead=1)
    d = dev(data)
    want = X.expected(batch, 3)
    out = torch.full((want["total"],), X.FILL, dtype=torch.uint8, device="cuda:0")

    def unchanged(e):
        assert (out.cpu().numpy() == X.FILL).all()
        small = S.batches()["smallest"]
        sd, sseg = S.place(small, b"", lead=0)
        frames, recs = e.decode_streams(dev(sd), sseg)
        S.check(S.records_of(recs), frames.cpu().numpy(), S.expected(small), segments=sseg)
        f1, r1 = e.decode_device(dev(X.ipbbpbb()[0]), syntax="main", b_pictures=True)
        assert np.array_equal(f1.cpu().numpy().reshape(-1), X.D.frames_of(X.alone(X.ipbbpbb()[0], 1)["decoded"]).reshape(-1))

    one = (ctypes.c_uint64 * 1)(0)
    for bad in (4, 8, 0x80000000, 7):
        assert raw(M, enc, d.data_ptr(), seg, out.data_ptr(), out.numel(), "i420", bad) == E_PARAM
        assert b"m2v_decode_streams_main_device" in enc._L.m2v_last_error(enc._h)
        unchanged(enc)
    for n in (0, 65536):
        assert enc._L.m2v_decode_streams_main_device(enc._h, d.data_ptr(), one, one, n, None, 0, 0, 3, None) == E_PARAM
    unchanged(enc)
    # the handle's options: the result does not depend on them, and they stay
    base = None
    for syntax, b, i in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)):
        try:
            enc.set_option("decode_syntax", syntax)
            enc.set_option("decode_b_pictures", b)
            enc.set_option("decode_interlaced", i)
            recs, got = run(env, enc, batch, 3)
            base = base or got.tobytes()
            assert got.tobytes() == base
            assert [enc._set.get(k, 0) for k in ("decode_syntax", "decode_b_pictures", "decode_interlaced")] == [syntax, b, i]
            if syntax:                          # the module's batch entry is still pinned to M2V_E_STATE there, and touches nothing
                off, nb = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg]), (ctypes.c_uint64 * len(seg))(*[n for _, n in seg])
                assert enc._L.m2v_decode_streams_device(enc._h, d.data_ptr(), off, nb, len(seg), out.data_ptr(), out.numel(), 0, 0, None) == E_STATE
                assert (out.cpu().numpy() == X.FILL).all()
        finally:
            for k in ("decode_syntax", "decode_b_pictures", "decode_interlaced"):
                enc.set_option(k, 0)
    unchanged(enc)
    # a resident call in flight
    e = M.Mpeg2Encoder(XL=4, YL=4)
    try:
        f444 = M.synth.clip(64, 64, 2, clip_index=3)
        d_in = torch.from_numpy(f444.reshape(2, -1).copy()).to("cuda:0")
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        e.encode_resident_begin(d_in.data_ptr(), 2, d_out.data_ptr(), d_out.numel(), 4, 4, 1)
        assert raw(M, e, d.data_ptr(), seg, out.data_ptr(), out.numel(), "i420", 3) == E_STATE
        e.encode_resident_end()
        unchanged(e)
        frames, recs = e.decode_streams(d, seg, out=out, syntax="main", b_pictures=True, interlaced=True)
        X.check(X.records_of(recs), out.cpu().numpy(), want, segments=seg)
        assert torch.equal(M.frames_of_stream(frames, recs[1]).reshape(-1), frames[int(recs[1]["out_offset"]):int(recs[2]["out_offset"])])
    finally:
        e.close()


@pytest.mark.parametrize("kind", ("ts", "ps"))
def test_containers(env, enc, kind):
    """the streams of the chunks batch in containers of tests/demux_writer.py, through decode_streams(container=, syntax="main",
    b_pictures=True, interlaced=True): demultiplexed and decoded on the device"""
    import demux_writer as DW
    M, D, X = env
    batch = list(X.chunks()) + [X.field48()[0]]
    boxes = [containers(DW, kind, s) for s in batch]
    data, seg = X.place(boxes, b"", lead=0)
    frames, recs = enc.decode_streams(dev(data), seg, container=kind, syntax="main", b_pictures=True, interlaced=True)
    want = X.expected(batch, 3)
    got = X.records_of(recs)
    for g, w in zip(got, want["records"]):
        assert (g["status"], g["pictures"], g["out_offset"], g["out_bytes"]) == (w["status"], w["pictures"], w["out_offset"], w["out_bytes"])
    assert np.array_equal(frames.cpu().numpy(), want["out"])
    assert [enc._set.get(k, 0) for k in ("decode_syntax", "decode_b_pictures", "decode_interlaced")] == [0, 0, 0]


def containers(DW, kind, stream):
    """the stream in a transport stream (PAT, PMT, one video PID, 184-byte payloads) or a program stream (a pack, a system header, PES
    packets of 1000 bytes, the end code) written with tests/demux_writer.py's units"""
    if kind == "ts":
        w = DW.TsWriter(5, video_pid=0x120)
        w.psi(0, DW.pat_section([(1, 0x1000)]))
        w.psi(0x1000, DW.pmt_section(1, 0x120, [(0x02, 0x120, b"")]))
        head = DW.pes_header(0xE0, 0, pts=9000, dts=None)
        data = head + stream
        w.video(data[:150], pusi=1, head=len(head), stamp=(9000, DW.ABSENT))
        for at in range(150, len(data), 184):
            w.video(data[at:at + 184])
        assert w.expect()["es"] == stream
        return w.bytes()
    w = DW.PsWriter(3)
    w.pack()
    w.system_header()
    for at in range(0, len(stream), 1000):
        part = stream[at:at + 1000]
        pts = 9000 if at == 0 else None
        n = len(DW.pes_header(0xE0, 0, pts=pts)) - 6 + len(part)
        w._unit(DW.pes_header(0xE0, n, pts=pts) + part)
    w.end()
    return w.bytes()


def test_python_keywords(env, enc):
    """the ValueErrors of the keywords; the defaults are today's calls; the probe-then-allocate path and frames_of_stream with syntax="main\""""
    M, D, X = env
    batch = X.chunks()
    data, seg = X.place(batch, GAP, lead=1)
    d = dev(data)
    for kw in (dict(mode="module", syntax="main"), dict(b_pictures=True), dict(interlaced=True), dict(syntax="module", b_pictures=True), dict(syntax="iso"),
               dict(syntax=None)):
        with pytest.raises(ValueError):
            enc.decode_streams(d, seg, **kw)
    frames, recs = enc.decode_streams(d, seg, syntax="main", b_pictures=True)
    want = X.expected(batch, 1)
    X.check(X.records_of(recs), frames.cpu().numpy(), want, segments=seg)
    for b in range(len(batch)):
        r = want["records"][b]
        assert np.array_equal(M.frames_of_stream(frames, recs[b]).cpu().numpy().reshape(-1), want["out"][r["out_offset"]:r["out_offset"] + r["out_bytes"]])
    # with the defaults the module's entry: a main-syntax B stream is refused there as ever
    _, recs = enc.decode_streams(d, seg)
    assert int(recs["rec"]["status"][0]) == D.SYNTAX
