"""-m gpu: m2v_decode_streams_main_ex_device - a batch of main-syntax streams in one call with the extended options (several slices a
row, slice extras, quant_matrix_extension; Table B-15, concealment vectors, dual prime) by the call's flags, a verdict per stream -
against the model of tests/decstreams_ex_cases.py (decoder.py composed stream by stream) and, where stated, against m2v_decode_device on
the same stream with the four options set as the flags say: byte for byte and integer for integer, no tolerance anywhere.  Every decode
writes into a buffer filled with 0xA5 with GUARD bytes in front of and behind the rooms, and every room that must stay untouched is
looked at byte by byte.  tests/test_decstreams_ex_cases.py runs the same batches through the host build of the same arithmetic - the
altered streams under AddressSanitizer as a stand-alone program - and shows that they hold what their names say.  Small shapes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4
GAP = b"\x00\x00\x01"
OPTIONS = ("decode_syntax", "decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools")


@pytest.fixture(scope="module")
def env():
    import decstreams_ex_cases as X
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


def raw(M, enc, es_ptr, seg, dst_ptr, cap, layout, flags, entry="m2v_decode_streams_main_ex_device"):
    """the C entry itself -> its answer"""
    off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
    nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
    return getattr(enc._L, entry)(enc._h, es_ptr, off, nb, len(seg), dst_ptr, cap, M.LAYOUTS_420[layout], flags, None)


def decode(env, enc, data, seg, flags=15, layout="i420", es_off=0, dst_off=0, cap=None, probe=False, entry="m2v_decode_streams_main_ex_device"):
    """one call through the C-ABI: the data es_off bytes behind an aligned address, the output dst_off bytes behind one, GUARD bytes of
    FILL around the rooms.  -> ([dict per stream], the destination from its first GUARD byte on, the index of output byte 0 in it); cap
    None: exactly the rooms a probe reports"""
    import torch
    M, D, X = env
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(data)])
    ptr = es.data_ptr() + es_off
    assert raw(M, enc, ptr, seg, None, 0, layout, flags, entry) == 0, enc._L.m2v_last_error(enc._h)
    r0 = X.records_of(enc.decode_streams_report())
    if probe:
        return r0, None, 0
    total = max(r["out_offset"] + r["out_bytes"] for r in r0)
    cap = total if cap is None else cap
    buf = torch.full((2 * X.GUARD + dst_off + max(cap, total) + 16,), X.FILL, dtype=torch.uint8, device="cuda:0")
    assert (buf.data_ptr() + X.GUARD) % 16 == 0
    torch.cuda.synchronize()
    assert raw(M, enc, ptr, seg, buf.data_ptr() + X.GUARD + dst_off, cap, layout, flags, entry) == 0, enc._L.m2v_last_error(enc._h)
    assert enc._L.m2v_decode_streams_report(enc._h, None, 0) == len(seg)
    recs = X.records_of(enc.decode_streams_report())
    assert enc._L.m2v_decode_streams_report(enc._h, None, 0) == 0
    got = buf.cpu().numpy()
    assert (got[X.GUARD + dst_off + max(cap, total):] == X.FILL).all(), "bytes behind the destination were written"
    return recs, got[:X.GUARD + dst_off + max(cap, total)], X.GUARD + dst_off


def run(env, enc, batch, flags=15, layout="i420", cap=None, placed=None, **kw):
    M, D, X = env
    data, seg = placed or X.place(batch, GAP, lead=1)
    recs, buf, base = decode(env, enc, data, seg, flags, layout, cap=cap, **kw)
    want = X.expected(batch, flags, layout, cap=cap)
    X.check(recs, buf, want, base=base, segments=seg)
    out = buf[base:base + want["total"]]
    assert ((out != X.FILL) <= want["written"]).all(), "a byte outside the rooms of OK streams was written"
    return recs, buf[base:]


def single(env, enc, stream, flags, layout="i420"):
    """m2v_decode_device on one stream with "decode_syntax" = main and the four options as the flags say -> (frames bytes or None, its
    record as a dict); the handle's options are put back"""
    import torch
    M, D, X = env
    held = [(k, enc._set.get(k, 0)) for k in OPTIONS]
    es = dev(stream) if len(stream) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    try:
        for k, v in zip(OPTIONS, (1, flags & 1, flags >> 1 & 1, flags >> 2 & 1, flags >> 3 & 1)):
            enc.set_option(k, v)
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
    seen = {}
    for b, s in enumerate(batch):
        if bytes(s) not in seen:
            seen[bytes(s)] = single(env, enc, s, flags, layout)
        frames, r1 = seen[bytes(s)]
        assert {k: recs[b][k] for k in D.STAT_FIELDS} == r1, b
        if frames is not None:
            assert np.array_equal(out[recs[b]["out_offset"]:recs[b]["out_offset"] + frames.size], frames), b


def test_tools(env, enc):
    """every valid stream of ext_cases and mbt_cases - rows cut into slices, slice extras, matrices per picture, Table B-15, concealment
    vectors, dual prime - interleaved with plain main, B and interlaced streams of other sizes: the lanes of one wavefront of the walk
    hold slice events of different streams.  Every layout; each stream's record and frames are also m2v_decode_device's for it alone"""
    M, D, X = env
    batch, flags = X.batches()["tools"]
    for layout in D.LAYOUTS:
        recs, out = run(env, enc, batch, flags, layout, dst_off=D.LAYOUTS.index(layout) * 5)
    equals_single(env, enc, batch, recs, out, flags, D.LAYOUTS[-1])


def test_flags(env, enc):
    """one mixed batch under every legal flag value: what a flag does not accept is a probe-stage refusal that takes no room (Table B-15
    and concealment vectors under 4 .. 7, at the coding extension), and the offsets behind it shift; the probe reports the decode's
    layout; flags 0 .. 3 are m2v_decode_streams_main_device's bytes and records"""
    M, D, X = env
    batch = X.mixed()
    data, seg = X.place(batch, GAP, lead=1)
    for flags in X.LEGAL_FLAGS:
        recs, out = run(env, enc, batch, flags)
        equals_single(env, enc, batch, recs, out, flags)
        probe, _, _ = decode(env, enc, data, seg, flags, probe=True)
        want = X.expected(batch, flags, probe=True)["records"]
        assert [(r["out_offset"], r["out_bytes"], r["status"]) for r in probe] == [(w["out_offset"], w["out_bytes"], w["status"]) for w in want]
        if flags < 4:
            old, buf, base = decode(env, enc, data, seg, flags, entry="m2v_decode_streams_main_device")
            assert old == recs and buf[base:].tobytes() == out.tobytes()


def test_verdicts_are_independent(env, enc):
    """the 30 hand-stated refusals of ext_cases and the 24 of mbt_cases, each between two good streams, under flags 15 and 7: probe-stage
    and slice-stage refusals, a slice that breaks continuity among the latter; the neighbours' bytes are right, the refused rooms
    untouched"""
    M, D, X = env
    batch = [s for _, s in X.verdicts()]
    recs, out = run(env, enc, batch, 15, "nv12", dst_off=3)
    equals_single(env, enc, batch, recs, out, 15, "nv12")
    run(env, enc, batch, 7)


@pytest.mark.parametrize("kind", ("ext", "mbt"))
def test_altered(env, enc, kind):
    """64 seeded alterations of a stream cut into slices with extras and a quant_matrix_extension / of a stream with all three macroblock
    tools, as one batch: every verdict and err_offset is the definition's.  (The same batches ran through the host build under
    AddressSanitizer in tests/test_decstreams_ex_cases.py.)"""
    M, D, X = env
    batch = X.altered(kind, dict(X.ALTERED)[kind])
    assert len(batch) == 64
    run(env, enc, batch, 15)


def test_chunks(env, enc):
    """the chunk stream - one, two, three slices a row in turn, matrices loaded at its first picture and put back by a repeated sequence
    header, dual-prime P pictures, B pictures - beside others at "decode_batch" 1, 2, 3, 5 and the default: matrices in force chunks
    after their load, a dual-prime picture whose reference is a carried slot, B pictures with both anchors carried - identical
    results, each the single call's"""
    M, D, X = env
    batch = X.chunks()
    results = []
    try:
        for k in X.DECODE_BATCHES:
            enc.set_option("decode_batch", k)
            recs, out = run(env, enc, batch, 15)
            results.append(out.tobytes())
        assert len(set(results)) == 1
        enc.set_option("decode_batch", 2)
        run(env, enc, batch, 15, "nv21", dst_off=7)
        run(env, enc, [s for _, s in X.verdicts()], 15)
        enc.set_option("decode_batch", 1)
        run(env, enc, batch, 13)                                  # (without flag 2 the chunk stream is a probe refusal: the others move up)
    finally:
        enc.set_option("decode_batch", 0)
    equals_single(env, enc, batch, recs, out, 15)


def test_late_refusal_writes_nothing(env, enc):
    """a stream lying in three chunks ("decode_batch" 1) whose last chunk holds a discontinuous slice: nothing of it is written, its
    neighbours are whole"""
    M, D, X = env
    batch, last = X.late()
    try:
        for k in (1, 2):
            enc.set_option("decode_batch", k)
            recs, _ = run(env, enc, batch, 15)
            assert (recs[1]["status"], recs[1]["err_offset"], recs[1]["out_bytes"]) == (D.SYNTAX, last, 0)
    finally:
        enc.set_option("decode_batch", 0)
    run(env, enc, batch, 15)


def test_long_streams(env, enc):
    """plan_cases' long_t and long_x (2 071 events each, nine to a range of the plan: ranges that hold several pictures, loads of both
    matrices and a reset) between short streams, at the default chunk and at "decode_batch" 5"""
    M, D, X = env
    batch = X.long_batch()
    recs, out = run(env, enc, batch, 15)
    try:
        enc.set_option("decode_batch", 5)
        again, out5 = run(env, enc, batch, 15, "nv12")
    finally:
        enc.set_option("decode_batch", 0)
    equals_single(env, enc, batch, recs, out, 15)


def test_cap(env, enc):
    """cap one byte short of the third stream's room: it and the one behind it are OVERFLOW, the two in front are written, nothing at
    or past cap; the probe reports the same layout"""
    M, D, X = env
    batch = X.cap_batch()
    want = X.expected(batch, 15)
    total, offs = want["total"], [w["out_offset"] for w in want["records"]]
    data, seg = X.place(batch, GAP, lead=1)
    probe, _, _ = decode(env, enc, data, seg, 15, probe=True)
    assert [r["out_offset"] for r in probe] == offs
    for cap, st in ((total, [None] * 4), (offs[3] - 1, [None, None, "cap", "cap"]), (offs[1], [None, "cap", "cap", "cap"]), (0, ["cap"] * 4)):
        recs, _ = run(env, enc, batch, 15, cap=cap, dst_off=1)
        assert [r["status"] for r in recs] == [D.OVERFLOW if s else D.OK for s in st] and [r["out_offset"] for r in recs] == offs


def test_alignment(env, enc):
    """sixteen streams at segment offsets 0 .. 15 mod 16 with start codes in the gaps and across both edges of every segment; the
    destination 1 and 7 bytes behind an aligned address with frame_bytes 3 and 1152 in turn, all four layouts"""
    M, D, X = env
    streams, data, seg = X.alignment()
    for dst_off in (1, 7, 0):
        for layout in D.LAYOUTS:
            run(env, enc, streams, 15, layout, placed=(data, seg), dst_off=dst_off)
    run(env, enc, streams, 4, "i420", placed=(data, seg), es_off=5, dst_off=9)


def test_many_streams(env, enc):
    """1 024 streams of 16 x 16 with one, two and three slices in turn in one chunk: every out_offset, every frame"""
    M, D, X = env
    batch, flags = X.batches()["many"]
    recs, _ = run(env, enc, batch, flags, placed=X.place(batch, b"", lead=0))
    assert [r["out_offset"] for r in recs[:4]] == [0, 384, 384 * 3, 384 * 6]


def test_the_entry_rules(env, enc):
    """flags 8, 9, 16 and 0x80000000, nstreams 0 and 65536: M2V_E_PARAM, m2v_last_error names the entry, nothing touched; M2V_E_STATE
    between encode_resident_begin and _end with no byte written and the next legal call right; the handle's five decode options change
    nothing and are not changed; after each, the old entries answer as before"""
    import torch
    M, D, X = env
    import decstreams_cases as S
    X0 = X.X0
    batch = X.chunks()
    data, seg = X.place(batch, GAP, lead=1)
    d = dev(data)
    want = X.expected(batch, 15)
    out = torch.full((want["total"],), X.FILL, dtype=torch.uint8, device="cuda:0")

    def unchanged(e):
        assert (out.cpu().numpy() == X.FILL).all()
        small = S.batches()["smallest"]
        sd, sseg = S.place(small, b"", lead=0)
        frames, recs = e.decode_streams(dev(sd), sseg)
        S.check(S.records_of(recs), frames.cpu().numpy(), S.expected(small), segments=sseg)
        old = X0.chunks()
        od, oseg = X0.place(old, GAP, lead=1)
        frames, recs = e.decode_streams(dev(od), oseg, syntax="main", b_pictures=True, interlaced=True)
        X0.check(X0.records_of(recs), frames.cpu().numpy(), X0.expected(old, 3), segments=oseg)
        for bad in (4, 8):                          # the old entry keeps its two flags
            assert raw(M, e, d.data_ptr(), seg, out.data_ptr(), out.numel(), "i420", bad, "m2v_decode_streams_main_device") == E_PARAM
        f1, r1 = e.decode_device(dev(X0.ipbbpbb()[0]), syntax="main", b_pictures=True)
        assert np.array_equal(f1.cpu().numpy().reshape(-1), D.frames_of(X0.alone(X0.ipbbpbb()[0], 1)["decoded"]).reshape(-1))

    one = (ctypes.c_uint64 * 1)(0)
    for bad in (8, 9, 16, 0x80000000):
        assert raw(M, enc, d.data_ptr(), seg, out.data_ptr(), out.numel(), "i420", bad) == E_PARAM
        assert b"m2v_decode_streams_main_ex_device" in enc._L.m2v_last_error(enc._h)
        unchanged(enc)
    for n in (0, 65536):
        assert enc._L.m2v_decode_streams_main_ex_device(enc._h, d.data_ptr(), one, one, n, None, 0, 0, 15, None) == E_PARAM
        assert b"m2v_decode_streams_main_ex_device" in enc._L.m2v_last_error(enc._h)
    unchanged(enc)
    # the handle's options: the result does not depend on them, and they stay
    base = None
    for values in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 1, 1, 1), (1, 0, 1, 1, 0), (1, 1, 0, 0, 0)):
        try:
            for k, v in zip(OPTIONS, values):
                enc.set_option(k, v)
            recs, got = run(env, enc, batch, 15)
            base = base or got.tobytes()
            assert got.tobytes() == base
            assert [enc._set.get(k, 0) for k in OPTIONS] == list(values)
        finally:
            for k in OPTIONS:
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
        for flags in (15, 3):
            assert raw(M, e, d.data_ptr(), seg, out.data_ptr(), out.numel(), "i420", flags) == E_STATE
        e.encode_resident_end()
        unchanged(e)
        frames, recs = e.decode_streams(d, seg, out=out, syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True)
        X.check(X.records_of(recs), out.cpu().numpy(), want, segments=seg)
        assert torch.equal(M.frames_of_stream(frames, recs[1]).reshape(-1), frames[int(recs[1]["out_offset"]):int(recs[2]["out_offset"])])
    finally:
        e.close()


def test_python_keywords(env, enc):
    """the ValueErrors of the two keywords; with both False the call is today's; the probe-then-allocate path; a container"""
    import demux_writer as DW
    M, D, X = env
    batch = X.chunks()
    data, seg = X.place(batch, GAP, lead=1)
    d = dev(data)
    for kw in (dict(extended=True), dict(syntax="module", extended=True), dict(syntax="main", mb_tools=True), dict(mb_tools=True),
               dict(syntax="main", mode="module", extended=True)):
        with pytest.raises(ValueError):
            enc.decode_streams(d, seg, **kw)
    import torch
    for flags in (5, 7, 15):                        # (into a filled tensor: under 7 the chunk stream keeps a room that must stay untouched)
        want = X.expected(batch, flags)
        out = torch.full((want["total"],), X.FILL, dtype=torch.uint8, device="cuda:0")
        frames, recs = enc.decode_streams(d, seg, out=out, syntax="main", b_pictures=bool(flags & 1), interlaced=bool(flags & 2), extended=True, mb_tools=bool(flags & 8))
        X.check(X.records_of(recs), frames.cpu().numpy(), want, segments=seg)
    frames, recs = enc.decode_streams(d, seg, syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True)      # the probe, then the allocation
    X.check(X.records_of(recs), frames.cpu().numpy(), want, segments=seg)
    for b in range(len(batch)):
        r = want["records"][b]
        assert np.array_equal(M.frames_of_stream(frames, recs[b]).cpu().numpy().reshape(-1), want["out"][r["out_offset"]:r["out_offset"] + r["out_bytes"]])
    # with both False the old entry: the chunk stream is refused there at its first quant_matrix_extension / second slice of a row
    _, recs = enc.decode_streams(d, seg, syntax="main", b_pictures=True, interlaced=True)
    assert [int(q) for q in recs["rec"]["status"]] == [w["status"] for w in X.X0.expected(batch, 3)["records"]]
    assert int(recs["rec"]["status"][1]) == D.SYNTAX
    # a transport stream around every stream
    boxes = []
    for s in batch:
        w = DW.TsWriter(5, video_pid=0x120)
        w.psi(0, DW.pat_section([(1, 0x1000)]))
        w.psi(0x1000, DW.pmt_section(1, 0x120, [(0x02, 0x120, b"")]))
        head = DW.pes_header(0xE0, 0, pts=9000, dts=None)
        payload = head + s
        w.video(payload[:150], pusi=1, head=len(head), stamp=(9000, DW.ABSENT))
        for at in range(150, len(payload), 184):
            w.video(payload[at:at + 184])
        boxes.append(w.bytes())
    cdata, cseg = X.place(boxes, b"", lead=0)
    frames, recs = enc.decode_streams(dev(cdata), cseg, container="ts", syntax="main", b_pictures=True, interlaced=True, extended=True, mb_tools=True)
    want = X.expected(batch, 15)
    for g, w in zip(X.records_of(recs), want["records"]):
        assert (g["status"], g["pictures"], g["out_offset"], g["out_bytes"]) == (w["status"], w["pictures"], w["out_offset"], w["out_bytes"])
    assert np.array_equal(frames.cpu().numpy(), want["out"])
    assert [enc._set.get(k, 0) for k in OPTIONS] == [0] * 5
