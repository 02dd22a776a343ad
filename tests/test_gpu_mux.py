"""-m gpu: the device muxer (m2v_set_mux_out, m2v_mux_device) against tests/mux_cases.py: every container is byte for byte what the CPU
muxers (m2vc_mux_ts / m2vc_mux_ps) return for the same elementary stream, the records are the offsets and sizes computed here, and
nothing outside the reported ranges of the output - filled with a sentinel first - changes.  No tolerance anywhere.
tests/test_mux_cases.py shows what the cases reach.  Nothing is larger than a few hundred KB."""
import numpy as np
import pytest

import mux_cases as Q

pytestmark = pytest.mark.gpu
M = Q.M
E_STATE = -4


def dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to("cuda:0")


def sentinel(n):
    import torch
    t = torch.full((n,), Q.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def same_bytes(got, want, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        m = min(a.size, b.size)
        d = np.nonzero(a[:m] != b[:m])[0]
        raise AssertionError("%s: %d bytes, expected %d, first difference at %s" % (what, a.size, b.size, d[0] if d.size else m))


def check_output(out, rec, wants, segs, what="", cap=None):
    """out: the whole output buffer (numpy); wants: per stream the container's bytes or the negative status"""
    lay = Q.layout([len(w) if isinstance(w, bytes) else w for w in wants], out.size if cap is None else cap)
    assert len(rec) == len(wants), (what, len(rec))
    touched = np.zeros(out.size, bool)
    for b, (w, (o, nb, st)) in enumerate(zip(wants, lay)):
        r = rec[b]
        assert (int(r["out_offset"]), int(r["out_bytes"]), int(r["status"])) == (o, nb, st), (what, b, r, (o, nb, st))
        if segs is not None and st != Q.OVERFLOW:
            assert (int(r["es_offset"]), int(r["es_bytes"])) == segs[b], (what, b)
        if st == 0:
            same_bytes(out[o:o + nb].tobytes(), w, "%s stream %d" % (what, b))
            touched[o:o + nb] = True
    assert (out[~touched] == Q.SENTINEL).all(), what + ": a byte outside the reported ranges changed"


@pytest.fixture(scope="module")
def enc():
    e = M.Mpeg2Encoder(6, 6, 3, 2)
    yield e
    e.close()


# ---- m2v_mux_device ----
@pytest.mark.parametrize("kind", Q.KINDS)
def test_mux_device_every_case_in_one_call(enc, kind):
    names = sorted(Q.cases())
    streams = [Q.cases()[n] for n in names] + [Q.oracle_clip(k)[1] for k in Q.ORACLE_CLIPS]
    wants = [Q.cpu_mux(kind, s) for s in streams]
    buf, segs = Q.place(streams, lead=3)
    out = sentinel(sum(len(w) for w in wants) + 64 * len(wants) + 77)
    _, rec = enc.mux_device(dev(buf), kind, segments=segs, out=out)
    check_output(out.cpu().numpy(), rec, wants, segs, kind)
    assert [int(v) for v in rec["pictures"]] == [len(Q.C.scan(s)[1]) for s in streams]
    assert len(enc.mux_report()) == 0                  # popped


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", ["long", "boundary0", "boundary1", "boundary2", "boundary3", "small"])
def test_mux_device_alone(enc, kind, name):
    es = Q.cases()[name]
    want = Q.cpu_mux(kind, es)
    out = sentinel(len(want) + 100)
    _, rec = enc.mux_device(dev(es), kind, out=out)
    check_output(out.cpu().numpy(), rec, [want], [(0, len(es))], name)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_mux_device_allocates_from_the_bound(enc, kind):
    es = Q.cases()["ts_stuffing"]
    out, rec = enc.mux_device(dev(es), kind)
    assert int(rec["status"][0]) == 0
    same_bytes(out[:int(rec["out_bytes"][0])].cpu().numpy().tobytes(), Q.cpu_mux(kind, es), kind)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_error_cases_yield_their_status_and_write_nothing(enc, kind):
    errs = Q.error_cases()
    names = sorted(errs)
    good = Q.cases()["rate3"]
    streams = [errs[n][0] for n in names[:3]] + [good] + [errs[n][0] for n in names[3:]]
    wants = [errs[n][1] for n in names[:3]] + [Q.cpu_mux(kind, good)] + [errs[n][1] for n in names[3:]]
    buf, segs = Q.place(streams)
    out = sentinel(len(wants[3]) + 4096)
    _, rec = enc.mux_device(dev(buf), kind, segments=segs, out=out)
    check_output(out.cpu().numpy(), rec, wants, segs, kind)
    for n in names:                                    # ... and each one alone
        out = sentinel(4096)
        _, rec = enc.mux_device(dev(errs[n][0]), kind, out=out)
        check_output(out.cpu().numpy(), rec, [errs[n][1]], None, n)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_cap_one_byte_short(enc, kind):
    es = Q.cases()["rate5"]
    want = Q.cpu_mux(kind, es)
    out = sentinel(len(want) + 64)
    _, rec = enc.mux_device(dev(es), kind, out=out, cap=len(want) - 1)
    assert (int(rec["status"][0]), int(rec["out_bytes"][0])) == (Q.OVERFLOW, 0)
    assert (out.cpu().numpy() == Q.SENTINEL).all()
    _, rec = enc.mux_device(dev(es), kind, out=out, cap=len(want))
    assert int(rec["status"][0]) == 0
    o = out.cpu().numpy()
    same_bytes(o[:len(want)].tobytes(), want, kind)
    assert (o[len(want):] == Q.SENTINEL).all()
    # a batch: the container that does not fit overflows and takes no room, the others are written
    streams = [Q.cases()[n] for n in Q.BATCH]
    wants = [Q.cpu_mux(kind, s) for s in streams]
    lay = Q.layout([len(w) for w in wants], 1 << 30)
    cap = lay[3][0] + lay[3][1] - 1                    # one byte short of the fourth
    buf, segs = Q.place(streams)
    out = sentinel(lay[-1][0] + lay[-1][1] + 64)
    _, rec = enc.mux_device(dev(buf), kind, segments=segs, out=out, cap=cap)
    assert [int(v) for v in rec["status"]][:4] == [0, 0, 0, Q.OVERFLOW]
    o = out.cpu().numpy()
    check_output(o, rec, wants, segs, kind, cap=cap)   # (a later container that fits what is left is written where the refused one would be)
    assert (o[cap:] == Q.SENTINEL).all(), "nothing past cap is ever written"


@pytest.mark.parametrize("kind", Q.KINDS)
def test_every_misalignment_of_stream_and_output(enc, kind):
    es = Q.cases()["rate4"]
    want = Q.cpu_mux(kind, es)
    for lead in range(16):
        turn = (7 * lead + 3) % 16                     # the output's misalignment: every value once, too
        buf, segs = Q.place([es], lead=lead)
        whole = sentinel(len(want) + 64)
        d_es = dev(bytes(16) + buf)[16:]               # (a view: the stream starts `lead` bytes past a 16-byte boundary)
        assert (d_es.data_ptr() + segs[0][0]) % 16 == lead and (whole.data_ptr() + turn) % 16 == turn
        _, rec = enc.mux_device(d_es, kind, segments=segs, out=whole[turn:])
        o = whole.cpu().numpy()
        check_output(o[turn:], rec, [want], segs, "%s lead %d turn %d" % (kind, lead, turn))
        assert (o[:turn] == Q.SENTINEL).all()


@pytest.mark.parametrize("kind", Q.KINDS)
def test_batch_of_five_streams(enc, kind):
    streams = [Q.cases()[n] for n in Q.BATCH]
    wants = [Q.cpu_mux(kind, s) for s in streams]
    buf, segs = Q.place(streams, lead=5, gap=11)
    whole = sentinel(sum(len(w) for w in wants) + 32 * 6 + 9)
    _, rec = enc.mux_device(dev(buf), kind, segments=segs, out=whole[9:])
    check_output(whole.cpu().numpy()[9:], rec, wants, segs, kind)


# ---- m2v_set_mux_out ----
def resident(e, frames, w, h, pf, kind, begin=False, mux_room=None):
    """a resident call over planar 4:4:4 frames with a container buffer of `kind` set (None: no buffer) -> what the check needs"""
    import torch
    n = frames.shape[0]
    xs, ys = w // 16, h // 16
    d_in = torch.from_numpy(np.ascontiguousarray(frames).reshape(n, -1)).to("cuda:0")
    room = n * (3 * 256 * xs * ys + 128) + (1 << 16)
    d_out = sentinel(room)
    d_mux = sentinel(M.mux_bound(kind, room, n) + 64 * n if mux_room is None else mux_room) if kind else None
    e.set_mux_out(kind, d_mux.data_ptr() if kind else None, d_mux.numel() if kind else 0)
    a = (d_in.data_ptr(), n, d_out.data_ptr(), room, xs, ys, pf)
    if begin:
        e.encode_resident_begin(*a)
        return d_in, d_out, d_mux
    nb = e.encode_resident(*a)
    return finish(e, nb, d_out, d_mux)


def finish(e, nb, d_out, d_mux):
    o = d_out.cpu().numpy()
    assert (o[nb:] == Q.SENTINEL).all()
    return o[:nb].tobytes(), (d_mux.cpu().numpy() if d_mux is not None else None), e.mux_report()


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("key", Q.ORACLE_CLIPS)
def test_resident_container_is_the_cpu_mux_of_the_oracle_stream(key, kind):
    frames, want_es, w, h, pf, ql = Q.oracle_clip(key)
    e = M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        es, mux, rec = resident(e, frames, w, h, pf, kind)
        same_bytes(es, want_es, "the elementary stream with the buffer set")
        check_output(mux, rec, [Q.cpu_mux(kind, want_es)], [(0, len(want_es))], key)
        assert int(rec["pictures"][0]) == frames.shape[0]
        es2, _, rec2 = resident(e, frames, w, h, pf, None)          # cleared: the same stream, no record
        assert es2 == want_es and len(rec2) == 0
    finally:
        e.close()


def test_begin_end_on_two_handles_taking_turns():
    fa, wa, w, h, pf, ql = Q.oracle_clip("ip")
    fb, wb, w2, h2, pf2, _ = Q.oracle_clip("i")
    a, b = M.Mpeg2Encoder(6, 6, 3, ql), M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        for turn in range(2):
            ka, kb = ("ts", "ps") if turn == 0 else ("ps", "ts")
            ha = resident(a, fa, w, h, pf, ka, begin=True)
            hb = resident(b, fb, w2, h2, pf2, kb, begin=True)
            es, mux, rec = finish(a, a.encode_resident_end(), ha[1], ha[2])
            assert es == wa
            check_output(mux, rec, [Q.cpu_mux(ka, wa)], [(0, len(wa))], "a turn %d" % turn)
            es, mux, rec = finish(b, b.encode_resident_end(), hb[1], hb[2])
            assert es == wb
            check_output(mux, rec, [Q.cpu_mux(kb, wb)], [(0, len(wb))], "b turn %d" % turn)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("chunk,split", [(4, 1), (5, 3)])
def test_batch_frames_cuts_the_clip_into_chunks(kind, chunk, split):
    frames, want_es, w, h, pf, ql = Q.oracle_clip("ip")
    e = M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        e.set_option("batch_frames", chunk)
        e.set_option("split_streams", split)
        es, mux, rec = resident(e, frames, w, h, pf, kind)
        assert es == want_es
        check_output(mux, rec, [Q.cpu_mux(kind, want_es)], [(0, len(want_es))], kind)
    finally:
        e.close()


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("chunk", [96, 4])
def test_one_container_per_clip_of_a_batch(kind, chunk):
    from oracle import m2v_oracle_ctypes as orc
    frames, _, w, h, pf, ql = Q.oracle_clip("ip")
    lengths = [3, 1, 5, 2]
    e = M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        e.set_option("batch_frames", chunk)
        e.set_sequences(lengths)
        es, mux, rec = resident(e, frames, w, h, pf, kind)
        clips, at = [], 0
        for n in lengths:
            clips.append(orc.encode(frames[at:at + n], w // 16, h // 16, pf, XL=6, YL=6, VL=3, Q=ql))
            at += n
        assert es == b"".join(clips)
        off = np.cumsum([0] + [len(c) for c in clips])
        check_output(mux, rec, [Q.cpu_mux(kind, c) for c in clips], [(int(off[b]), len(c)) for b, c in enumerate(clips)], kind)
        assert [int(v) for v in rec["pictures"]] == lengths
        assert len(e.sequence_report()) == len(lengths)
    finally:
        e.close()


@pytest.mark.parametrize("kind", Q.KINDS)
def test_stream_description_repeated_headers_and_a_gop_list(kind):
    """the expected elementary stream is the one the same settings give with no buffer set (tests/test_gpu_stream_desc.py and
    tests/test_gpu_gop_starts.py hold that one against the oracle); the container is the CPU mux of it"""
    frames, _, w, h, pf, ql = Q.oracle_clip("ip")
    e = M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        e.set_stream_desc(M.stream_desc(fps=(30000, 1001), repeat_headers=True))
        e.set_gop_starts([2, 7])
        want_es, _, _ = resident(e, frames, w, h, pf, None)
        info, pics = Q.C.scan(want_es)
        assert info.frame_rate_code == 4 and want_es.count(b"\x00\x00\x01\xb3") == info.gops == 4        # GOPs start at 0, 2, 6 (cadence), 7
        es, mux, rec = resident(e, frames, w, h, pf, kind)
        assert es == want_es
        check_output(mux, rec, [Q.cpu_mux(kind, want_es)], [(0, len(want_es))], kind)
    finally:
        e.close()


def test_elementary_stream_overflow_gives_every_record_the_overflow_status():
    import torch
    frames, want_es, w, h, pf, ql = Q.oracle_clip("ip")
    e = M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        e.set_sequences([5, 6])
        n = frames.shape[0]
        d_in = torch.from_numpy(np.ascontiguousarray(frames).reshape(n, -1)).to("cuda:0")
        d_out, d_mux = sentinel(1 << 20), sentinel(1 << 20)
        e.set_mux_out("ts", d_mux.data_ptr(), d_mux.numel())
        with pytest.raises(M.M2VError):
            e.encode_resident(d_in.data_ptr(), n, d_out.data_ptr(), 256, w // 16, h // 16, pf)
        rec = e.mux_report()
        assert [int(v) for v in rec["status"]] == [Q.OVERFLOW, Q.OVERFLOW] and not rec["out_bytes"].any()
        assert (d_mux.cpu().numpy() == Q.SENTINEL).all()
    finally:
        e.close()


def test_encode_tensor_and_encode_batch_return_the_container():
    import torch
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.randint(0, 256, size=(6, 64, 96, 3)).astype(np.uint8)).to("cuda:0")
    e = M.Mpeg2Encoder(6, 6, 3, 2)
    try:
        es = e.encode_tensor(x, 2).cpu().numpy().tobytes()
        for kind in Q.KINDS:
            got = e.encode_tensor(x, 2, container=kind)
            same_bytes(got.cpu().numpy().tobytes(), Q.cpu_mux(kind, es), "encode_tensor " + kind)
        assert e.encode_tensor(x, 2).cpu().numpy().tobytes() == es          # the handle's setting is back: no buffer
        stream, offsets = e.encode_batch(x, 2, lengths=[2, 4])
        s = stream.cpu().numpy().tobytes()
        clips = [s[offsets[b]:offsets[b + 1]] for b in range(2)]
        got, where = e.encode_batch(x, 2, lengths=[2, 4], container="ts")
        g = got.cpu().numpy().tobytes()
        assert len(where) == 2 and all(o % 32 == 0 for o, _ in where)
        for b, (o, nb) in enumerate(where):
            same_bytes(g[o:o + nb], Q.cpu_mux("ts", clips[b]), "encode_batch clip %d" % b)
    finally:
        e.close()


def test_push_and_mux_device_refusals():
    import torch
    frames, _, w, h, pf, ql = Q.oracle_clip("i")
    e = M.Mpeg2Encoder(6, 6, 3, ql)
    try:
        d_mux = sentinel(1 << 16)
        e.set_mux_out("ps", d_mux.data_ptr(), d_mux.numel())
        assert e._L.m2v_push_frames(e._h, w // 16, h // 16, pf, np.ascontiguousarray(frames).ctypes.data, frames.shape[0]) == E_STATE
        assert b"m2v_set_mux_out" in e._L.m2v_last_error(e._h)
        e.set_mux_out(None)
        assert e.encode(frames, w // 16, h // 16, pf) == Q.oracle_clip("i")[1]      # cleared: the port works
        # m2v_mux_device refuses while a resident call is in flight
        hold = resident(e, frames, w, h, pf, None, begin=True)
        with pytest.raises(M.M2VError):
            e.mux_device(dev(Q.cases()["one"]), "ts")
        e.encode_resident_end()
        with pytest.raises(M.M2VError):
            e.set_mux_out("ts", 0, 16)
        assert (d_mux.cpu().numpy() == Q.SENTINEL).all() and hold is not None
    finally:
        e.close()


def test_tb_devmux_writes_the_device_muxed_files(tmp_path):
    """m2v_tb -ps -ts -devmux: the files beside the .m2v come from m2v_mux_device, and are the CPU muxers' bytes"""
    import os
    import subprocess
    M.build()
    tb = os.path.join(Q.ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    clip = M.synth.clip(160, 96, 7, clip_index=95)
    fin = tmp_path / "v.yuv"
    fin.write_bytes(clip.tobytes())
    out = tmp_path / "v.m2v"
    r = subprocess.run([tb, "-p", "3", "-ps", "-ts", "-devmux", str(fin), "160", "96", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    es = out.read_bytes()
    assert (tmp_path / "v.m2v.mpg").read_bytes() == Q.cpu_mux("ps", es)
    assert (tmp_path / "v.m2v.ts").read_bytes() == Q.cpu_mux("ts", es)
