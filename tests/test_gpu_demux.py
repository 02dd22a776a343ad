"""-m gpu: the device demultiplexer (m2v_demux_device) against tests/demux_cases.py: the bytes, the stamps and every field of the records
are what the specification (m2vc_demux_ts / m2vc_demux_ps) answers for each container, streams and stamps land where the layout computed
here says, and nothing outside those ranges - filled with a sentinel first - changes.  No tolerance anywhere.
tests/test_demux_cases.py shows what the cases reach.  The two large containers are a few MB; everything else is a few hundred KB."""
import numpy as np
import pytest

import demux_cases as DC

pytestmark = pytest.mark.gpu
M = DC.M
E_PARAM, E_STATE = -1, -4
S64 = int(np.array([DC.SENTINEL] * 8, np.uint8).view(np.int64)[0])


def dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to("cuda:0")


def sentinel(n):
    import torch
    t = torch.full((n,), DC.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def place(blobs, lead=0, gap=7):
    buf, seg = bytearray([DC.SENTINEL] * lead), []
    for s in blobs:
        seg.append((len(buf), len(s)))
        buf += s + bytes([DC.SENTINEL] * gap)
    return bytes(buf), seg


@pytest.fixture(scope="module")
def enc():
    e = M.Mpeg2Encoder(6, 6, 3, 2)
    yield e
    e.close()


def run(enc, kind, blobs, arg=None, lead=0, turn=0, cap=None, stamp_cap=None, room=None):
    """one m2v_demux_device through the C-ABI over the containers placed `lead` bytes past a 16-byte boundary, into a buffer `turn` bytes
    past one and a stamp table, sentinels all around -> (output [from turn on], stamps [all rows, one more than stamp_cap], records, segments)"""
    import ctypes
    import torch
    buf, segs = place(blobs, lead=lead)
    d_src = dev(bytes(16) + buf)[16:]
    assert d_src.data_ptr() % 16 == 0
    need = M.demux_bound([len(b) for b in blobs])
    whole = sentinel((need if room is None else room) + 64 + turn)
    cap = whole.numel() - turn - 32 if cap is None else cap
    nst = sum(len(b) // 9 + 1 for b in blobs) if stamp_cap is None else stamp_cap
    st = torch.full((nst + 1, 4), S64, dtype=torch.int64, device="cuda:0")
    off = (ctypes.c_uint64 * len(segs))(*[a for a, _ in segs])
    nb = (ctypes.c_uint64 * len(segs))(*[b for _, b in segs])
    rc = enc._L.m2v_demux_device(enc._h, DC.KINDS[kind], d_src.data_ptr(), off, nb, len(segs), -1 if arg is None else arg, whole.data_ptr() + turn, cap,
                                 st.data_ptr(), nst, None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    rec = enc.demux_report()
    o = whole.cpu().numpy()
    assert (o[:turn] == DC.SENTINEL).all() and (o[turn + cap:] == DC.SENTINEL).all(), "a byte outside [0, cap) changed"
    return o[turn:], st.cpu().numpy().view(np.uint64), rec, segs


def check(out, stamps, rec, wants, segs, what, cap, stamp_cap):
    """wants: per container the specification's dict.  The layout: each stream on the next 32-byte boundary behind the one before, a
    refused one takes no room and no stamps"""
    assert len(rec) == len(wants), what
    touched = np.zeros(out.size, bool)
    end, at = 0, 0
    for b, w in enumerate(wants):
        r = rec[b]
        o = (end + 31) // 32 * 32
        st = w["status"]
        if st == DC.OK and o + len(w["es"]) > cap:
            st = DC.OVERFLOW
        assert (int(r["src_offset"]), int(r["src_bytes"]), int(r["out_offset"]), int(r["status"])) == (segs[b][0], segs[b][1], o, st), (what, b, r)
        if st == DC.OK:
            assert {f: int(r[f]) for f in DC.RECORD_FIELDS} == w["record"] and int(r["err_offset"]) == 0, (what, b, r, w["record"])
            got = out[o:o + len(w["es"])].tobytes()
            if got != w["es"]:
                d = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(w["es"], np.uint8))[0]
                raise AssertionError("%s container %d: first difference at %d of %d" % (what, b, d[0], len(got)))
            touched[o:o + len(w["es"])] = True
            end = o + len(w["es"])
            n = len(w["stamps"])
            k = max(0, min(n, stamp_cap - at))
            assert [tuple(int(v) for v in row) for row in stamps[at:at + k]] == w["stamps"][:k], (what, b)
            at += n
        else:
            assert {f: int(r[f]) for f in DC.RECORD_FIELDS} == dict.fromkeys(DC.RECORD_FIELDS, 0), (what, b, r)
            assert int(r["err_offset"]) == (w["err_offset"] if st == DC.SYNTAX else 0), (what, b, r, w["err_offset"])
    assert (out[~touched] == DC.SENTINEL).all(), what + ": a byte outside the reported ranges changed"
    assert (stamps[min(at, stamp_cap):] == np.uint64(S64 & 0xFFFFFFFFFFFFFFFF)).all(), what + ": a stamp outside the table's used part changed"


def spec(kind, blobs, arg):
    return [DC.cpu(kind, b, arg) for b in blobs]


def batch(enc, kind, blobs, arg, what, **kw):
    out, stamps, rec, segs = run(enc, kind, blobs, arg, **kw)
    cap = kw.get("cap")
    check(out, stamps, rec, spec(kind, blobs, arg), segs, what, out.size - 32 if cap is None else cap, stamps.shape[0] - 1)
    return rec


# ---- every written case, every refusal, every altered container ----
@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_written_cases_and_refusals(enc, kind):
    every = {**DC.cases(), **DC.refusals()}
    by_arg = {}
    for name in sorted(every):
        c = every[name]
        if c["kind"] == kind:
            by_arg.setdefault(c["arg"], []).append(c)
    assert len(by_arg) >= 2
    for arg, group in by_arg.items():                  # (one call has one `stream` argument)
        rec = batch(enc, kind, [c["data"] for c in group], arg, "%s arg %r" % (kind, arg), lead=3)
        for c, r in zip(group, rec):                   # the writer's log, too
            assert (int(r["status"]), int(r["err_offset"])) == (c["expect"]["status"], c["expect"]["err_offset"])
    assert len(enc.demux_report()) == 0                # popped


@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_altered_containers_in_one_call(enc, kind):
    blobs = DC.altered(kind)
    rec = batch(enc, kind, blobs, DC.alter_arg(kind), kind + " altered", lead=11, turn=5)
    st = np.asarray(rec["status"])
    assert (st == DC.OK).sum() > len(blobs) // 10 and (st != DC.OK).sum() > len(blobs) // 10


@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_every_misalignment_of_source_and_destination(enc, kind):
    c = DC.cases()["ts_shapes" if kind == "ts" else "ps_shapes"]
    for lead, turn in [(k, 0) for k in range(16)] + [(0, k) for k in range(1, 16)] + [(k, (7 * k + 3) % 16) for k in range(1, 16)]:
        batch(enc, kind, [c["data"]], c["arg"], "%s lead %d turn %d" % (kind, lead, turn), lead=lead, turn=turn)


@pytest.mark.parametrize("kind", ["ts", "ps"])
@pytest.mark.parametrize("count", [1, 2, 300])
def test_batches_of_mixed_verdicts_and_a_short_stamp_table(enc, kind, count):
    good = [c for n, c in sorted(DC.cases().items()) if c["kind"] == kind and c["arg"] is None and len(c["data"]) < 60000]
    bad = [c for n, c in sorted(DC.refusals().items()) if c["kind"] == kind and c["arg"] is None]
    pick = [(bad if k % 3 == 1 else good)[(k // 3 + k) % len(bad if k % 3 == 1 else good)] for k in range(count)]
    blobs = [c["data"] for c in pick]
    total = sum(len(c["expect"]["stamps"]) for c in pick)
    rec = batch(enc, kind, blobs, None, "%s batch of %d" % (kind, count), lead=1, turn=9, stamp_cap=max(1, total * 2 // 3 - 1))
    if count > 1:
        assert int(rec["status"][1]) != DC.OK and int(rec["out_bytes"][1]) == 0
        if count > 2:
            assert int(rec["out_offset"][2]) == (int(rec["out_offset"][0]) + int(rec["out_bytes"][0]) + 31) // 32 * 32
    assert int(rec["pes_packets"].sum()) == total and total >= 2      # (more stamps than the table holds)


@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_cap_one_byte_short(enc, kind):
    c = DC.cases()["ts_shapes" if kind == "ts" else "ps_many_units"]
    n = len(c["expect"]["es"])
    out, stamps, rec, _ = run(enc, kind, [c["data"]], c["arg"], cap=n - 1)
    assert (int(rec["status"][0]), int(rec["out_bytes"][0]), int(rec["pes_packets"][0])) == (DC.OVERFLOW, 0, 0)
    assert (out == DC.SENTINEL).all() and (stamps == np.uint64(S64 & 0xFFFFFFFFFFFFFFFF)).all()
    batch(enc, kind, [c["data"]], c["arg"], "exactly cap", cap=n)
    # a batch: the stream that does not fit overflows and takes no room, a later one that fits what is left is written in its place
    small = DC.alter_base("ts")[0] if kind == "ts" else DC.cases()["ps_shapes"]
    assert 0 < len(small["expect"]["es"]) < n - 1
    rec = batch(enc, kind, [c["data"], c["data"], small["data"]], None, "overflow in a batch", cap=(n + 31) // 32 * 32 + n - 1)
    assert [int(v) for v in rec["status"]] == [DC.OK, DC.OVERFLOW, DC.OK]


def launch_shape(kind, blobs, cap, blocks=4096):
    """the grids of one call as include/m2v_mi355x.h states them (option "demux_blocks"): at most `blocks` workgroups of 256 lanes a
    launch, shared out among the containers -> (workgroups per container of the kernels over tiles / table entries, lanes of the write-out)"""
    per = max(1, blocks // len(blobs))
    if kind == "ts":
        want = max(1, max((len(b) // 188 + DC.scan_tile() // 188 - 1) // (DC.scan_tile() // 188) for b in blobs))
    else:
        want = max(1, (max(len(b) for b in blobs) // 9 + 256) // 256)
    return min(want, per), 256 * min(max(1, (cap // 16 + 255) // 256), blocks)


@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_a_container_of_a_few_mb(enc, kind):
    """The kernels over tiles, table entries and output units stride their grids.  That a launch does not cover its work at once - so
    that the loops take a second trip and more, re-initialising and reusing their LDS - is shown here from the sizes, not assumed:
    with the default grid in a batch large enough that a container's share of the workgroups is smaller than its tiles, and with option
    "demux_blocks" = 2 and 3, where every kernel goes round many times.  (The program stream's chain is one lane: it has no tile pass and
    no reachability path, in LDS or in memory.)"""
    c = DC.big(kind)
    tile = DC.scan_tile() // 188
    assert len(c["data"]) > 2 << 20 and c["expect"]["status"] == DC.OK and c["arg"] is None
    tiles = (len(c["data"]) // 188 + tile - 1) // tile
    units = len(c["expect"]["es"]) // 16
    entries = len(c["expect"]["stamps"])               # (PS: one table entry per PES packet)
    out, stamps, rec, segs = run(enc, kind, [c["data"]], None, lead=7, turn=13)
    check(out, stamps, rec, [c["expect"]], segs, kind + " big", out.size - 32, stamps.shape[0] - 1)
    # the default grid: 700 small containers behind the big one leave it 5 workgroups for its 13 tiles
    small = DC.cases()[kind + "_shapes"]
    blobs = [c["data"]] + [small["data"]] * (700 if kind == "ts" else 300)
    per, _ = launch_shape(kind, blobs, M.demux_bound([len(b) for b in blobs]) + 32)
    if kind == "ts":
        assert tiles >= 13 and per <= 5 and tiles > 2 * per
    batch(enc, kind, blobs, None, kind + " big in a large batch")
    # two workgroups for everything, then three among three containers (one each)
    try:
        for blocks, blobs in ((2, [c["data"]]), (3, [small["data"], c["data"], small["data"]])):
            enc.set_option("demux_blocks", blocks)
            cap = M.demux_bound([len(b) for b in blobs]) + 32
            per, lanes = launch_shape(kind, blobs, cap, blocks)
            assert per == (2 if blocks == 2 else 1) and lanes == 256 * blocks
            assert units > 100 * lanes                 # the write-out: hundreds of trips
            if kind == "ts":
                assert tiles > 6 * per                 # k_ts_tiles, k_demux_table: a second tile pass and more
            else:
                assert entries > 2 * 256 * per         # k_demux_table's stamps
            batch(enc, kind, blobs, None, "%s big with %d workgroups" % (kind, blocks), lead=5, turn=3)
        with pytest.raises(M.M2VError):
            enc.set_option("demux_blocks", 4097)
    finally:
        enc.set_option("demux_blocks", 0)


# ---- on the handle: what the muxer wrote comes back, and the decoder takes it ----
def test_round_trip_and_decode_from_a_container():
    import torch
    x = torch.from_numpy(M.synth.clip(96, 64, 5, clip_index=77)).to("cuda:0")
    e = M.Mpeg2Encoder(6, 6, 3, 2)
    try:
        frames = x.permute(0, 2, 3, 1).contiguous() if x.shape[1] == 3 else x
        es = e.encode_tensor(frames, 4)
        info, _ = DC.C.scan(es.cpu().numpy().tobytes())
        assert info.pictures == 5 and info.p_pictures == 4
        stream = es[:info.bytes]                       # without the final word's padding
        for mode in ("iso", "module"):
            want, _ = e.decode_device(es, mode=mode)
            for kind in ("ts", "ps"):
                box = e.encode_tensor(frames, 4, container=kind)
                out, rec = e.demux_device(box, kind)
                assert int(rec["status"][0]) == DC.OK and int(rec["out_offset"][0]) == 0
                assert torch.equal(out[:int(rec["out_bytes"][0])], stream), kind
                got, r = e.decode_device(box, mode=mode, container=kind)
                assert torch.equal(got, want) and int(r["pictures"]) == 5, (kind, mode)
        # a batch's containers through `segments`
        s, offsets = e.encode_batch(frames, 1, lengths=[2, 3])
        s = s.cpu().numpy().tobytes()
        clips = [s[offsets[b]:offsets[b + 1]] for b in range(2)]
        for kind in ("ts", "ps"):
            box, where = e.encode_batch(frames, 1, lengths=[2, 3], container=kind)
            out, rec, stamps = e.demux_device(box, kind, segments=where, stamps=True)
            o = out.cpu().numpy().tobytes()
            for b in range(2):
                n = DC.C.scan(clips[b])[0].bytes
                assert int(rec["status"][b]) == DC.OK and o[int(rec["out_offset"][b]):int(rec["out_offset"][b] + rec["out_bytes"][b])] == clips[b][:n], (kind, b)
            assert stamps.shape[0] == int(rec["pes_packets"].sum()) >= 5
        with pytest.raises(M.M2VError, match="M2V_DEMUX_SYNTAX"):
            e.decode_device(es, container="ts")        # an elementary stream is no transport stream
    finally:
        e.close()


def test_state_and_parameter_rules():
    import ctypes
    import torch
    c = DC.cases()["ts_shapes"]
    e = M.Mpeg2Encoder(6, 6, 3, 2)
    try:
        src, out = dev(c["data"]), sentinel(len(c["data"]) + 64)
        one = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(len(c["data"]))
        call = lambda kind, stream, n=1, off=one[0], nb=one[1]: e._L.m2v_demux_device(e._h, kind, src.data_ptr(), off, nb, n, stream, out.data_ptr(), out.numel(),
                                                                                      None, 0, None)
        assert call(3, -1) == E_PARAM and call(0, -1) == E_PARAM
        assert call(1, 0x2000) == E_PARAM and call(1, -2) == E_PARAM and call(2, 0xDF) == E_PARAM and call(2, 0xF0) == E_PARAM and call(2, 0) == E_PARAM
        many = (ctypes.c_uint64 * 65536)()
        assert call(1, -1, n=65536, off=many, nb=many) == E_PARAM and call(1, -1, n=0) == E_PARAM
        assert (out.cpu().numpy() == DC.SENTINEL).all()
        # while a sequence is in progress
        frames = M.synth.clip(96, 64, 2, clip_index=3)
        d_in = torch.from_numpy(np.ascontiguousarray(frames).reshape(2, -1)).to("cuda:0")
        d_es = sentinel(1 << 18)
        e.encode_resident_begin(d_in.data_ptr(), 2, d_es.data_ptr(), d_es.numel(), 6, 4, 1)
        assert call(1, -1) == E_STATE and b"m2v_demux_device" in e._L.m2v_last_error(e._h)
        with pytest.raises(M.M2VError):
            e.demux_device(src, "ts")
        e.encode_resident_end()
        assert (out.cpu().numpy() == DC.SENTINEL).all()
        # the next legal call gives the right result
        got, rec = e.demux_device(src, "ts", out=out)
        n = int(rec["out_bytes"][0])
        assert int(rec["status"][0]) == DC.OK and got.cpu().numpy()[:n].tobytes() == c["expect"]["es"]
        for bad in (dict(kind="avi"), dict(kind="ts", segments=[(0, len(c["data"]) + 1)]), dict(kind="ts", segments=[]), dict(kind="ts", cap=out.numel() + 1, out=out)):
            with pytest.raises(ValueError):
                e.demux_device(src, **bad)
    finally:
        e.close()


def test_tb_demux_and_decode_from_a_container(tmp_path):
    """m2v_tb -demux and m2v_tb -decode -container: file to file through m2v_demux_device"""
    import os
    import subprocess
    import torch
    M.build()
    tb = os.path.join(DC.ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    x = torch.from_numpy(M.synth.clip(96, 64, 3, clip_index=78)).to("cuda:0").permute(0, 2, 3, 1).contiguous()
    e = M.Mpeg2Encoder(6, 6, 3, 2)
    try:
        es = e.encode_tensor(x, 2).cpu().numpy().tobytes()
        want = e.decode_device(e.encode_tensor(x, 2), layout="nv12", mode="module")[0].cpu().numpy().tobytes()
    finally:
        e.close()
    n = DC.C.scan(es)[0].bytes
    (tmp_path / "v.ts").write_bytes(DC.C.mux_ts(es))
    (tmp_path / "v.mpg").write_bytes(DC.C.mux_ps(es))
    r = subprocess.run([tb, "-demux", "ts", str(tmp_path / "v.ts"), str(tmp_path / "v.m2v"), "-pid", "0x100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "3 PES packets" in r.stdout, r.stdout + r.stderr
    assert (tmp_path / "v.m2v").read_bytes() == es[:n]
    r = subprocess.run([tb, "-decode", str(tmp_path / "v.mpg"), str(tmp_path / "v.yuv"), "-container", "ps", "-mode", "module", "-reconfmt", "nv12"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "v.yuv").read_bytes() == want
    r = subprocess.run([tb, "-demux", "ps", str(tmp_path / "v.ts"), str(tmp_path / "x.m2v")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "status -2" in r.stderr and not (tmp_path / "x.m2v").exists(), r.stdout + r.stderr
