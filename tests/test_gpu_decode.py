"""-m gpu: m2v_decode_device against the oracle's `recon` dumps (through recon_cases.write_layout) and, where stated, decoder.decode -
byte for byte, no tolerance anywhere.  Every decode writes into a buffer filled with 0xA5 with GUARD bytes in front of and behind the
frames that must stay 0xA5, and the capacity handed in is exactly the frames' bytes.  tests/test_dec_cases.py runs the same streams
through the host build of the same arithmetic and shows that the cases are not vacuous.  Small shapes; what each case is for is in its
docstring."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import dec_cases
    return dec_cases.M, dec_cases


@pytest.fixture(scope="module")
def enc(env):
    M, D = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(M, D, enc, stream, layout="i420", mode="module", es_off=0, dst_off=0, cap=None, probe=False):
    """one m2v_decode_device through the C-ABI: the stream es_off bytes behind an aligned address, the frames dst_off bytes behind one,
    GUARD bytes of FILL around them.  -> (frames [n, frame bytes] or None, record); asserts the guards, and with a status other than
    OK that nothing at all was written"""
    import torch
    room = 1 << 16
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    r0 = None
    if cap is None or probe:
        assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES[mode], None) == 0
        r0 = enc.decode_report()
        room = int(r0["pictures"]) * int(r0["frame_bytes"])
        if probe:
            return None, r0
    cap = room if cap is None else cap
    buf = torch.full((2 * D.GUARD + dst_off + max(cap, room) + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, cap, M.LAYOUTS_420[layout],
                                  D.MODES[mode], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r = enc.decode_report()
    got = buf.cpu().numpy()
    a, b = D.GUARD + dst_off, D.GUARD + dst_off + int(r["out_bytes"])
    assert (got[:a] == D.FILL).all() and (got[b:] == D.FILL).all(), "bytes outside the frames were written"
    if r["status"] != D.OK:
        assert r["out_bytes"] == 0
        return None, r
    return got[a:b].reshape(int(r["pictures"]), -1), r


def same(got, want, what=""):
    assert got is not None, (what, "refused")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    assert bad.size == 0, (what, "%d bytes differ, first at" % bad.size, bad[:8].tolist(), "frame bytes", want.shape[1])


def names_of_recon():
    import dec_cases
    return dec_cases.recon_names()


@pytest.mark.parametrize("name", names_of_recon())
def test_recon_cases(env, enc, name):
    """recon_cases.gpu_cases() - 64 x 64, 96 x 64, 80 x 112 (40-byte chroma rows), 272 x 64, the fit cases as coded and with the true
    size in the header (the crop to 100 x 70 and 49 x 49), levels per GOP, the cap's redo, GOP starts at 2 and 7 - against the oracle's
    dump, in all four layouts; plain streams in M2V_DEC_MODULE, the conformant one in M2V_DEC_ISO.  The record's counts are the stream's"""
    M, D = env
    c = D.recon_streams()[name]
    mode = "iso" if c["conformant"] else "module"
    for layout in D.LAYOUTS:
        want = D.expected_from_dump(c, layout)
        got, r = decode(M, D, enc, c["stream"], layout, mode)
        same(got, want, (name, layout))
        w, h = c["region"] or (c["W"], c["H"])
        assert (r["width"], r["height"], r["pictures"], r["frame_bytes"]) == (w, h, want.shape[0], want.shape[1])
    d = M.decoder.sequence_headers(c["stream"])
    assert (d[0], d[1]) == (r["width"], r["height"]) and r["es_bytes"] == len(c["stream"]) and r["chains"] == r["gops"] >= 1


def clip_cases():
    import dec_cases
    return dec_cases.clip_cases()


def clip_ids():
    import dec_cases
    return [dec_cases.clip_id(fc) for fc in dec_cases.clip_cases()]


_dumps = {}


def clip_dump(D, fc, conformant):
    """the oracle's stream and recon dump of a clip case"""
    import entropy_clips as E, search_clips as SR, transform_clips as T
    from oracle import m2v_oracle_ctypes as orc
    key = (fc, conformant)
    if key not in _dumps:
        family, case = fc
        if family == "e":
            clip, pf, VL, Q = E.cached_clip(*case)
        elif family == "s":
            (clip, pf), VL, Q = SR.cached_clip(*case), case[1], case[2]
        else:
            clip, pf, VL, Q = T.cached_clip(*case)
        clip = np.asarray(clip)
        s, dump = orc.encode(clip, clip.shape[3] // 16, clip.shape[2] // 16, pf, 7, 7, VL, Q, dump=True, conformant=conformant)
        _dumps.clear()                                          # (one at a time: the dumps are large)
        _dumps[key] = (s, dump["recon"], clip.shape[3], clip.shape[2])
    return _dumps[key]


@pytest.mark.parametrize("fc", clip_cases(), ids=clip_ids())
def test_clips(env, enc, fc):
    """the entropy, search (VECTOR_LEVEL 3) and transform clips: every table code and escape, DC size, pattern and vector delta, every
    legal vector at every edge and corner with every half-pel phase, the dequantiser's boundaries, saturation, mismatch control and both
    clip ranges - plain -> MODULE, conformant -> ISO, I420, against the oracle's dump"""
    M, D = env
    import recon_cases as R
    for conformant in (False, True):
        s, recon, W, H = clip_dump(D, fc, conformant)
        got, r = decode(M, D, enc, s, "i420", "iso" if conformant else "module")
        same(got, R.write_layout(recon, W, H, "i420"), (fc, conformant))


def test_crossed_modes(env, enc):
    """ISO on a plain stream and MODULE on a conformant one: no dump says what that gives, decoder.decode does"""
    M, D = env
    import search_clips as SR
    rs = D.recon_streams()
    p_heavy = [c for c in SR.cases() if c[0] == "interior" and c[1] == 3][0]
    streams = [rs["unref"]["stream"], rs["g80"]["stream"], D.clip_stream("s", p_heavy, False), rs["conformant"]["stream"], D.clip_stream("s", p_heavy, True)]
    for k, s in enumerate(streams):
        mode, quirks = ("iso", False) if k < 3 else ("module", True)
        got, _ = decode(M, D, enc, s, "i420", mode)
        same(got, D.frames_of(M.decoder.decode(s, quirks=quirks)), (k, mode))


@pytest.mark.parametrize("name", ("starts", "levels"))
def test_decode_batch(env, name):
    """chunks of 1, 2, 3 pictures and the default: the same bytes.  "starts" is 12 frames in chains of 2, 4, 1, 4 and 1: the reference is
    carried across every kind of chunk edge"""
    M, D = env
    c = D.recon_streams()[name]
    want = D.expected_from_dump(c, "nv12")
    e = M.Mpeg2Encoder()
    try:
        for batch in (1, 2, 3, 0):
            e.set_option("decode_batch", batch)
            got, r = decode(M, D, e, c["stream"], "nv12", "module")
            same(got, want, (name, batch))
            if name == "starts":
                assert r["pictures"] == 12 and r["chains"] == 5
    finally:
        e.close()


def test_any_byte_address(env, enc):
    """the stream at byte offsets 0 .. 15 and the frames at 0, 1, 7 and 15; cap == out_bytes is OK, one byte less is M2V_DEC_OVERFLOW
    with the whole buffer untouched"""
    M, D = env
    c = D.recon_streams()["fit49x49_444_true"]                   # rows of 49 and 25 bytes
    for layout, offs in (("i420", range(16)), ("nv21", (3, 9))):
        want = D.expected_from_dump(c, layout)
        for es_off in offs:
            for dst_off in (0, 1, 7, 15):
                got, r = decode(M, D, enc, c["stream"], layout, "module", es_off=es_off, dst_off=dst_off, cap=want.size)
                same(got, want, (layout, es_off, dst_off))
    got, r = decode(M, D, enc, c["stream"], "i420", "module", dst_off=7, cap=want.size - 1)
    assert got is None and r["status"] == D.OVERFLOW and r["out_bytes"] == 0


def test_scan_tile_streams(env, enc):
    """start codes at T - 3 .. T from a multiple of the scan's tile, and a slice, a picture header and a sequence header across one
    (tests/test_dec_cases.py asserts that the streams do that)"""
    M, D = env
    assert M.decode_scan_tile() == D.host_lib().dec_host_scan_tile()
    for s in D.tile_streams():
        want, r = D.host_decode(s, "i420", "module")            # (the CPU file holds the host build to decoder.py on these streams)
        got, rg = decode(M, D, enc, s, "i420", "module")
        same(got, want)
        assert rg["repeated_headers"] == r["repeated_headers"] > 0 and rg["gops"] == r["gops"]


def _oracle(frames, pf, dump=True):
    from oracle import m2v_oracle_ctypes as orc
    return orc.encode(frames, frames.shape[3] // 16, frames.shape[2] // 16, pf, 7, 7, 3, 2, dump=dump)


@pytest.mark.parametrize("W,H,n,pf", ((2048, 64, 2, 1), (64, 2048, 2, 1), (1920, 1152, 9, 8)), ids=("widest", "tallest", "1920x1152"))
def test_extreme_geometry(env, W, H, n, pf):
    """128 macroblocks in a slice and 128 slices, each at the fewest rows / columns the encoder codes (four), and one 1920 x 1152 GOP of
    nine frames - against the oracle's dump, once.  (The smallest geometry, 64 x 64, is recon_cases' "ionly".)"""
    M, D = env
    import recon_cases as R
    frames = M.synth.clip(W, H, n, clip_index=77)
    s, dump = _oracle(frames, pf)
    e = M.Mpeg2Encoder()
    try:
        got, r = decode(M, D, e, s, "i420", "module")
        same(got, R.write_layout(dump["recon"], W, H, "i420"))
    finally:
        e.close()


def test_i_only_62_pictures(env, enc):
    M, D = env
    import desc_cases as DC
    import recon_cases as R
    frames, W, H = DC.ionly()
    s, dump = _oracle(np.asarray(frames), 0)
    got, r = decode(M, D, enc, s, "yv12", "module")
    same(got, R.write_layout(dump["recon"], W, H, "yv12"))
    assert r["pictures"] == r["gops"] == r["chains"] == 62


def test_probe(env, enc):
    """d_dst == NULL: the record is right and nothing is written"""
    M, D = env
    c = D.recon_streams()["fit100x70_i420_true"]
    _, r = decode(M, D, enc, c["stream"], "nv12", "module", probe=True)
    d = M.decoder.decode(c["stream"])
    assert (r["status"], r["pictures"], r["width"], r["height"], r["gops"]) == (D.OK, len(d.pictures), 100, 70, len(d.gops))
    assert r["frame_bytes"] == M.frame_bytes(100, 70, "nv12") and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    # the buffer the handle decoded into last, filled again: a probe behind that decode, with its capacity, leaves it as it is
    import torch
    es = dev(c["stream"])
    ctx = torch.full((int(r["out_bytes"]),), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), es.numel(), ctx.data_ptr(), ctx.numel(), 0, 1, None) == 0
    assert enc.decode_report()["status"] == D.OK and not bool((ctx == D.FILL).all())
    ctx.fill_(D.FILL)
    torch.cuda.synchronize()
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr(), es.numel(), None, ctx.numel(), 0, 1, None) == 0
    r2 = enc.decode_report()
    assert (r2["status"], r2["pictures"], r2["out_bytes"]) == (D.OK, r["pictures"], r["pictures"] * M.frame_bytes(100, 70, "i420"))
    assert bool((ctx == D.FILL).all())


def refusal_cases():
    import dec_cases
    return sorted(list(dec_cases.handmade()) + list(dec_cases.truncations()))


@pytest.mark.parametrize("name", refusal_cases())
def test_refusals(env, enc, name):
    """the hand-made cases and two truncations (each went through the stand-alone sanitizer program of tests/test_dec_cases.py): the
    status is M2V_DEC_SYNTAX, out_bytes 0, nothing written - and the next valid decode on the same handle is right"""
    M, D = env
    x = dict(D.handmade(), **D.truncations())[name]
    _, host = D.host_decode(x, "i420", "module")
    got, r = decode(M, D, enc, x, "i420", "module", cap=1 << 14)
    assert got is None and r["status"] == D.SYNTAX and r["err_offset"] == host["err_offset"]
    s = D.small()
    got, r = decode(M, D, enc, s, "i420", "module")
    same(got, D.frames_of(M.decoder.decode(s, quirks=True)), "the valid decode behind " + name)


@pytest.mark.parametrize("batch", (0, 10), ids=("one_chunk", "chunks_of_10"))
def test_two_bad_slices_in_different_blocks(env, batch):
    """62 I pictures, 248 slices: four blocks of the slice walk in one chunk, or seven chunks.  Slices 21 and 162 are refused; err_offset
    is the earlier one's, the host build's answer, whichever block or chunk is walked first - and the valid decode behind it is right"""
    M, D = env
    x, at = D.two_bad_slices()
    _, host = D.host_decode(x, "i420", "module")
    assert (host["status"], host["err_offset"]) == (D.SYNTAX, at)
    e = M.Mpeg2Encoder()
    try:
        e.set_option("decode_batch", batch)
        got, r = decode(M, D, e, x, "i420", "module", cap=62 * 6144)
        assert got is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0)
        s = D.small()
        got, r = decode(M, D, e, s, "i420", "module")
        same(got, D.frames_of(M.decoder.decode(s, quirks=True)))
    finally:
        e.close()


def test_python_entry(env, enc):
    """Mpeg2Encoder.decode_device: probes, allocates, returns [n, frame_bytes]; a refusal raises with the status and the offset"""
    M, D = env
    c = D.recon_streams()["g80"]
    f, r = enc.decode_device(dev(c["stream"]), "nv12", "module")
    same(f.cpu().numpy(), D.expected_from_dump(c, "nv12"))
    assert enc.decode_report()["pictures"] == r["pictures"] == f.shape[0]
    with pytest.raises(M.M2VError, match=r"M2V_DEC_SYNTAX.*err_offset \d+"):
        enc.decode_device(dev(D.handmade()["picture_type_3"]), "i420", "iso")
    assert enc.decode_report()["status"] == D.SYNTAX
    s = dev(c["stream"])
    assert enc._L.m2v_decode_device(enc._h, s.data_ptr(), s.numel(), None, 0, 4, 0, None) == E_PARAM
    assert enc._L.m2v_decode_device(enc._h, s.data_ptr(), s.numel(), None, 0, 0, 2, None) == E_PARAM


def test_state(env):
    """M2V_E_STATE while a sequence is in progress and between _begin and _end; an encode before and after a decode on one handle gives
    the stream of a fresh handle"""
    M, D = env
    import torch
    c = D.recon_streams()["g80"]
    rgb = torch.from_numpy(np.random.RandomState(4).randint(0, 256, size=(3, 64, 80, 3)).astype(np.uint8)).to("cuda:0")
    fresh = M.Mpeg2Encoder()
    want = fresh.encode_tensor(rgb, 2).cpu().numpy().tobytes()
    fresh.close()
    e = M.Mpeg2Encoder()
    try:
        s = dev(c["stream"])
        args = (e._h, s.data_ptr(), s.numel(), None, 0, 0, 1, None)
        assert e.encode_tensor(rgb, 2).cpu().numpy().tobytes() == want
        got, _ = decode(M, D, e, c["stream"], "i420", "module")
        same(got, D.expected_from_dump(c, "i420"))
        assert e.encode_tensor(rgb, 2).cpu().numpy().tobytes() == want
        # a port sequence in progress
        f444 = M.synth.clip(64, 64, 2, clip_index=3)
        e.push_frames(4, 4, 1, f444[:1])
        assert e._L.m2v_decode_device(*args) == E_STATE
        e.reset()
        # between _begin and _end
        d_in = torch.from_numpy(f444.reshape(2, -1).copy()).to("cuda:0")
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        e.encode_resident_begin(d_in.data_ptr(), 2, d_out.data_ptr(), d_out.numel(), 4, 4, 1)
        assert e._L.m2v_decode_device(*args) == E_STATE
        e.encode_resident_end()
        assert e._L.m2v_decode_device(*args) == 0 and e.decode_report()["status"] == D.OK
    finally:
        e.close()


@pytest.mark.parametrize("name,size", (("fit100x70_444_true", (100, 70)), ("starts", None)), ids=("100x70", "96x64"))
def test_round_trip_on_the_device(env, name, size):
    """decode_device in I420, its output straight into encode_resident420 with the frame size set: the stream is the oracle's for the
    expected frames.  Nothing passes through the host but the comparison"""
    M, D = env
    import torch
    from oracle import m2v_oracle_ctypes as orc
    c = D.recon_streams()[name]
    w, h = size or (c["W"], c["H"])
    want_frames = D.expected_from_dump(c, "i420")
    n = want_frames.shape[0]
    padded = M.pad_frames(want_frames, w, h, "i420") if size else want_frames
    want = orc.encode(M.to444(padded, c["W"], c["H"]), c["W"] // 16, c["H"] // 16, 2, 7, 7, 3, 2)
    e = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        frames, _ = e.decode_device(dev(c["stream"]), "i420", "module")
        if size:
            e.set_frame_size(w, h)
        d_out = torch.empty(1 << 22, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        nb = e.encode_resident420(frames.data_ptr(), n, d_out.data_ptr(), d_out.numel(), c["W"] // 16, c["H"] // 16, 2, "i420")
        assert d_out[:nb].cpu().numpy().tobytes() == want
    finally:
        e.close()


def test_c_caller_and_m2v_tb(env, tmp_path):
    """integration/decode_caller.c (gcc, C99) and m2v_tb -decode write the file planes_of_recon expects"""
    M, D = env
    M.build()
    libdir = os.path.join(ROOT, "fpga-mpeg2-encoder_amd")
    exe = str(tmp_path / "decode_caller")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           os.path.join(ROOT, "integration", "decode_caller.c"), "-L" + libdir, "-lm2v_mi355x", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    c = D.recon_streams()["fit100x70_rgb24_true"]
    (tmp_path / "in.m2v").write_bytes(c["stream"])
    want = D.expected_from_dump(c, "nv12")
    y, u, v = M.planes_of_recon(want, 100, 70, "nv12")
    for out, argv in (("c.yuv", [exe, str(tmp_path / "in.m2v"), str(tmp_path / "c.yuv"), "2", "1"]),
                      ("tb.yuv", [os.path.join(libdir, "m2v_tb"), "-decode", str(tmp_path / "in.m2v"), str(tmp_path / "tb.yuv"), "-reconfmt", "nv12", "-mode", "module"])):
        r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.frombuffer((tmp_path / out).read_bytes(), np.uint8)
        gy, gu, gv = M.planes_of_recon(got, 100, 70, "nv12")
        assert np.array_equal(gy, y) and np.array_equal(gu, u) and np.array_equal(gv, v), out
    (tmp_path / "bad.m2v").write_bytes(D.handmade()["end_code_missing"])
    r = subprocess.run([exe, str(tmp_path / "bad.m2v"), str(tmp_path / "bad.yuv"), "0", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "status -2" in r.stdout
