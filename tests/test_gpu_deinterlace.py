"""-m gpu: m2v_deinterlace_device against deinterlace_frames (the numpy statement of the header's definition) - byte for byte, no
tolerance anywhere.  The cases are those of tests/deint_cases.py at their smallest shapes; tests/test_deint_cases.py runs them through
the host build of the same arithmetic, through an independent reference and against literals.  Every call writes into a buffer of FILL
with guards around exactly the output's bytes."""
import os
import subprocess

import numpy as np
import pytest

import deint_cases as D

pytestmark = pytest.mark.gpu
M = D.M
E_PARAM, E_STATE, E_OVERFLOW = -1, -4, -6
FILL, GUARD = 0xA5, 256
ROOT = D.ROOT


@pytest.fixture(scope="module")
def enc():
    e = M.Mpeg2Encoder(XL=6, YL=6)
    yield e
    e.close()


def dev(a):
    import torch
    a = np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, np.uint8)
    return torch.from_numpy(a.reshape(-1).copy()).to("cuda:0")


def codes(c):
    return M.LAYOUTS_420[c["layout"]], M.DEINT_MODES[c["mode"]], M.DEINT_RATES[c["rate"]], M.DEINT_ORDERS[c["order"]]


def run(enc, c, x, src_off=0, dst_off=0, stream=None):
    """one m2v_deinterlace_device through the C-ABI, the source src_off bytes and the output dst_off bytes behind an allocation's start,
    a capacity of exactly the output's bytes -> the output; asserts the guards"""
    import torch
    w, h = c["size"]
    n = len(x)
    room = M.deinterlace_bound(w, h, n, c["rate"])
    src = torch.cat([torch.zeros(src_off, dtype=torch.uint8, device="cuda:0"), dev(x)])
    buf = torch.full((2 * GUARD + dst_off + room,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    layout, mode, rate, order = codes(c)
    rc = enc._L.m2v_deinterlace_device(enc._h, src.data_ptr() + src_off, n, w, h, layout, mode, rate, order, buf.data_ptr() + GUARD + dst_off, room,
                                       stream.cuda_stream if stream is not None else None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    (stream or torch.cuda).synchronize()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    a, b = GUARD + dst_off, GUARD + dst_off + room
    assert (got[:a] == FILL).all() and (got[b:] == FILL).all(), "bytes outside the output were written"
    return got[a:b].reshape(-1, M.frame_bytes(w, h, c["layout"]))


@pytest.mark.parametrize("c", D.cases(), ids=D.name_of)
def test_cases_on_the_device(enc, c):
    """(fails on a library without the entry: the symbol is absent)"""
    x = D.source(c)
    want = D.expected(c, x)
    got = run(enc, c, x)
    assert got.shape == want.shape and np.array_equal(got, want), (D.name_of(c), int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0]))


@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 1), (3, 7), (7, 3), (1, 1)])
def test_any_byte_address(enc, src_off, dst_off):
    """source and destination at byte offsets 0, 1, 3 and 7 of an allocation, at a width of whole 16-byte lanes and at odd ones"""
    for c in (dict(size=(256, 17), nframes=2, layout="i420", mode="adaptive", rate="field", order="tff"),
              dict(size=(515, 16), nframes=3, layout="nv12", mode="adaptive", rate="frame", order="bff"),
              dict(size=(35, 9), nframes=2, layout="yv12", mode="line", rate="field", order="bff"),
              dict(size=(257, 33), nframes=1, layout="nv21", mode="blend", rate="frame", order="tff")):
        x = D.source(c)
        assert np.array_equal(run(enc, c, x, src_off, dst_off), D.expected(c, x)), D.name_of(c)


def test_python_surface_and_a_stream_of_its_own(enc):
    import torch
    c = dict(size=(48, 32), nframes=3, layout="i420", mode="adaptive", rate="field", order="tff")
    x = D.source(c)
    want = D.expected(c, x)
    s = torch.cuda.Stream()
    assert np.array_equal(run(enc, c, x, stream=s), want)
    d = dev(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = enc.deinterlace_device(d, 48, 32, "i420", "adaptive", "field", "tff")
    s.synchronize()
    assert got.shape == want.shape and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    out = torch.full((want.size + 5,), FILL, dtype=torch.uint8, device="cuda:0")
    got = enc.deinterlace_device(d.reshape(3, -1), 48, 32, out=out, stream=s, rate="field")
    s.synchronize()
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want) and (out[want.size:].cpu().numpy() == FILL).all()
    assert np.array_equal(enc.deinterlace_device(d, 48, 32, mode="blend").cpu().numpy(), M.deinterlace_frames(x, 48, 32, "i420", "blend"))
    assert enc.deinterlace_device(d[:0], 48, 32).shape == (0, x.shape[1])
    with pytest.raises(ValueError):
        enc.deinterlace_device(d[:-1], 48, 32)
    with pytest.raises(ValueError):
        enc.deinterlace_device(d, 48, 32, mode="bob")
    with pytest.raises(M.M2VError):
        enc.deinterlace_device(d, 48, 32, mode="blend", rate="field")


def test_refusals_leave_the_destination_alone(enc):
    """every M2V_E_PARAM and M2V_E_OVERFLOW of the header through the entry itself; cap one byte short writes nothing; overlapping ranges"""
    import torch
    L, h = enc._L, enc._h
    w, hh, n = 48, 32, 3
    fb = M.frame_bytes(w, hh, "i420")
    x = D.clip(w, hh, n, "i420", 5)
    # one allocation: [ source | output ] with room for a field-rate output, so that ranges can be made to overlap
    buf = torch.full((n * fb + 2 * n * fb + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    buf[:n * fb] = dev(x)
    torch.cuda.synchronize()
    src, dst = buf.data_ptr(), buf.data_ptr() + n * fb

    def call(**kw):
        a = dict(src=src, n=n, w=w, h=hh, layout=0, mode=1, rate=0, order=0, dst=dst, cap=n * fb)
        a.update(kw)
        return L.m2v_deinterlace_device(h, a["src"] or None, a["n"], a["w"], a["h"], a["layout"], a["mode"], a["rate"], a["order"], a["dst"] or None, a["cap"], None)
    for kw in (dict(layout=4), dict(layout=-1), dict(mode=3), dict(mode=-1), dict(rate=2), dict(rate=-1), dict(order=2), dict(order=-1),
               dict(mode=2, rate=1, cap=2 * n * fb), dict(w=0), dict(h=1), dict(w=16385), dict(h=16385), dict(src=0), dict(dst=0),
               dict(dst=src), dict(dst=dst - 1), dict(dst=src + fb), dict(src=dst + fb), dict(src=dst + n * fb - 1), dict(rate=1, cap=2 * n * fb, src=dst + 2 * n * fb - 1)):
        assert call(**kw) == E_PARAM, kw
        assert L.m2v_last_error(h).startswith(b"m2v_deinterlace_device: ")
    assert b"overlap" in L.m2v_last_error(h)
    for kw in (dict(cap=n * fb - 1), dict(cap=0), dict(rate=1, cap=2 * n * fb - 1)):
        assert call(**kw) == E_OVERFLOW, kw
    assert call(n=0, cap=0) == 0 and call(n=0, cap=0, src=0, dst=0) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n * fb], x.reshape(-1)) and (got[n * fb:] == FILL).all(), "a refused call wrote"
    # touching ranges are legal
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf[n * fb:2 * n * fb].cpu().numpy(), M.deinterlace_frames(x, w, hh).reshape(-1))


def test_state(enc):
    """M2V_E_STATE where m2v_decode_device answers it: between the halves of a resident call"""
    import torch
    w, hh, n = 48, 32, 2
    fb = M.frame_bytes(w, hh, "i420")
    x = dev(D.clip(w, hh, n, "i420", 6))
    out = torch.full((n * fb,), FILL, dtype=torch.uint8, device="cuda:0")
    d_in = torch.zeros(2 * 3 * 64 * 64, dtype=torch.uint8, device="cuda:0")
    d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    args = (enc._h, x.data_ptr(), n, w, hh, 0, 1, 0, 0, out.data_ptr(), n * fb, None)
    enc.encode_resident_begin(d_in.data_ptr(), 2, d_out.data_ptr(), d_out.numel(), 4, 4, 1)
    try:
        assert enc._L.m2v_deinterlace_device(*args) == E_STATE
    finally:
        enc.encode_resident_end()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()
    assert enc._L.m2v_deinterlace_device(*args) == 0


def chain_stream():
    import ilace_cases as I
    import ilace_writer as IW
    rng = np.random.RandomState(8128)
    return IW.stream(48, 32, I.pictures(rng, "IPP", 3, IW.mb_rows(32, False)))[0]


def test_two_calls_with_a_decode_between(enc):
    """two calls back to back on one handle, a decode_device between them: the handle keeps nothing of a call"""
    import torch
    c = dict(size=(48, 32), nframes=3, layout="i420", mode="adaptive", rate="frame", order="tff")
    x = D.source(c)
    d = dev(x)
    torch.cuda.synchronize()
    a = enc.deinterlace_device(d, 48, 32)
    frames, r = enc.decode_device(dev(chain_stream()), syntax="main", interlaced=True)
    b = enc.deinterlace_device(d, 48, 32, rate="field", order="bff")
    torch.cuda.synchronize()
    assert r["pictures"] == 3 and frames.shape == (3, x.shape[1])
    assert np.array_equal(a.cpu().numpy(), D.expected(c, x))
    assert np.array_equal(b.cpu().numpy(), M.deinterlace_frames(x, 48, 32, "i420", "adaptive", "field", "bff"))


def test_chain_decode_deinterlace_encode(enc):
    """an interlaced 48 x 32 stream decoded on the device, its frames through deinterlace_device into the resident 4:2:0 encode (the
    frames' size set as the source size, the picture 64 x 64): the stream is, byte for byte, the same entry's stream for
    deinterlace_frames(decoder.decode(...).frames) uploaded"""
    import torch
    import dec_cases as DC
    s = chain_stream()
    d = M.decoder.decode(bytes(s), quirks=False, syntax="main", b_pictures=False, interlaced=True)
    woven = DC.frames_of(d, "i420")
    assert woven.shape == (3, M.frame_bytes(48, 32, "i420"))
    d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    enc.set_source_size(48, 32)
    try:
        for mode, rate in (("adaptive", "frame"), ("adaptive", "field"), ("line", "frame")):
            want_frames = M.deinterlace_frames(woven, 48, 32, "i420", mode, rate, "tff")
            assert not np.array_equal(want_frames[0], woven[0])
            up = dev(want_frames)
            torch.cuda.synchronize()
            nb = enc.encode_resident420(up.data_ptr(), len(want_frames), d_out.data_ptr(), d_out.numel(), 4, 4, 2, "i420")
            want = d_out[:nb].cpu().numpy().tobytes()
            enc.set_source_size(0, 0)
            frames, _ = enc.decode_device(dev(s), syntax="main", interlaced=True)
            enc.set_source_size(48, 32)
            prog = enc.deinterlace_device(frames, 48, 32, "i420", mode, rate, "tff")
            torch.cuda.synchronize()
            nb = enc.encode_resident420(prog.data_ptr(), prog.shape[0], d_out.data_ptr(), d_out.numel(), 4, 4, 2, "i420")
            assert d_out[:nb].cpu().numpy().tobytes() == want, (mode, rate)
            assert np.array_equal(prog.cpu().numpy(), want_frames)
    finally:
        enc.set_source_size(0, 0)


def test_m2v_tb_and_c_caller(tmp_path):
    """m2v_tb -decode ... -deint adaptive -fieldrate writes the file the Python path gives; integration/deint_caller.c (gcc, C99) runs
    the chain and writes a stream that decodes to as many pictures as there were fields"""
    import dec_cases as DC
    M.build()
    libdir = os.path.join(ROOT, "fpga-mpeg2-encoder_amd")
    s = chain_stream()
    (tmp_path / "in.m2v").write_bytes(s)
    d = M.decoder.decode(bytes(s), quirks=False, syntax="main", b_pictures=False, interlaced=True)
    woven = DC.frames_of(d, "nv12")
    for flags, (mode, rate, order) in ((["-deint", "adaptive", "-fieldrate"], ("adaptive", "field", "tff")), (["-deint", "blend"], ("blend", "frame", "tff")),
                                       (["-deint", "line", "-bff"], ("line", "frame", "bff"))):
        r = subprocess.run([os.path.join(libdir, "m2v_tb"), "-decode", str(tmp_path / "in.m2v"), str(tmp_path / "tb.yuv"), "-reconfmt", "nv12", "-syntax", "main",
                            "-interlaced"] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.frombuffer((tmp_path / "tb.yuv").read_bytes(), np.uint8)
        assert np.array_equal(got, M.deinterlace_frames(woven, 48, 32, "nv12", mode, rate, order).reshape(-1)), flags
    r = subprocess.run([os.path.join(libdir, "m2v_tb"), "-decode", str(tmp_path / "in.m2v"), str(tmp_path / "tb.yuv"), "-deint", "blend", "-fieldrate"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    exe = str(tmp_path / "deint_caller")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           os.path.join(ROOT, "integration", "deint_caller.c"), "-L" + libdir, "-lm2v_mi355x", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / "in.m2v"), str(tmp_path / "out.m2v"), "1", "1", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "3 woven frames 48 x 32 -> 6 progressive frames" in r.stdout, r.stdout + r.stderr
    out = M.decoder.decode((tmp_path / "out.m2v").read_bytes(), quirks=True)
    assert len(out.frames) == 6
