"""-m gpu: frames of any size (m2v_set_frame_size) through every entry that takes whole frames, byte for byte against the oracle's
stream for the frames padded to whole macroblocks in their own format (M.pad_frames; tests/test_input_fit.py pins that definition).
Every comparison is exact.

Error paths use the library's own checks only."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P6 = (6, 6, 3, 2)
E_PARAM, E_STATE = -1, -4
_want = {}


@pytest.fixture(scope="module")
def env():
    import fit_cases
    return fit_cases.M, fit_cases


@pytest.fixture(scope="module")
def enc6(env):
    M, F = env
    enc = M.Mpeg2Encoder(*P6)
    yield enc
    enc.close()


def want_of(F, planes, pf, params):
    """the oracle's stream for planar 4:4:4 frames [n, 3, H, W], computed once per distinct input (the RGB layouts of one picture, and
    the 4:2:0 layouts of one frame, give the same planes)"""
    key = (hashlib.sha1(planes.tobytes()).hexdigest(), planes.shape, pf, params)
    if key not in _want:
        _, _, H, W = planes.shape
        _want[key] = F.orc.encode(planes, W // 16, H // 16, pf, *params)
    return _want[key]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def pin(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).pin_memory().numpy()


def resident(enc, x, w, h, pf, kind, matrix="bt601", begin=False):
    """one sequence of the w x h frames x [n, bytes] of `kind` through the resident entry of that kind (or its _begin / _end halves)"""
    import torch
    import m2v_load
    M = m2v_load.load()
    xs, ys = M.fit_size(w, h)
    n = x.shape[0]
    d_in = dev(x)
    d_out = torch.empty(n * 3 * 256 * xs * ys * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), xs, ys, pf)
    if kind == "444":
        nb = enc.encode_resident(*a) if not begin else enc.encode_resident_begin(*a)
    elif kind in M.LAYOUTS_420:
        nb = enc.encode_resident420(*a, kind) if not begin else enc.encode_resident420_begin(*a, kind)
    else:
        nb = enc.encode_resident_rgb(*a, kind, matrix) if not begin else enc.encode_resident_rgb_begin(*a, kind, matrix)
    if begin:
        nb = enc.encode_resident_end()
    return d_out[:nb].cpu().numpy().tobytes()


def push(enc, M, x, xs, ys, pf, kind, matrix="bt601"):
    if kind == "444":
        enc.push_frames(xs, ys, pf, x)
    elif kind in M.LAYOUTS_420:
        enc.push_frames420(xs, ys, pf, x, kind)
    else:
        enc.push_rgb(xs, ys, pf, x, kind, matrix)


def push_pull(enc, M, x, xs, ys, pf, kind, out, pos, matrix="bt601"):
    if kind == "444":
        return enc.push_frames_pull(xs, ys, pf, x, out, pos)
    if kind in M.LAYOUTS_420:
        return enc.push_frames420_pull(xs, ys, pf, x, out, pos, kind)
    return enc.push_rgb_pull(xs, ys, pf, x, out, pos, kind, matrix)


def port(enc, M, frames, w, h, pf, path, step=2):
    """one sequence through the port path: frames = [(kind, [1, bytes] frame)] in order, consecutive frames of one kind pushed `step` at
    a time; path: pageable, pinned0 / 1 / 2 (page-locked source, option direct_upload) or pull (the _pull form, page-locked)"""
    xs, ys = M.fit_size(w, h)
    if path != "pageable":
        enc.set_option("direct_upload", {"pinned0": 0, "pinned1": 1, "pinned2": 2, "pull": 1}[path])
    calls, k = [], 0
    while k < len(frames):
        j = k
        while j < len(frames) and j - k < step and frames[j][0] == frames[k][0]:
            j += 1
        block = np.concatenate([f for _, f in frames[k:j]], axis=0)
        calls.append((frames[k][0], block if path == "pageable" else pin(block)))
        k = j
    try:
        if path == "pull":
            out = np.zeros(len(frames) * 3 * 256 * xs * ys * 2 + (1 << 16), np.uint8)
            pos, last = 0, False
            for kind, block in calls:
                m, last = push_pull(enc, M, block, xs, ys, pf, kind, out, pos)
                pos += m
                assert not last
            enc.sequence_stop()
            while not last:
                m, last = enc.pull_into(out, pos)
                pos += m
            return out[:pos].tobytes()
        for kind, block in calls:
            push(enc, M, block, xs, ys, pf, kind)
        if path == "pinned2":
            enc.upload_wait()
        enc.sequence_stop()
        return enc.pull_all()
    finally:
        enc.set_option("direct_upload", 1)


# ---- 1: the pass alone ----
SIZES_PASS = [(w, 49) for w in range(65, 81)] + [(72, h) for h in range(49, 65)]


@pytest.mark.parametrize("kind", ["444", "nv12", "i420", "rgb24", "bgrx", "rgbp"])
def test_pass_alone(env, enc6, kind):
    """every phase of a 16-byte segment against the last column for each element size, 1 to 15 padded columns and rows, odd chroma
    sizes: the padded, converted planes as the macroblock kernel reads them (m2v_debug_read, what = 4)"""
    M, F = env
    for w, h in SIZES_PASS:
        W, H = F.padded(w, h)
        x = F.source(w, h, 1, kind, seed=1000 + w + 100 * h, noise=True)
        enc6.set_frame_size(w, h)
        resident(enc6, x, w, h, 0, kind)
        got = enc6.debug_read(4, 3 * W * H, np.uint8)
        assert got.size == 3 * W * H and np.array_equal(got.reshape(1, 3, H, W), F.planes(x, w, h, kind)), (kind, w, h)
    enc6.set_frame_size(0, 0)


# ---- 2: streams, resident ----
SIZES = [(65, 49), (66, 50), (79, 63), (72, 57), (71, 64), (113, 81)]


@pytest.mark.parametrize("w,h", SIZES)
def test_resident_streams(env, enc6, w, h):
    M, F = env
    enc6.set_frame_size(w, h)
    for k, kind in enumerate(F.KINDS):
        x = F.source(w, h, 3, kind, seed=20 + w)
        matrices = ("bt601", "bt709", "bt601f", "bt709f") if (w, h) == (79, 63) and kind in F.KINDS_RGB else ("bt601",)
        for matrix in matrices:
            want = want_of(F, F.planes(x, w, h, kind, matrix), 2, P6)
            assert resident(enc6, x, w, h, 2, kind, matrix) == want, (kind, matrix)
        if SIZES[k % len(SIZES)] == (w, h):               # the two halves: one size per kind
            assert resident(enc6, x, w, h, 2, kind, begin=True) == want_of(F, F.planes(x, w, h, kind), 2, P6), kind
    enc6.set_frame_size(0, 0)


@pytest.mark.parametrize("VL,w,h", [(1, 79, 63), (2, 66, 50)])
def test_resident_streams_vector_levels(env, VL, w, h):
    M, F = env
    params = (6, 6, VL, 2)
    enc = M.Mpeg2Encoder(*params)
    try:
        enc.set_frame_size(w, h)
        for kind in F.KINDS:
            x = F.source(w, h, 3, kind, seed=40 + VL)
            assert resident(enc, x, w, h, 2, kind) == want_of(F, F.planes(x, w, h, kind), 2, params), kind
    finally:
        enc.close()


# ---- 3: streams, port path ----
PORT_KINDS = ("444", "i420", "nv21", "rgb24", "xbgr")
PATHS = ("pageable", "pinned0", "pinned1", "pinned2", "pull")


@pytest.fixture(scope="module")
def enc_port(env):
    M, F = env
    enc = M.Mpeg2Encoder(*P6)
    enc.set_option("batch_frames", 3)
    yield enc
    enc.close()


@pytest.mark.parametrize("w,h", [(71, 55), (66, 50)])
@pytest.mark.parametrize("kind", PORT_KINDS)
def test_port_streams(env, enc_port, kind, w, h):
    """7 frames, chunks of 3, pushed 2 at a time: chunks and calls do not line up"""
    M, F = env
    x = F.source(w, h, 7, kind, seed=60 + w)
    want = want_of(F, F.planes(x, w, h, kind), 2, P6)
    enc_port.set_frame_size(w, h)
    for path in PATHS:
        assert port(enc_port, M, [(kind, x[k:k + 1]) for k in range(7)], w, h, 2, path) == want, path
    enc_port.set_frame_size(0, 0)


def test_port_alternating_kinds_and_two_sizes(env, enc_port):
    """every frame of another kind; then a second sequence of another size on the same handle"""
    M, F = env
    for (w, h), path in (((71, 55), "pageable"), ((66, 50), "pinned1"), ((113, 81), "pull")):
        frames, planes = [], []
        for k in range(7):
            kind = PORT_KINDS[k % 5]
            x = F.source(w, h, 7, kind, seed=80 + w)[k:k + 1]
            frames.append((kind, x))
            planes.append(F.planes(x, w, h, kind))
        enc_port.set_frame_size(w, h)
        assert port(enc_port, M, frames, w, h, 2, path, step=1) == want_of(F, np.concatenate(planes, axis=0), 2, P6), (w, h, path)
    enc_port.set_frame_size(0, 0)


# ---- 4: the header ----
def test_header_true_and_module(env, enc6, enc_port):
    M, F = env
    w, h = 71, 55
    for kind in ("i420", "rgb24", "444"):
        x = F.source(w, h, 3, kind, seed=90)
        want = want_of(F, F.planes(x, w, h, kind), 2, P6)
        true = M.set_header_size(want, w, h)
        assert true != want
        for enc in (enc6, enc_port):
            enc.set_frame_size(w, h, "true")
        got = resident(enc6, x, w, h, 2, kind)
        assert got == true, kind
        assert port(enc_port, M, [(kind, x[k:k + 1]) for k in range(3)], w, h, 2, "pageable") == true, kind
        for enc in (enc6, enc_port):
            enc.set_frame_size(w, h, "module")
        assert resident(enc6, x, w, h, 2, kind) == want, kind
        assert port(enc_port, M, [(kind, x[k:k + 1]) for k in range(3)], w, h, 2, "pinned1") == want, kind
    d = M.decoder.decode(got)
    assert (d.width, d.height) == (w, h) and len(d.frames) == 3
    assert all(f[0].shape == (h, w) and f[1].shape == f[2].shape == (28, 36) for f in d.frames)
    full = M.decoder.decode(want)
    assert all(np.array_equal(a[0][:h, :w], b[0]) for a, b in zip(full.frames, d.frames))
    for enc in (enc6, enc_port):
        enc.set_frame_size(0, 0)


# ---- 5: full size once ----
@pytest.mark.parametrize("kind", ["i420", "rgb24"])
def test_full_size_1080(env, kind):
    M, F = env
    w, h, params = 1920, 1080, (7, 7, 3, 2)
    x = F.source(w, h, 2, kind, seed=5, noise=True)
    want = want_of(F, F.planes(x, w, h, kind), 1, params)
    enc = M.Mpeg2Encoder(*params)
    try:
        enc.set_frame_size(w, h)
        assert M.fit_size(w, h) == (120, 68)
        assert resident(enc, x, w, h, 1, kind) == want
        if kind == "i420":
            enc.set_frame_size(w, h, "true")
            got = resident(enc, x, w, h, 1, kind)
            assert got == M.set_header_size(want, w, h)
            assert int.from_bytes(got[4:7], "big") == (1920 << 12) | 1080
    finally:
        enc.close()


# ---- 6: no-op and errors ----
def test_noop_and_errors(env):
    import torch
    M, F = env
    enc = M.Mpeg2Encoder(*P6)
    L, hd = enc._L, enc._h
    try:
        # a size of whole macroblocks: the same bytes as no size set
        x = F.source(80, 64, 3, "444", seed=7)
        want = want_of(F, x.reshape(3, 3, 64, 80), 2, P6)
        assert resident(enc, x, 80, 64, 2, "444") == want
        enc.set_frame_size(80, 64, "true")
        assert resident(enc, x, 80, 64, 2, "444") == want
        assert port(enc, M, [("444", x)], 80, 64, 2, "pageable", step=3) == want
        y = F.source(80, 64, 3, "nv12", seed=7)
        assert resident(enc, y, 80, 64, 2, "nv12") == want_of(F, F.planes(y, 80, 64, "nv12"), 2, P6)
        enc.set_frame_size(0, 0)
        # arguments
        for w, h, hdr in ((48, 64, 0), (64, 48, 0), (0, 55, 0), (71, 0, 0), (-71, 55, 0), (71, -1, 0), ((16 << 6) + 1, 64, 0), (64, (16 << 6) + 1, 0),
                          (71, 55, 2), (71, 55, -1), (0, 0, 7)):
            assert L.m2v_set_frame_size(hd, w, h, hdr) == E_PARAM, (w, h, hdr)
            assert L.m2v_last_error(hd)
        assert L.m2v_set_frame_size(hd, 16 << 6, 16 << 6, 1) == 0 and L.m2v_set_frame_size(hd, 49, 49, 0) == 0
        # busy
        w, h = 71, 55
        xs, ys = M.fit_size(w, h)
        z = F.source(w, h, 3, "i420", seed=8)
        want = want_of(F, F.planes(z, w, h, "i420"), 2, P6)
        enc.set_frame_size(w, h)
        enc.push_frames420(xs, ys, 2, z[:1], "i420")
        assert enc.busy and L.m2v_set_frame_size(hd, 66, 50, 0) == E_STATE and L.m2v_set_frame_size(hd, 0, 0, 0) == E_STATE
        enc.push_frames420(xs, ys, 2, z[1:], "i420")
        enc.sequence_stop()
        assert enc.pull_all() == want and not enc.busy
        # reset keeps the setting
        enc.reset()
        assert resident(enc, z, w, h, 2, "i420") == want
        # a wrong xsize16 / ysize16 on the starting call: nothing started
        d_in, d_out = dev(z), torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        n = ctypes.c_size_t(0)
        for bad in ((xs - 1, ys), (xs, ys + 1), (xs + 1, ys)):
            assert L.m2v_encode_resident420(hd, bad[0], bad[1], 2, d_in.data_ptr(), 3, 0, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == E_PARAM
            assert L.m2v_push_frames420(hd, bad[0], bad[1], 2, z.ctypes.data, 3, 0) == E_PARAM
            assert L.m2v_push_frames(hd, bad[0], bad[1], 2, z.ctypes.data, 1) == E_PARAM
            assert not enc.busy
        assert resident(enc, z, w, h, 2, "i420") == want
        # the port has no partial macroblock, strips take whole padded frames
        b = np.zeros(64, np.uint8)
        assert L.m2v_push_beats(hd, xs, ys, 2, b.ctypes.data, b.ctypes.data, b.ctypes.data, 16, 0) == E_STATE
        assert b"frame size" in L.m2v_last_error(hd)
        assert L.m2v_push_packed(hd, xs, ys, 2, b.ctypes.data, 4, 0, 0) == E_STATE
        assert L.m2v_strip_begin(hd, xs, ys, 2, d_in.data_ptr(), 1, 0, ys, None) == E_STATE
        assert b"strips" in L.m2v_last_error(hd)
        assert not enc.busy
        assert port(enc, M, [("i420", z)], w, h, 2, "pageable", step=3) == want
        # off again: frames are W x H
        enc.set_frame_size(0, 0)
        assert enc.frame_size is None
        # ... at once: a sequence that beats start, whole frames behind them - nothing of the old size is left on the handle
        f = x.reshape(3, 3, -1)
        enc.push_beats(5, 4, 2, f[0, 0], f[0, 1], f[0, 2])
        enc.push_frames(5, 4, 2, x[1:])
        enc.sequence_stop()
        assert enc.pull_all() == want_of(F, x.reshape(3, 3, 64, 80), 2, P6)
        assert resident(enc, x, 80, 64, 2, "444") == want_of(F, x.reshape(3, 3, 64, 80), 2, P6)
    finally:
        enc.close()


# ---- 7: the torch entry ----
def test_encode_tensor_any_size(env):
    """header= is what asks for padding: tests/test_gpu_input_rgb.py::test_encode_tensor holds encode_tensor without it to a ValueError
    for a 72 x 64 tensor, so the keyword has no default that pads"""
    import torch
    M, F = env
    w, h, n, pf = 71, 55, 3, 2
    enc = M.Mpeg2Encoder(*P6)
    try:
        hwc = F.source(w, h, n, "rgb24", seed=70).reshape(n, h, w, 3)     # one picture in three forms
        p = F.source(w, h, n, "rgbp", seed=70).reshape(n, 3, h, w)
        want = want_of(F, F.planes(hwc.reshape(n, -1), w, h, "rgb24"), pf, P6)
        true = M.set_header_size(want, w, h)
        x4 = F.source(w, h, n, "xrgb", seed=70).reshape(n, h, w, 4)
        enc.set_frame_size(66, 50, "module")                             # the handle's own setting: back afterwards
        assert enc.encode_tensor(dev(hwc), pf, header="true").cpu().numpy().tobytes() == true
        assert enc.frame_size == (66, 50, 0)
        assert enc.encode_tensor(dev(x4), pf, order="xrgb", header="true").cpu().numpy().tobytes() == true
        assert enc.encode_tensor(dev(p), pf, header="true").cpu().numpy().tobytes() == true     # [n, 3, h, w]
        assert enc.encode_tensor(dev(hwc), pf, header="module").cpu().numpy().tobytes() == want
        assert enc.encode_tensor(dev(p), pf, header="module").cpu().numpy().tobytes() == want
        with pytest.raises(ValueError):
            enc.encode_tensor(dev(hwc), pf, header="nosuch")
        with pytest.raises(ValueError):
            enc.encode_tensor(dev(hwc), pf)                              # padding is asked for with the keyword: without it, as ever
        with pytest.raises(ValueError):
            enc.encode_tensor(torch.zeros((1, 48, 71, 3), dtype=torch.uint8, device="cuda:0"), pf, header="true")   # pads to 48 rows: below 64
        assert enc.frame_size == (66, 50, 0)
        # the setting really is back: a 66 x 50 frame goes in
        y = F.source(66, 50, 3, "444", seed=71)
        assert resident(enc, y, 66, 50, 2, "444") == want_of(F, F.planes(y, 66, 50, "444"), 2, P6)
        # whole macroblocks with a setting on the handle: as ever
        t = F.source(80, 64, n, "rgb24", seed=72).reshape(n, 64, 80, 3)
        assert enc.encode_tensor(dev(t), pf).cpu().numpy().tobytes() == want_of(F, M.rgb_to444(t.reshape(n, -1), 80, 64, "rgb24"), pf, P6)
        assert enc.frame_size == (66, 50, 0)
        assert enc.encode_tensor(dev(t), pf, header="true").cpu().numpy().tobytes() == want_of(F, M.rgb_to444(t.reshape(n, -1), 80, 64, "rgb24"), pf, P6)
        enc.set_frame_size(0, 0)
        assert enc.encode_tensor(dev(hwc), pf, header="true").cpu().numpy().tobytes() == true
        assert enc.frame_size is None
    finally:
        enc.close()


# ---- 8: m2v_tb ----
def test_tb_pad(env, tmp_path):
    M, F = env
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    assert os.path.exists(tb), "m2v_tb is built by __graft_entry__.build()"
    w, h, n = 71, 55, 3
    x = F.source(w, h, n, "i420", seed=33)
    fin, fout = tmp_path / "in.yuv", tmp_path / "out.m2v"
    fin.write_bytes(x.tobytes() + b"\x55" * 100)                         # a trailing partial frame is ignored (TB:220)
    want = want_of(F, F.planes(x, w, h, "i420"), 23, (7, 6, 3, 2))
    tail = [str(fin), str(w), str(h), str(fout)]
    r = subprocess.run([tb, "-pad", "-i420"] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert fout.read_bytes() == want
    r = subprocess.run([tb, "-truesize", "-i420"] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert fout.read_bytes() == M.set_header_size(want, w, h)
    r = subprocess.run([tb, "-i420"] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "*** xsize=  71 is invalid, which must in range [64,2048], and must be a multiple of 16" in r.stdout
    r = subprocess.run([tb, "-i420", str(fin), "80", str(h), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "*** ysize=  55 is invalid, which must in range [64,1024], and must be a multiple of 16" in r.stdout
    r = subprocess.run([tb, "-pad", "-bubbles"] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage:" in r.stderr
