"""-m gpu: frames of another size (m2v_set_source_size) through the resident entries, byte for byte against the oracle's stream for
pad_frames(scale_frames(x)) (tests/test_input_scale.py pins that definition and the library's arithmetic on the CPU).  Every comparison
is exact.

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
    import scale_cases
    return scale_cases.M, scale_cases.F, scale_cases


@pytest.fixture(scope="module")
def enc6(env):
    M, F, S = env
    enc = M.Mpeg2Encoder(*P6)
    yield enc
    enc.close()


def want_of(F, planes, pf, params):
    """the oracle's stream for planar 4:4:4 frames [n, 3, H, W], computed once per distinct input"""
    key = (hashlib.sha1(planes.tobytes()).hexdigest(), planes.shape, pf, params)
    if key not in _want:
        _, _, H, W = planes.shape
        _want[key] = F.orc.encode(planes, W // 16, H // 16, pf, *params)
    return _want[key]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def resident(enc, x, w, h, pf, kind, matrix="bt601", begin=False):
    """one sequence of the frames x [n, bytes] of `kind` (of whatever size the handle is set to take) at picture size w x h through the
    resident entry of that kind (or its _begin / _end halves)"""
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


def set_sizes(enc, sw, sh, w, h, filter="triangle", header="module"):
    """the picture size (a frame size only where it is not whole macroblocks) and the source size"""
    enc.set_frame_size(*((w, h, header) if w % 16 or h % 16 else (0, 0)))
    enc.set_source_size(sw, sh, filter)


def clear(enc):
    enc.set_frame_size(0, 0)
    enc.set_source_size(0, 0)


# ---- 1: the pass alone ----
@pytest.mark.parametrize("filter", ["triangle", "area"])
@pytest.mark.parametrize("kind", ["444", "i420", "nv12", "rgb24", "bgrx", "rgbp"])
def test_pass_alone(env, enc6, kind, filter):
    """the resampled, padded, converted planes as the macroblock kernel reads them (m2v_debug_read, what = 4): integer ratios, none,
    8 : 1 with taps past both edges, enlarging, identity in one dimension, every count of padded columns and rows"""
    M, F, S = env
    for (sw, sh), (w, h) in S.PASS_SIZES:
        W, H = F.padded(w, h)
        x = F.source(sw, sh, 1, kind, seed=1000 + sw + w + 100 * h, noise=True)
        set_sizes(enc6, sw, sh, w, h, filter)
        resident(enc6, x, w, h, 0, kind)
        got = enc6.debug_read(4, 3 * W * H, np.uint8)
        assert got.size == 3 * W * H and np.array_equal(got.reshape(1, 3, H, W), S.planes(x, sw, sh, w, h, kind, filter)), (kind, filter, sw, sh, w, h)
    clear(enc6)


# ---- 2: streams, resident ----
SIZES = [((142, 98), (71, 49)), ((97, 131), (79, 63)), ((160, 128), (80, 64))]          # (the last: no padding, and no frame size is set)


@pytest.mark.parametrize("src,pic", SIZES)
def test_resident_streams(env, enc6, src, pic):
    M, F, S = env
    (sw, sh), (w, h) = src, pic
    for k, kind in enumerate(F.KINDS):
        filter = S.FILTERS[k % 2]
        set_sizes(enc6, sw, sh, w, h, filter)
        x = F.source(sw, sh, 3, kind, seed=20 + sw)
        matrices = ("bt601", "bt709", "bt601f", "bt709f") if pic == (79, 63) and kind in F.KINDS_RGB else ("bt601",)
        for matrix in matrices:
            want = want_of(F, S.planes(x, sw, sh, w, h, kind, filter, matrix), 2, P6)
            assert resident(enc6, x, w, h, 2, kind, matrix) == want, (kind, matrix)
        if SIZES[k % len(SIZES)] == (src, pic):           # the two halves: one size per kind
            assert resident(enc6, x, w, h, 2, kind, begin=True) == want_of(F, S.planes(x, sw, sh, w, h, kind, filter), 2, P6), kind
    clear(enc6)


@pytest.mark.parametrize("VL,src,pic,batch", [(1, (97, 131), (79, 63), 96), (2, (142, 98), (71, 49), 96), (3, (97, 131), (79, 63), 2)])
def test_resident_streams_vector_levels_and_chunks(env, VL, src, pic, batch):
    """VECTOR_LEVEL 1 and 2, and batch_frames 2: a chunk boundary falls inside the three frames"""
    M, F, S = env
    (sw, sh), (w, h) = src, pic
    params = (6, 6, VL, 2)
    enc = M.Mpeg2Encoder(*params)
    try:
        enc.set_option("batch_frames", batch)
        for k, kind in enumerate(F.KINDS):
            filter = S.FILTERS[(k + 1) % 2]
            set_sizes(enc, sw, sh, w, h, filter)
            x = F.source(sw, sh, 3, kind, seed=40 + VL)
            assert resident(enc, x, w, h, 2, kind) == want_of(F, S.planes(x, sw, sh, w, h, kind, filter), 2, params), kind
    finally:
        enc.close()


# ---- 3: the header ----
def test_header_true_and_module(env, enc6):
    M, F, S = env
    (sw, sh), (w, h) = (142, 98), (71, 55)
    for kind in ("i420", "rgb24", "444"):
        x = F.source(sw, sh, 3, kind, seed=90)
        want = want_of(F, S.planes(x, sw, sh, w, h, kind), 2, P6)
        true = M.set_header_size(want, w, h)
        assert true != want
        set_sizes(enc6, sw, sh, w, h, header="true")
        got = resident(enc6, x, w, h, 2, kind)
        assert got == true, kind
        set_sizes(enc6, sw, sh, w, h, header="module")
        assert resident(enc6, x, w, h, 2, kind) == want, kind
    d = M.decoder.decode(got)
    assert (d.width, d.height) == (w, h) and len(d.frames) == 3
    assert all(f[0].shape == (h, w) and f[1].shape == f[2].shape == (28, 36) for f in d.frames)
    clear(enc6)


# ---- 4: no-op and errors ----
def test_noop_and_errors(env):
    import torch
    M, F, S = env
    enc = M.Mpeg2Encoder(*P6)
    L, hd = enc._L, enc._h
    try:
        # a source of the picture size: the same bytes as none set, with and without a frame size
        x = F.source(80, 64, 3, "444", seed=7)
        want = want_of(F, x.reshape(3, 3, 64, 80), 2, P6)
        assert resident(enc, x, 80, 64, 2, "444") == want
        enc.set_source_size(80, 64, "area")
        assert enc.source_size == (80, 64, 1)
        assert resident(enc, x, 80, 64, 2, "444") == want
        y = F.source(71, 55, 3, "nv12", seed=7)
        enc.set_frame_size(71, 55)
        enc.set_source_size(71, 55)
        assert resident(enc, y, 71, 55, 2, "nv12") == want_of(F, F.planes(y, 71, 55, "nv12"), 2, P6)
        clear(enc)
        # arguments
        for sw, sh, f in ((-1, 5, 0), (5, -1, 0), (0, 5, 0), (5, 0, 0), (16385, 5, 0), (5, 16385, 0), (5, 5, 2), (5, 5, -1), (0, 0, 7)):
            assert L.m2v_set_source_size(hd, sw, sh, f) == E_PARAM, (sw, sh, f)
            assert L.m2v_last_error(hd)
        assert L.m2v_set_source_size(hd, 16384, 16384, 1) == 0 and L.m2v_set_source_size(hd, 1, 1, 0) == 0 and L.m2v_set_source_size(hd, 0, 0, 1) == 0
        # busy
        (sw, sh), (w, h) = (142, 98), (71, 49)
        xs, ys = M.fit_size(w, h)
        z = F.source(sw, sh, 3, "i420", seed=8)
        want = want_of(F, S.planes(z, sw, sh, w, h, "i420"), 2, P6)
        set_sizes(enc, sw, sh, w, h)
        d_in, d_out = dev(z), torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        enc.encode_resident420_begin(d_in.data_ptr(), 3, d_out.data_ptr(), d_out.numel(), xs, ys, 2, "i420")
        assert L.m2v_set_source_size(hd, 100, 100, 0) == E_STATE and L.m2v_set_source_size(hd, 0, 0, 0) == E_STATE
        nb = enc.encode_resident_end()
        assert d_out[:nb].cpu().numpy().tobytes() == want
        # reset keeps the setting
        enc.reset()
        assert resident(enc, z, w, h, 2, "i420") == want
        # more than 8 times the picture: refused by the starting call with nothing started, and the next legal call is right
        enc.set_source_size(569, 392)
        big = dev(np.zeros((1, M.frame_bytes(569, 392, "i420")), np.uint8))
        n = ctypes.c_size_t(0)
        assert L.m2v_encode_resident420(hd, xs, ys, 2, big.data_ptr(), 1, 0, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == E_PARAM
        text = L.m2v_last_error(hd)
        assert b"569 x 392" in text and b"71 x 49" in text and b"m2v_set_source_size" in text
        assert not enc.busy
        enc.set_source_size(71, 393)
        assert L.m2v_encode_resident420(hd, xs, ys, 2, big.data_ptr(), 1, 0, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == E_PARAM
        assert not enc.busy
        enc.set_source_size(sw, sh)
        assert resident(enc, z, w, h, 2, "i420") == want
        # the port and the strips resample nothing
        b = np.zeros(1 << 16, np.uint8)
        out, last = np.zeros(1 << 16, np.uint8), ctypes.c_int(0)
        ptrs = (ctypes.c_void_p * 1)(d_in.data_ptr())
        refusals = (
            lambda: L.m2v_push_frames(hd, xs, ys, 2, b.ctypes.data, 1),
            lambda: L.m2v_push_frames420(hd, xs, ys, 2, b.ctypes.data, 1, 0),
            lambda: L.m2v_push_rgb(hd, xs, ys, 2, b.ctypes.data, 1, 0, 0),
            lambda: L.m2v_push_frames_pull(hd, xs, ys, 2, b.ctypes.data, 1, out.ctypes.data, out.size, ctypes.byref(last)),
            lambda: L.m2v_push_frames420_pull(hd, xs, ys, 2, b.ctypes.data, 1, 0, out.ctypes.data, out.size, ctypes.byref(last)),
            lambda: L.m2v_push_rgb_pull(hd, xs, ys, 2, b.ctypes.data, 1, 0, 0, out.ctypes.data, out.size, ctypes.byref(last)),
            lambda: L.m2v_strip_assemble(hd, xs, ys, 2, 1, 1, ptrs, ptrs, d_out.data_ptr(), d_out.numel(), None, None),
            lambda: L.m2v_push_beats(hd, xs, ys, 2, b.ctypes.data, b.ctypes.data, b.ctypes.data, 16, 0),
            lambda: L.m2v_push_packed(hd, xs, ys, 2, b.ctypes.data, 4, 0, 0),
            lambda: L.m2v_strip_begin(hd, xs, ys, 2, d_in.data_ptr(), 1, 0, ys, None),
        )
        enc.set_frame_size(0, 0)                          # (a frame size has refusals of its own for some of these)
        for k, call in enumerate(refusals):
            assert call() == E_STATE, k
            assert b"m2v_set_source_size" in L.m2v_last_error(hd), k
            assert not enc.busy
        assert b"strips" in L.m2v_last_error(hd)
        # off again: frames are W x H, at once and through every path
        enc.set_source_size(0, 0)
        assert enc.source_size is None
        enc.push_frames(5, 4, 2, x)
        enc.sequence_stop()
        assert enc.pull_all() == want_of(F, x.reshape(3, 3, 64, 80), 2, P6)
        assert resident(enc, x, 80, 64, 2, "444") == want_of(F, x.reshape(3, 3, 64, 80), 2, P6)
    finally:
        enc.close()


# ---- 5: with the rest ----
def _composed(env, c, x, sw, sh, filter):
    """one resident call of the settings c (tests/compose_cases.py) fed the sw x sh frames x with the source size set, against
    expected() of the same call fed scale_frames(x) at the picture size; a sentinel around every output"""
    import torch
    import compose_cases as C
    M, F, S = env
    D = C.D
    w, h, header = c["geom"]
    xs, ys = M.fit_size(w, h)
    C.MATERIAL["scale"] = S.scaled(x, sw, sh, w, h, c["kind"], filter)
    want = C.expected(c)
    n = len(x)
    enc = M.Mpeg2Encoder(6, 6, *c["vlq"])
    try:
        enc.set_frame_size(*((w, h, header) if header else (0, 0)))
        enc.set_source_size(sw, sh, filter)
        enc.set_option("stats", c["stats"])
        if C.starts_of(c):
            enc.set_gop_starts(C.starts_of(c))
        if c["desc"]:
            enc.set_stream_desc(D.struct(C.desc_of(c)))
        if C.lengths_of(c):
            enc.set_sequences(C.lengths_of(c))
        d_out = torch.full((C.stream_room(c),), C.SENTINEL, dtype=torch.uint8, device="cuda:0")
        nbytes = n * M.frame_bytes(w, h, c["recon"])
        d_recon = torch.full((nbytes + C.GUARD,), C.FILL, dtype=torch.uint8, device="cuda:0")
        enc.set_recon_out(d_recon.data_ptr(), nbytes, c["recon"])
        d_mux = torch.full((C.mux_room(c),), C.SENTINEL, dtype=torch.uint8, device="cuda:0")
        enc.set_mux_out(c["mux"], d_mux.data_ptr(), d_mux.numel())
        d_in = dev(x)
        torch.cuda.synchronize()
        nb = enc.encode_resident420(d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), xs, ys, c["pf"], c["kind"])
        got = dict(stream_buf=d_out.cpu().numpy(), nbytes=nb, recon_buf=d_recon.cpu().numpy(), mux_buf=d_mux.cpu().numpy(),
                   sequence_report=enc.sequence_report(), gop_report=enc.gop_report(), scene_report=enc.scene_report(),
                   picture_stats=enc.picture_stats(), mux_report=enc.mux_report())
        C.check(got, want, "scaled")
    finally:
        enc.close()
        C.MATERIAL.pop("scale", None)


@pytest.mark.parametrize("with_list", [True, False])
def test_with_the_rest(env, with_list):
    """the source size together with "stats", a reconstruction buffer, a description with repeated headers, a TS container and - a
    batch and a GOP list refuse each other - a GOP list in one call, a batch of two clips in the other"""
    import compose_cases as C
    M, F, S = env
    (sw, sh), (w, h) = (150, 105), (100, 70)
    x = F.source(sw, sh, C.N, "i420", seed=C.CLIP_INDEX)
    c = C.call(geom=(w, h, "true"), kind="i420", stats=1, recon="i420", desc="repeat", mux="ts", material="scale",
               **(dict(layout="list") if with_list else dict(seqs=(5, 7))))
    _composed(env, c, x, sw, sh, "triangle" if with_list else "area")


# ---- 6: the torch entry ----
def test_encode_tensor_size(env):
    import torch
    M, F, S = env
    (sw, sh), (w, h), n, pf = (142, 98), (71, 55), 3, 2
    enc = M.Mpeg2Encoder(*P6)
    try:
        hwc = F.source(sw, sh, n, "rgb24", seed=70)
        p = F.source(sw, sh, n, "rgbp", seed=70)
        x4 = F.source(sw, sh, n, "xrgb", seed=70)
        want = {f: want_of(F, S.planes(hwc, sw, sh, w, h, "rgb24", f), pf, P6) for f in S.FILTERS}
        assert want["triangle"] != want["area"]
        true = M.set_header_size(want["triangle"], w, h)
        enc.set_frame_size(66, 50, "module")                             # the handle's own settings: back afterwards
        enc.set_source_size(100, 90, "area")
        assert enc.encode_tensor(dev(hwc.reshape(n, sh, sw, 3)), pf, header="true", size=(w, h)).cpu().numpy().tobytes() == true
        assert enc.frame_size == (66, 50, 0) and enc.source_size == (100, 90, 1)
        assert enc.encode_tensor(dev(x4.reshape(n, sh, sw, 4)), pf, order="xrgb", header="true", size=(w, h)).cpu().numpy().tobytes() == true
        assert enc.encode_tensor(dev(p.reshape(n, 3, sh, sw)), pf, header="module", size=(w, h), filter="area").cpu().numpy().tobytes() == want["area"]
        assert enc.frame_size == (66, 50, 0) and enc.source_size == (100, 90, 1)
        # a picture size of whole macroblocks needs no header=; one that is not still does
        t = F.source(sw, sh, n, "rgb24", seed=72)
        assert enc.encode_tensor(dev(t.reshape(n, sh, sw, 3)), pf, size=(80, 64)).cpu().numpy().tobytes() == \
            want_of(F, S.planes(t, sw, sh, 80, 64, "rgb24"), pf, P6)
        with pytest.raises(ValueError):
            enc.encode_tensor(dev(hwc.reshape(n, sh, sw, 3)), pf, size=(w, h))
        with pytest.raises(ValueError):
            enc.encode_tensor(dev(hwc.reshape(n, sh, sw, 3)), pf, header="true", size=(w, h), filter="cubic")
        with pytest.raises(ValueError):
            enc.encode_tensor(dev(hwc.reshape(n, sh, sw, 3)), pf, header="true", size=(17, 49))        # 142 is more than 8 x 17
        with pytest.raises(ValueError):
            enc.encode_tensor(dev(hwc.reshape(n, sh, sw, 3)), pf, header="true", size=(w,))
        # without size= the tensor is the picture, whatever the handle holds
        u = F.source(80, 64, n, "rgb24", seed=73)
        assert enc.encode_tensor(dev(u.reshape(n, 64, 80, 3)), pf).cpu().numpy().tobytes() == want_of(F, M.rgb_to444(u, 80, 64, "rgb24"), pf, P6)
        assert enc.frame_size == (66, 50, 0) and enc.source_size == (100, 90, 1)
        # the settings really are back: a 100 x 90 frame goes in and a 66 x 50 picture comes out
        v = F.source(100, 90, 3, "444", seed=71)
        assert resident(enc, v, 66, 50, 2, "444") == want_of(F, S.planes(v, 100, 90, 66, 50, "444", "area"), 2, P6)
        # encode_batch passes both keywords through
        clear(enc)
        stream, offsets = enc.encode_batch(dev(hwc.reshape(n, sh, sw, 3)), pf, lengths=[1, 2], header="module", size=(w, h), filter="area")
        pl = S.planes(hwc, sw, sh, w, h, "rgb24", "area")
        s = stream.cpu().numpy().tobytes()
        assert s[offsets[0]:offsets[0] + len(want_of(F, pl[:1], pf, P6))] == want_of(F, pl[:1], pf, P6)
        assert s[offsets[1]:offsets[2]] == want_of(F, pl[1:], pf, P6)
        assert enc.frame_size is None and enc.source_size is None
    finally:
        enc.close()


# ---- 7: m2v_tb ----
def test_tb_scale(env, tmp_path):
    M, F, S = env
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    assert os.path.exists(tb), "m2v_tb is built by __graft_entry__.build()"
    (sw, sh), (w, h), n = (142, 98), (71, 55), 3
    x = F.source(sw, sh, n, "i420", seed=33)
    fin, fout = tmp_path / "in.yuv", tmp_path / "out.m2v"
    fin.write_bytes(x.tobytes() + b"\x55" * 100)                         # a trailing partial frame is ignored (TB:220)
    tail = [str(fin), str(w), str(h), str(fout)]
    for f in S.FILTERS:
        want = want_of(F, S.planes(x, sw, sh, w, h, "i420", f), 23, (7, 6, 3, 2))
        r = subprocess.run([tb, "-pad", "-i420", "-scale", "%dx%d" % (sw, sh), "-filter", f] + tail, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert fout.read_bytes() == want, f
    r = subprocess.run([tb, "-truesize", "-i420", "-scale", "%dx%d" % (sw, sh)] + tail, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert fout.read_bytes() == M.set_header_size(want_of(F, S.planes(x, sw, sh, w, h, "i420"), 23, (7, 6, 3, 2)), w, h)
    for bad in (["-scale", "142"], ["-scale", "142x"], ["-scale", "0x98"], ["-scale", "142x98x3"], ["-scale", "16385x98"], ["-scale", "142x98", "-filter", "cubic"],
                ["-scale", "142x98", "-bubbles"]):
        r = subprocess.run([tb, "-pad", "-i420"] + bad + tail, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "usage:" in r.stderr, bad


# ---- 8: full size once ----
@pytest.mark.parametrize("kind,filter", [("i420", "triangle"), ("rgb24", "area")])
def test_full_size_1080_to_720(env, kind, filter):
    M, F, S = env
    (sw, sh), (w, h), params = (1920, 1080), (1280, 720), (7, 7, 3, 2)
    x = F.source(sw, sh, 2, kind, seed=5, noise=True)
    want = want_of(F, S.planes(x, sw, sh, w, h, kind, filter), 1, params)
    enc = M.Mpeg2Encoder(*params)
    try:
        enc.set_source_size(sw, sh, filter)
        assert M.fit_size(w, h) == (80, 45)
        assert resident(enc, x, w, h, 1, kind) == want
    finally:
        enc.close()
