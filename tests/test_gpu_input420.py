"""-m gpu: 4:2:0 input (I420, YV12, NV12, NV21) through every entry point that takes it, byte for byte against the oracle's stream
for the 4:4:4 frames whose chroma planes are the 4:2:0 planes repeated 2 x 2 (M.to444; tests/test_input420.py pins that definition).

Error paths use the library's own checks only."""
import ctypes
import importlib
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("i420", "yv12", "nv12", "nv21")
PATHS = ("pageable", "pinned0", "pinned1", "pinned2", "pull", "resident", "begin_end")


@pytest.fixture(scope="module")
def env():
    import m2v_load
    from oracle import m2v_oracle_ctypes as orc
    return m2v_load.load(), orc


def clip420(M, W, H, n, layout, ci, noise=False):
    """n 4:2:0 frames [n, W*H*3/2] in `layout`: a synthetic clip through the module's own down-conversion, or white noise"""
    if noise:
        return np.random.default_rng(ci).integers(0, 256, (n, W * H * 3 // 2), dtype=np.uint8)
    return M.to420(M.synth.clip(W, H, n, clip_index=ci, scene_len=4), layout)


def pin(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def drain(enc):
    enc.sequence_stop()
    return enc.pull_all()


def port_encode(M, enc, x, xs, ys, pf, layout, path, split=None):
    """one sequence of the frames x through a port path of `enc`, `split` frames per call (None: all at once)"""
    n = x.shape[0]
    step = split or n
    if path == "pageable":
        src = x
    else:
        src = pin(x)
        enc.set_option("direct_upload", {"pinned0": 0, "pinned1": 1, "pinned2": 2, "pull": 1}[path])
    if path == "pull":
        out = np.zeros(n * x.shape[1] * 2 + (1 << 16), np.uint8)
        pos, last = 0, False
        for k in range(0, n, step):
            m, last = enc.push_frames420_pull(xs, ys, pf, src[k:k + step], out, pos, layout)
            pos += m
            assert not last
        enc.sequence_stop()
        while not last:
            m, last = enc.pull_into(out, pos)
            pos += m
        return out[:pos].tobytes()
    for k in range(0, n, step):
        enc.push_frames420(xs, ys, pf, src[k:k + step], layout)
    if path == "pinned2":
        enc.upload_wait()
    return drain(enc)


def resident_encode420(M, enc, x, xs, ys, pf, layout):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    d_out = torch.empty(x.size * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    nb = enc.encode_resident420(d_in.data_ptr(), x.shape[0], d_out.data_ptr(), d_out.numel(), xs, ys, pf, layout)
    return d_out[:nb].cpu().numpy().tobytes()


def encode420(M, x, xs, ys, pf, layout, path, XL=7, YL=7, VL=3, Q=2, batch_frames=None, split=None, options=()):
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)
    try:
        if batch_frames:
            enc.set_option("batch_frames", batch_frames)
        for k, v in options:
            enc.set_option(k, v)
        if path == "resident":
            return resident_encode420(M, enc, x, xs, ys, pf, layout)
        return port_encode(M, enc, x, xs, ys, pf, layout, path, split)
    finally:
        enc.close()


# ---- 4: each layout x each path ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout_and_path(env, layout, path):
    import torch
    M, orc = env
    W, H, n, pf = 160, 128, 5, 4
    x = clip420(M, W, H, n, layout, 400)
    want = orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, pf, 7, 7, 3, 2)
    if path != "begin_end":
        assert encode420(M, x, W // 16, H // 16, pf, layout, path) == want
        return
    # two handles taking turns, two sequences each in flight after the other's _begin
    y = clip420(M, W, H, n, layout, 401)
    want_y = orc.encode(M.to444(y, W, H, layout), W // 16, H // 16, pf, 7, 7, 3, 2)
    encs = [M.Mpeg2Encoder(7, 7, 3, 2), M.Mpeg2Encoder(7, 7, 3, 2)]
    try:
        d_in = [torch.from_numpy(a).to("cuda:0") for a in (x, y)]
        d_out = [torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        got = []
        encs[0].encode_resident420_begin(d_in[0].data_ptr(), n, d_out[0].data_ptr(), d_out[0].numel(), W // 16, H // 16, pf, layout)
        for turn in range(1, 5):
            k = turn & 1
            encs[k].encode_resident420_begin(d_in[k].data_ptr(), n, d_out[k].data_ptr(), d_out[k].numel(), W // 16, H // 16, pf, layout)
            nb = encs[k ^ 1].encode_resident_end()
            got.append((k ^ 1, d_out[k ^ 1][:nb].cpu().numpy().tobytes()))
        nb = encs[0].encode_resident_end()
        got.append((0, d_out[0][:nb].cpu().numpy().tobytes()))
        assert len(got) == 5
        for k, data in got:
            assert data == (want, want_y)[k], "handle %d" % k
    finally:
        for e in encs:
            e.close()


# ---- 5: geometry ----
@pytest.mark.parametrize("W,H,n,pf,XL,YL", [
    (64, 64, 4, 3, 7, 7),
    (80, 112, 4, 3, 7, 7),             # odd xsize16: planar chroma rows start 8-byte aligned only
    (1200, 80, 3, 2, 7, 7),            # xsize16 = 75
    (1440, 704, 3, 2, 7, 6),           # c1's largest geometry
    (640, 480, 3, 0, 7, 7),            # c2: I frames only
    (1920, 1152, 9, 8, 7, 7),          # c3: the first GOP
])
def test_geometries(env, W, H, n, pf, XL, YL):
    M, orc = env
    pic = M.to444(clip420(M, W, H, n, "i420", 410, noise=W * H <= 80 * 112), W, H, "i420")       # one clip, handed in in every layout
    want = orc.encode(pic, W // 16, H // 16, pf, XL, YL, 3, 2)
    for layout, path in (("i420", "pinned1"), ("nv12", "resident"), ("yv12", "resident"), ("nv21", "pageable"), ("i420", "resident"),
                         ("nv12", "pinned2")):
        assert encode420(M, M.to420(pic, layout), W // 16, H // 16, pf, layout, path, XL, YL) == want, (layout, path)


def test_size_above_the_clamp_and_pframes_extremes(env):
    M, orc = env
    enc = M.Mpeg2Encoder(4, 4, 1, 2)                        # at most 256 x 256
    try:
        assert enc.geometry(20, 2) == (256, 64)
        for pf, layout in ((255, "i420"), (0, "nv12"), (255, "nv21"), (0, "yv12")):
            x = clip420(M, 256, 64, 4, layout, 420 + pf)   # the frames are supplied in the clamped geometry
            want = orc.encode(M.to444(x, 256, 64, layout), 20, 2, pf, 4, 4, 1, 2)
            assert enc.encode(x, 20, 2, pf, layout=layout) == want, (pf, layout)
            assert resident_encode420(M, enc, x, 20, 2, pf, layout) == want, (pf, layout, "resident")
    finally:
        enc.close()


# ---- 6: port semantics ----
@pytest.mark.parametrize("batch", [1, 4, 96])
def test_splits_that_line_up_with_nothing(env, batch):
    M, orc = env
    W, H, n, pf = 128, 96, 13, 4
    for layout, path, split in (("i420", "pageable", 3), ("nv12", "pinned1", 7), ("yv12", "pinned2", 2), ("nv21", "pull", 5), ("nv12", "pinned0", 1)):
        x = clip420(M, W, H, n, layout, 430)
        want = orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, pf, 7, 7, 3, 2)
        assert encode420(M, x, W // 16, H // 16, pf, layout, path, batch_frames=batch, split=split) == want, (layout, path, split)
        if batch != 96:
            assert encode420(M, x, W // 16, H // 16, pf, layout, "resident", batch_frames=batch) == want, (layout, "resident")


@pytest.mark.parametrize("batch,page_locked", [(1, False), (4, True), (96, False), (96, True), (5, True)])
def test_444_packed_and_420_frames_alternate_in_one_sequence(env, batch, page_locked):
    M, orc = env
    W, H, n, pf = 96, 64, 14, 5
    clip = M.to444(clip420(M, W, H, n, "i420", 440), W, H, "i420")            # the pictures, 4:4:4, chroma 2 x 2 constant
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, 3, 2)
    hold = pin if page_locked else np.ascontiguousarray
    enc = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        enc.set_option("batch_frames", batch)
        kinds = ["444", "i420", "yuv24", "nv12", "ayuv32", "yv12", "444", "nv21", "nv21", "uyv24", "i420", "i420", "444", "nv12"]
        for f, kind in enumerate(kinds):
            fr = clip[f:f + 1]
            if kind == "444":
                enc.push_frames(W // 16, H // 16, pf, hold(fr))
            elif kind in LAYOUTS:
                enc.push_frames420(W // 16, H // 16, pf, hold(M.to420(fr, kind)), kind)
            else:
                code, bpp = enc.PACKED[kind]
                px = np.zeros((H * W, bpp), np.uint8)
                order = {"yuv24": (0, 1, 2), "uyv24": (1, 0, 2), "yuvx32": (0, 1, 2), "ayuv32": (1, 2, 3)}[kind]
                for c in range(3):
                    px[:, order[c]] = fr[0, c].reshape(-1)
                enc.push_packed(W // 16, H // 16, pf, hold(px), kind)
        assert drain(enc) == want
    finally:
        enc.close()


def test_three_sequences_stop_drop_state_param_and_reset(env):
    import torch
    M, orc = env
    L = M.lib()
    enc = M.Mpeg2Encoder(7, 6, 3, 2)
    try:
        # three sequences back to back on one handle, another layout and size each
        for k, (W, H, n, layout) in enumerate([(288, 208, 4, "nv12"), (640, 320, 3, "i420"), (160, 704, 3, "nv21")]):
            x = clip420(M, W, H, n, layout, 450 + k)
            want = orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, 23, 7, 6, 3, 2)
            assert not enc.busy
            assert enc.encode(x, W // 16, H // 16, 23, layout=layout) == want, "sequence %d" % k
            assert not enc.busy
        W, H, pf = 96, 64, 2
        x = clip420(M, W, H, 4, "yv12", 460)
        x444 = M.to444(x, W, H, "yv12")
        # stop on a frame boundary; frames pushed after the stop and before `last` is pulled are dropped, with their pframes_count
        enc.push_frames420(6, 4, pf, x[:2], "yv12")
        enc.sequence_stop()
        enc.push_frames420(6, 4, 7, x[2:3], "yv12")
        buf = np.zeros(1 << 16, np.uint8)
        m, last = enc.push_frames420_pull(6, 4, pf, x[3:4], buf, 0, "yv12")        # dropped as well; its pull half hands the stream out
        got = buf[:m].tobytes()
        while not last:
            m, last = enc.pull_into(buf, 0)
            got += buf[:m].tobytes()
        assert got == orc.encode(x444[:2], 6, 4, pf, 7, 6, 3, 2) and not enc.busy
        # M2V_E_PARAM: unknown layouts, a NULL pointer with frames; nothing starts
        for bad in (4, -1, 17):
            assert L.m2v_push_frames420(enc._h, 6, 4, pf, x.ctypes.data, 1, bad) == -1
            assert b"layout" in L.m2v_last_error(enc._h)
            assert L.m2v_push_frames420_pull(enc._h, 6, 4, pf, x.ctypes.data, 1, bad, buf.ctypes.data, buf.size, None) == -1
            assert L.m2v_encode_resident420(enc._h, 6, 4, pf, 256, 1, bad, 256, 256, None, None) == -1
            assert L.m2v_encode_resident420_begin(enc._h, 6, 4, pf, 256, 1, bad, 256, 256, None) == -1
        assert L.m2v_push_frames420(enc._h, 6, 4, pf, None, 1, 0) == -1
        assert L.m2v_push_frames420(enc._h, 6, 4, pf, None, 0, 0) == 0
        assert not enc.busy
        # M2V_E_STATE after a partial m2v_push_beats frame; the frame can still be completed by beats
        y, u, v = (x444[0, c].reshape(-1) for c in range(3))
        enc.push_beats(6, 4, pf, y[:400], u[:400], v[:400])
        assert L.m2v_push_frames420(enc._h, 6, 4, pf, x.ctypes.data, 1, 1) == -4
        assert b"partially filled" in L.m2v_last_error(enc._h)
        enc.push_beats(6, 4, pf, y[400:], u[400:], v[400:])
        enc.push_frames420(6, 4, pf, x[1:], "yv12")
        assert drain(enc) == orc.encode(x444, 6, 4, pf, 7, 6, 3, 2)
        # M2V_E_STATE while a resident sequence is in flight, and for the resident entries while the port is busy
        d_in = torch.from_numpy(x).to("cuda:0")
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        enc.encode_resident420_begin(d_in.data_ptr(), 4, d_out.data_ptr(), d_out.numel(), 6, 4, pf, "yv12")
        assert L.m2v_push_frames420(enc._h, 6, 4, pf, x.ctypes.data, 1, 1) == -4
        assert L.m2v_encode_resident420_begin(enc._h, 6, 4, pf, d_in.data_ptr(), 4, 1, d_out.data_ptr(), d_out.numel(), None) == -4
        nb = enc.encode_resident_end()
        assert d_out[:nb].cpu().numpy().tobytes() == orc.encode(x444, 6, 4, pf, 7, 6, 3, 2)
        enc.push_frames420(6, 4, pf, x[:1], "yv12")
        n = ctypes.c_size_t(0)
        assert L.m2v_encode_resident420(enc._h, 6, 4, pf, d_in.data_ptr(), 4, 1, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == -4
        # a device pointer that is not 16-byte aligned is refused by the library's own check
        enc.reset()
        assert L.m2v_encode_resident420(enc._h, 6, 4, pf, d_in.data_ptr() + 8, 1, 1, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == -1
        # m2v_reset in mid-sequence (frames buffered and a chunk submitted), then a clean encode
        enc.set_option("batch_frames", 2)
        enc.push_frames420(6, 4, pf, x[:3], "yv12")
        assert enc.busy
        enc.reset()
        assert not enc.busy and enc.pull() == (b"", False)
        assert enc.encode(x, 6, 4, pf, layout="yv12") == orc.encode(x444, 6, 4, pf, 7, 6, 3, 2)
    finally:
        enc.close()


# ---- 7: stage level ----
@pytest.mark.parametrize("W,H", [(80, 112), (160, 128)])
def test_expanded_input_is_to444(env, W, H):
    """m2v_debug_read(4): what k_expand420 left for the chunk's kernels, from the shipped library"""
    M, orc = env
    n = 3
    enc = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        assert M.lib().m2v_debug_read(enc._h, 4, np.zeros(16, np.uint8).ctypes.data, 16) == -4       # no such call yet
        for layout in LAYOUTS:
            x = clip420(M, W, H, n, layout, 470, noise=True)
            resident_encode420(M, enc, x, W // 16, H // 16, 2, layout)
            got = enc.debug_read(4, n * 3 * W * H, np.uint8).reshape(n, 3, H, W)
            assert np.array_equal(got, M.to444(x, W, H, layout)), layout
        # the last chunk of a sequence in chunks of 2 frames: its third frame alone
        enc.set_option("batch_frames", 2)
        resident_encode420(M, enc, x, W // 16, H // 16, 0, "nv21")
        got = enc.debug_read(4, n * 3 * W * H, np.uint8)
        assert got.size == 3 * W * H and np.array_equal(got.reshape(1, 3, H, W), M.to444(x[2:], W, H, "nv21"))
    finally:
        enc.close()


@pytest.mark.parametrize("layout", ["i420", "nv21"])
def test_stages_of_a_420_encode_equal_the_oracles(env, layout):
    """the comparison tests/gpu_util.py::compare_stages makes for 4:4:4, for a 4:2:0 encode on the debug library"""
    import gpu_util as G
    M, orc = env
    W, H, n, pf = 160, 128, 5, 4
    x = clip420(M, W, H, n, layout, 480)
    ref_bytes, ref = orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, pf, 7, 7, 3, 2, dump=True)
    mbs = (W // 16) * (H // 16)
    enc = M.Mpeg2Encoder(7, 7, 3, 2, debug=True)
    try:
        enc.set_option("keep_recon", 1)
        assert resident_encode420(M, enc, x, W // 16, H // 16, pf, layout) == ref_bytes
        info = enc.debug_read(0, n * mbs * 4, np.uint32).reshape(n, mbs)
        coef = enc.debug_read(1, n * mbs * 768, np.int16).reshape(n, mbs, 6, 64)
        bits = enc.debug_read(2, n * mbs * 4, np.uint32).reshape(n, mbs).astype(np.int64)
        recon = enc.debug_read(3, n * (W * H * 3 // 2), np.uint8).reshape(n, -1)
    finally:
        enc.close()
    assert G.first_diff(ref["mb_inter"], (info & 1).astype(np.int8)) is None
    assert G.first_diff(ref["mb_cbp"], ((info >> 1) & 63).astype(np.uint8)) is None
    assert G.first_diff(ref["mb_mvx"], ((info >> 8) & 255).astype(np.uint8).view(np.int8)) is None
    assert G.first_diff(ref["mb_mvy"], ((info >> 16) & 255).astype(np.uint8).view(np.int8)) is None
    assert G.first_diff(ref["coef"], coef) is None
    bits.reshape(n, -1, W // 16)[:, :, 0] -= 38                       # the slice header on the first macroblock of a row
    assert G.first_diff(ref["mb_bits"], bits) is None
    for f in range(n):
        if (f % (pf + 1)) < pf and f != n - 1:                        # frames that are referenced later
            assert np.array_equal(ref["recon"][f], recon[f]), "recon of frame %d" % f


# ---- 8: module parameters ----
def test_vector_and_q_levels_and_conformant(env):
    M, orc = env
    W, H, n, pf = 160, 128, 4, 3
    k = 0
    for VL in (1, 2, 3):
        for Q in (1, 2, 3, 4):
            layout = LAYOUTS[k % 4]
            k += 1
            x = clip420(M, W, H, n, layout, 490 + k)
            want = orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, pf, 7, 7, VL, Q)
            assert encode420(M, x, W // 16, H // 16, pf, layout, "resident", VL=VL, Q=Q) == want, (VL, Q, layout)
    x = clip420(M, W, H, n, "nv12", 499)
    want = orc.encode(M.to444(x, W, H, "nv12"), W // 16, H // 16, pf, 7, 7, 3, 2, conformant=True)
    assert encode420(M, x, W // 16, H // 16, pf, "nv12", "resident", options=(("conformant", 1),)) == want
    assert encode420(M, x, W // 16, H // 16, pf, "nv12", "pinned1", options=(("conformant", 1),)) == want


# ---- 9: fuzz ----
def test_fuzz_60_cases(env):
    """size, pframes_count, layout, path, split, batch_frames, VECTOR_LEVEL, Q_LEVEL; every case drawn is run.
    Time bound for the file's fuzz: 10 minutes (the oracle on the CPU is most of it)."""
    M, orc = env
    rng = np.random.default_rng(420)
    t0 = time.monotonic()
    for case in range(60):
        W, H = 16 * int(rng.integers(4, 17)), 16 * int(rng.integers(4, 13))
        VL, Q = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        pf = int(rng.choice([0, 1, 2, 3, 5, 8, 255]))
        n = int(rng.integers(1, 8))
        bf = int(rng.choice([1, 2, 3, 96]))
        layout = LAYOUTS[int(rng.integers(0, 4))]
        path = PATHS[int(rng.integers(0, 6))]                          # (begin_end has its own test)
        split = int(rng.integers(1, n + 1))
        x = clip420(M, W, H, n, layout, 5000 + case, noise=bool(rng.integers(0, 2)))
        want = orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, pf, 7, 7, VL, Q)
        got = encode420(M, x, W // 16, H // 16, pf, layout, path, VL=VL, Q=Q, batch_frames=bf, split=split)
        assert got == want, "case %d: %dx%d n=%d pf=%d VL=%d Q=%d batch=%d %s %s split=%d" % (case, W, H, n, pf, VL, Q, bf, layout, path, split)
    assert time.monotonic() - t0 < 600


# ---- 10: m2v_tb ----
def test_tb_nv12_and_i420_files(env, tmp_path):
    M, orc = env
    M.build()
    C = importlib.import_module(M.__name__ + ".container")
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    vids = [(288, 208, 3), (160, 96, 26)]                               # the second one crosses a GOP boundary (pframes 23)
    for opt, layout in (("-nv12", "nv12"), ("-i420", "i420")):
        args, wants = [], []
        for k, (W, H, n) in enumerate(vids):
            x = clip420(M, W, H, n, layout, 500 + k)
            fin = tmp_path / ("%s%d.yuv" % (layout, k))
            fin.write_bytes(x.tobytes() + b"\x55" * 1000)               # a trailing partial frame is ignored (TB:220)
            args += [str(fin), str(W), str(H), str(tmp_path / ("%s%d.m2v" % (layout, k)))]
            wants.append(orc.encode(M.to444(x, W, H, layout), W // 16, H // 16, 23, 7, 6, 3, 2))
        r = subprocess.run([tb, opt, "-ps"] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("end of video") == 2
        for k, (W, H, n) in enumerate(vids):
            es = (tmp_path / ("%s%d.m2v" % (layout, k))).read_bytes()
            assert es == wants[k], "%s video %d" % (layout, k)
            info, pics = C.scan(es)
            assert len(pics) == n
            assert (tmp_path / ("%s%d.m2v.mpg" % (layout, k))).read_bytes() == C.mux_ps(es)
    r = subprocess.run([tb, "-nv12", "-yv12"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage:" in r.stderr


# ---- 11: one decode ----
def test_decoded_chroma_against_the_source_planes(env, capsys):
    M, orc = env
    W, H, n, pf = 96, 64, 4, 3
    x = clip420(M, W, H, n, "i420", 510)
    got = encode420(M, x, W // 16, H // 16, pf, "i420", "pinned1")
    via444 = encode420_444(M, M.to444(x, W, H, "i420"), W // 16, H // 16, pf)
    assert got == via444                                               # the two routes give ONE stream ...
    dec = M.decoder
    out, ref = dec.decode(got, quirks=True), dec.decode(via444, quirks=True)
    c = W * H // 4
    for f in range(n):
        src_u, src_v = x[f, W * H:W * H + c].reshape(H // 2, W // 2), x[f, W * H + c:].reshape(H // 2, W // 2)
        pu, pv = dec.psnr(out.frames[f][1], src_u), dec.psnr(out.frames[f][2], src_v)
        assert (pu, pv) == (dec.psnr(ref.frames[f][1], src_u), dec.psnr(ref.frames[f][2], src_v))     # ... hence one PSNR
        assert np.array_equal(out.frames[f][0], ref.frames[f][0])
        with capsys.disabled():
            print("frame %d: decoded chroma against the 4:2:0 source planes: U %.2f dB, V %.2f dB" % (f, pu, pv))


def encode420_444(M, clip, xs, ys, pf):
    enc = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        return enc.encode(clip, xs, ys, pf)
    finally:
        enc.close()
