"""-m gpu: RGB input (seven layouts, four matrices) through every entry point that takes it, byte for byte against the oracle's stream
for the planar 4:4:4 frames of the integer transform (M.rgb_to444; tests/test_input_rgb.py pins that definition).  Exact everywhere:
there is no tolerance in this file.

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
LAYOUTS = ("rgb24", "bgr24", "rgbx", "bgrx", "xrgb", "xbgr", "rgbp")
MATRICES = ("bt601", "bt709", "bt601f", "bt709f")
PATHS = ("pageable", "pinned0", "pinned1", "pinned2", "pull", "resident", "begin_end")
WHERE = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgbx": (4, (0, 1, 2)), "bgrx": (4, (2, 1, 0)), "xrgb": (4, (1, 2, 3)),
         "xbgr": (4, (3, 2, 1))}
KNOWN = {                       # (R, G, B) -> (Y, U, V) in the order of MATRICES; pure red and pure blue clamp in the full-range ones
    (0, 0, 0): ((16, 128, 128), (16, 128, 128), (0, 128, 128), (0, 128, 128)),
    (255, 255, 255): ((235, 128, 128), (235, 128, 128), (255, 128, 128), (255, 128, 128)),
    (128, 128, 128): ((126, 128, 128), (126, 128, 128), (128, 128, 128), (128, 128, 128)),
    (255, 0, 0): ((81, 90, 240), (63, 102, 240), (76, 85, 255), (54, 99, 255)),
    (0, 255, 0): ((145, 54, 34), (173, 42, 26), (150, 44, 21), (182, 30, 12)),
    (0, 0, 255): ((41, 240, 110), (32, 240, 118), (29, 255, 107), (18, 255, 116)),
}


@pytest.fixture(scope="module")
def env():
    import m2v_load
    from oracle import m2v_oracle_ctypes as orc
    return m2v_load.load(), orc


def pictures(M, W, H, n, ci, noise=False):
    """n RGB pictures [n, H, W, 3]: a synthetic clip (its three planes taken as R, G, B), or white noise"""
    if noise:
        return np.random.default_rng(ci).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return np.ascontiguousarray(M.synth.clip(W, H, n, clip_index=ci, scene_len=4).transpose(0, 2, 3, 1))


def pack(pic, layout, seed=0):
    """pictures [n, H, W, 3] -> frames [n, W*H*bpp] in `layout`, the ignored byte of the 32-bit layouts filled with noise"""
    n, H, W, _ = pic.shape
    if layout == "rgbp":
        return np.ascontiguousarray(pic.transpose(0, 3, 1, 2)).reshape(n, -1)
    bpp, where = WHERE[layout]
    px = np.random.default_rng(seed).integers(0, 256, (n, H, W, bpp), dtype=np.uint8)
    for c in range(3):
        px[..., where[c]] = pic[..., c]
    return px.reshape(n, -1)


def clip_rgb(M, W, H, n, layout, ci, noise=False):
    return pack(pictures(M, W, H, n, ci, noise), layout, ci)


def pin(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def drain(enc):
    enc.sequence_stop()
    return enc.pull_all()


def port_encode(M, enc, x, xs, ys, pf, layout, matrix, path, split=None):
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
            m, last = enc.push_rgb_pull(xs, ys, pf, src[k:k + step], out, pos, layout, matrix)
            pos += m
            assert not last
        enc.sequence_stop()
        while not last:
            m, last = enc.pull_into(out, pos)
            pos += m
        return out[:pos].tobytes()
    for k in range(0, n, step):
        enc.push_rgb(xs, ys, pf, src[k:k + step], layout, matrix)
    if path == "pinned2":
        enc.upload_wait()
    return drain(enc)


def resident_encode_rgb(M, enc, x, xs, ys, pf, layout, matrix):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    d_out = torch.empty(x.size * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    nb = enc.encode_resident_rgb(d_in.data_ptr(), x.shape[0], d_out.data_ptr(), d_out.numel(), xs, ys, pf, layout, matrix)
    return d_out[:nb].cpu().numpy().tobytes()


def encode_rgb(M, x, xs, ys, pf, layout, matrix, path, XL=7, YL=7, VL=3, Q=2, batch_frames=None, split=None, options=()):
    enc = M.Mpeg2Encoder(XL, YL, VL, Q)
    try:
        if batch_frames:
            enc.set_option("batch_frames", batch_frames)
        for k, v in options:
            enc.set_option(k, v)
        if path == "resident":
            return resident_encode_rgb(M, enc, x, xs, ys, pf, layout, matrix)
        return port_encode(M, enc, x, xs, ys, pf, layout, matrix, path, split)
    finally:
        enc.close()


# ---- 1: each layout x each path, the matrices rotating (every layout meets all four) ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout_and_path(env, layout, path):
    import torch
    M, orc = env
    W, H, n, pf = 160, 128, 5, 4
    matrix = MATRICES[(LAYOUTS.index(layout) + PATHS.index(path)) % 4]
    x = clip_rgb(M, W, H, n, layout, 600)
    want = orc.encode(M.rgb_to444(x, W, H, layout, matrix), W // 16, H // 16, pf, 7, 7, 3, 2)
    if path != "begin_end":
        assert encode_rgb(M, x, W // 16, H // 16, pf, layout, matrix, path) == want
        return
    # two handles taking turns, two sequences each in flight after the other's _begin
    y = clip_rgb(M, W, H, n, layout, 601)
    want_y = orc.encode(M.rgb_to444(y, W, H, layout, matrix), W // 16, H // 16, pf, 7, 7, 3, 2)
    encs = [M.Mpeg2Encoder(7, 7, 3, 2), M.Mpeg2Encoder(7, 7, 3, 2)]
    try:
        d_in = [torch.from_numpy(a).to("cuda:0") for a in (x, y)]
        d_out = [torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        got = []
        encs[0].encode_resident_rgb_begin(d_in[0].data_ptr(), n, d_out[0].data_ptr(), d_out[0].numel(), W // 16, H // 16, pf, layout, matrix)
        for turn in range(1, 5):
            k = turn & 1
            encs[k].encode_resident_rgb_begin(d_in[k].data_ptr(), n, d_out[k].data_ptr(), d_out[k].numel(), W // 16, H // 16, pf, layout, matrix)
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


# ---- 2: geometry ----
@pytest.mark.parametrize("W,H,n,pf,XL,YL", [
    (64, 64, 4, 3, 7, 7),
    (80, 112, 4, 3, 7, 7),             # odd xsize16
    (1200, 80, 3, 2, 7, 7),            # xsize16 = 75
    (1440, 704, 3, 2, 7, 6),           # c1's largest geometry
    (640, 480, 3, 0, 7, 7),            # c2: I frames only
    (1920, 1152, 9, 8, 7, 7),          # c3: the first GOP
])
def test_geometries(env, W, H, n, pf, XL, YL):
    M, orc = env
    pic = pictures(M, W, H, n, 610, noise=W * H <= 80 * 112)             # one clip, handed in in several layouts
    wants = {}
    for layout, matrix, path in (("rgb24", "bt601", "pinned1"), ("bgrx", "bt601", "resident"), ("rgbp", "bt601", "resident"),
                                 ("xrgb", "bt709", "pageable"), ("bgr24", "bt709", "resident"), ("rgbx", "bt601", "pinned2")):
        if matrix not in wants:
            wants[matrix] = orc.encode(M.rgb_to444(pack(pic, "rgb24"), W, H, "rgb24", matrix), W // 16, H // 16, pf, XL, YL, 3, 2)
        assert encode_rgb(M, pack(pic, layout), W // 16, H // 16, pf, layout, matrix, path, XL, YL) == wants[matrix], (layout, matrix, path)


def test_size_above_the_clamp_and_pframes_extremes(env):
    M, orc = env
    enc = M.Mpeg2Encoder(4, 4, 1, 2)                        # at most 256 x 256
    try:
        assert enc.geometry(20, 2) == (256, 64)
        for pf, layout, matrix in ((255, "rgb24", "bt601f"), (0, "xbgr", "bt709"), (255, "rgbp", "bt709f"), (0, "bgr24", "bt601")):
            x = clip_rgb(M, 256, 64, 4, layout, 620 + pf)  # the frames are supplied in the clamped geometry
            want = orc.encode(M.rgb_to444(x, 256, 64, layout, matrix), 20, 2, pf, 4, 4, 1, 2)
            assert enc.encode(x, 20, 2, pf, layout=layout, matrix=matrix) == want, (pf, layout)
            assert resident_encode_rgb(M, enc, x, 20, 2, pf, layout, matrix) == want, (pf, layout, "resident")
    finally:
        enc.close()


# ---- 3: port semantics ----
@pytest.mark.parametrize("batch", [1, 4, 96])
def test_splits_that_line_up_with_nothing(env, batch):
    M, orc = env
    W, H, n, pf = 128, 96, 13, 4
    for layout, matrix, path, split in (("rgb24", "bt601", "pageable", 3), ("bgrx", "bt709", "pinned1", 7), ("rgbp", "bt601f", "pinned2", 2),
                                        ("xrgb", "bt709f", "pull", 5), ("bgr24", "bt601", "pinned0", 1)):
        x = clip_rgb(M, W, H, n, layout, 630)
        want = orc.encode(M.rgb_to444(x, W, H, layout, matrix), W // 16, H // 16, pf, 7, 7, 3, 2)
        assert encode_rgb(M, x, W // 16, H // 16, pf, layout, matrix, path, batch_frames=batch, split=split) == want, (layout, path, split)
        if batch != 96:
            assert encode_rgb(M, x, W // 16, H // 16, pf, layout, matrix, "resident", batch_frames=batch) == want, (layout, "resident")


@pytest.mark.parametrize("batch,page_locked", [(1, False), (4, True), (96, False), (96, True), (5, True)])
def test_rgb_444_packed_and_420_frames_alternate_in_one_sequence(env, batch, page_locked):
    M, orc = env
    W, H, pf = 96, 64, 5
    # (kind, matrix): neighbours 2 / 3 and 9 / 10 differ in the matrix only, 3 / 4 in the layout only; a 4 B/px frame arrives in a
    # chunk whose packed bytes were sized for 3 B/px (frames 0 -> 4) and for 1.5 B/px (5 -> 6)
    kinds = [("rgb24", "bt601"), ("444", None), ("rgb24", "bt601"), ("rgb24", "bt709"), ("bgrx", "bt709"), ("i420", None), ("xrgb", "bt601f"),
             ("yuv24", None), ("rgbp", "bt709f"), ("rgbp", "bt709f"), ("rgbp", "bt601"), ("nv12", None), ("ayuv32", None), ("bgr24", "bt601f"),
             ("444", None), ("xbgr", "bt601")]
    n = len(kinds)
    pic = pictures(M, W, H, n, 640)
    yuv = M.to444(M.to420(M.synth.clip(W, H, n, clip_index=641, scene_len=4), "i420"), W, H, "i420")     # for the frames that arrive as YUV
    clip = np.empty((n, 3, H, W), np.uint8)
    sends = []
    for f, (kind, matrix) in enumerate(kinds):
        if kind in LAYOUTS:
            x = pack(pic[f:f + 1], kind, f)
            clip[f] = M.rgb_to444(x, W, H, kind, matrix)[0]
            sends.append(x)
        else:
            clip[f] = yuv[f]
            sends.append(None)
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, 3, 2)
    hold = pin if page_locked else np.ascontiguousarray
    enc = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        enc.set_option("batch_frames", batch)
        for f, (kind, matrix) in enumerate(kinds):
            fr = clip[f:f + 1]
            if kind in LAYOUTS:
                enc.push_rgb(W // 16, H // 16, pf, hold(sends[f]), kind, matrix)
            elif kind == "444":
                enc.push_frames(W // 16, H // 16, pf, hold(fr))
            elif kind in M.LAYOUTS_420:
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
        # three sequences back to back on one handle, another layout, matrix and size each
        for k, (W, H, n, layout, matrix) in enumerate([(288, 208, 4, "bgrx", "bt709"), (640, 320, 3, "rgb24", "bt601"), (160, 704, 3, "rgbp", "bt601f")]):
            x = clip_rgb(M, W, H, n, layout, 650 + k)
            want = orc.encode(M.rgb_to444(x, W, H, layout, matrix), W // 16, H // 16, 23, 7, 6, 3, 2)
            assert not enc.busy
            assert enc.encode(x, W // 16, H // 16, 23, layout=layout, matrix=matrix) == want, "sequence %d" % k
            assert not enc.busy
        W, H, pf = 96, 64, 2
        x = clip_rgb(M, W, H, 4, "bgr24", 660)
        x444 = M.rgb_to444(x, W, H, "bgr24", "bt709")
        # stop on a frame boundary; frames pushed after the stop and before `last` is pulled are dropped, with their pframes_count
        enc.push_rgb(6, 4, pf, x[:2], "bgr24", "bt709")
        enc.sequence_stop()
        enc.push_rgb(6, 4, 7, x[2:3], "bgr24", "bt709")
        buf = np.zeros(1 << 16, np.uint8)
        m, last = enc.push_rgb_pull(6, 4, pf, x[3:4], buf, 0, "bgr24", "bt709")        # dropped as well; its pull half hands the stream out
        got = buf[:m].tobytes()
        while not last:
            m, last = enc.pull_into(buf, 0)
            got += buf[:m].tobytes()
        assert got == orc.encode(x444[:2], 6, 4, pf, 7, 6, 3, 2) and not enc.busy
        # M2V_E_PARAM: unknown layouts and matrices, a NULL pointer with frames; nothing starts
        for bad in (7, -1, 17):
            assert L.m2v_push_rgb(enc._h, 6, 4, pf, x.ctypes.data, 1, bad, 0) == -1
            assert b"layout" in L.m2v_last_error(enc._h)
            assert L.m2v_push_rgb_pull(enc._h, 6, 4, pf, x.ctypes.data, 1, bad, 0, buf.ctypes.data, buf.size, None) == -1
            assert b"layout" in L.m2v_last_error(enc._h)
            assert L.m2v_encode_resident_rgb(enc._h, 6, 4, pf, 256, 1, bad, 0, 256, 256, None, None) == -1
            assert b"layout" in L.m2v_last_error(enc._h)
            assert L.m2v_encode_resident_rgb_begin(enc._h, 6, 4, pf, 256, 1, bad, 0, 256, 256, None) == -1
        for bad in (4, -1, 9):
            assert L.m2v_push_rgb(enc._h, 6, 4, pf, x.ctypes.data, 1, 1, bad) == -1
            assert b"matrix" in L.m2v_last_error(enc._h)
            assert L.m2v_push_rgb_pull(enc._h, 6, 4, pf, x.ctypes.data, 1, 1, bad, buf.ctypes.data, buf.size, None) == -1
            assert b"matrix" in L.m2v_last_error(enc._h)
            assert L.m2v_encode_resident_rgb(enc._h, 6, 4, pf, 256, 1, 1, bad, 256, 256, None, None) == -1
            assert b"matrix" in L.m2v_last_error(enc._h)
            assert L.m2v_encode_resident_rgb_begin(enc._h, 6, 4, pf, 256, 1, 1, bad, 256, 256, None) == -1
        assert L.m2v_push_rgb(enc._h, 6, 4, pf, None, 1, 0, 0) == -1
        assert L.m2v_push_rgb(enc._h, 6, 4, pf, None, 0, 0, 0) == 0
        assert L.m2v_encode_resident_rgb(enc._h, 6, 4, pf, None, 1, 0, 0, 256, 256, None, None) == -1
        assert not enc.busy
        # M2V_E_STATE after a partial m2v_push_beats frame; the frame can still be completed by beats
        y, u, v = (x444[0, c].reshape(-1) for c in range(3))
        enc.push_beats(6, 4, pf, y[:400], u[:400], v[:400])
        assert L.m2v_push_rgb(enc._h, 6, 4, pf, x.ctypes.data, 1, 1, 1) == -4
        assert b"partially filled" in L.m2v_last_error(enc._h)
        enc.push_beats(6, 4, pf, y[400:], u[400:], v[400:])
        enc.push_rgb(6, 4, pf, x[1:], "bgr24", "bt709")
        assert drain(enc) == orc.encode(x444, 6, 4, pf, 7, 6, 3, 2)
        # M2V_E_STATE while a resident sequence is in flight, and for the resident entries while the port is busy
        d_in = torch.from_numpy(x).to("cuda:0")
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        enc.encode_resident_rgb_begin(d_in.data_ptr(), 4, d_out.data_ptr(), d_out.numel(), 6, 4, pf, "bgr24", "bt709")
        assert L.m2v_push_rgb(enc._h, 6, 4, pf, x.ctypes.data, 1, 1, 1) == -4
        assert L.m2v_encode_resident_rgb_begin(enc._h, 6, 4, pf, d_in.data_ptr(), 4, 1, 1, d_out.data_ptr(), d_out.numel(), None) == -4
        nb = enc.encode_resident_end()
        assert d_out[:nb].cpu().numpy().tobytes() == orc.encode(x444, 6, 4, pf, 7, 6, 3, 2)
        enc.push_rgb(6, 4, pf, x[:1], "bgr24", "bt709")
        n = ctypes.c_size_t(0)
        assert L.m2v_encode_resident_rgb(enc._h, 6, 4, pf, d_in.data_ptr(), 4, 1, 1, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == -4
        # a device pointer that is not 16-byte aligned is refused by the library's own check
        enc.reset()
        assert L.m2v_encode_resident_rgb(enc._h, 6, 4, pf, d_in.data_ptr() + 8, 1, 1, 1, d_out.data_ptr(), d_out.numel(), ctypes.byref(n), None) == -1
        assert b"16-byte aligned" in L.m2v_last_error(enc._h)
        assert L.m2v_encode_resident_rgb_begin(enc._h, 6, 4, pf, d_in.data_ptr() + 4, 1, 1, 1, d_out.data_ptr(), d_out.numel(), None) == -1
        # m2v_reset in mid-sequence (frames buffered and a chunk submitted), then a clean encode
        enc.set_option("batch_frames", 2)
        enc.push_rgb(6, 4, pf, x[:3], "bgr24", "bt709")
        assert enc.busy
        enc.reset()
        assert not enc.busy and enc.pull() == (b"", False)
        assert enc.encode(x, 6, 4, pf, layout="bgr24", matrix="bt709") == orc.encode(x444, 6, 4, pf, 7, 6, 3, 2)
    finally:
        enc.close()


# ---- 4: stage level ----
@pytest.mark.parametrize("W,H", [(80, 112), (160, 128)])
def test_converted_input_is_rgb_to444(env, W, H):
    """m2v_debug_read(4): what k_rgb2yuv left for the chunk's kernels, from the shipped library - the kernel's arithmetic on its own.
    Noise frames, each layout x each matrix, and a frame that holds the known answers (pure red and pure blue among them: the two
    pixels whose chroma clamps in the full-range matrices)."""
    M, orc = env
    n = 3
    enc = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        assert M.lib().m2v_debug_read(enc._h, 4, np.zeros(16, np.uint8).ctypes.data, 16) == -4       # no such call yet
        pic = pictures(M, W, H, n, 670, noise=True)
        for k, rgb in enumerate(KNOWN):
            pic[1, 0, k] = rgb                         # the corner cases, at the start of a row ...
            pic[1, H - 1, W - 1 - k] = rgb             # ... and at the very end of the frame
            pic[2, 5, 16 * (k % (W // 16)) + 15] = rgb
        for layout in LAYOUTS:
            x = pack(pic, layout, 671)
            for mi, matrix in enumerate(MATRICES):
                resident_encode_rgb(M, enc, x, W // 16, H // 16, 2, layout, matrix)
                got = enc.debug_read(4, n * 3 * W * H, np.uint8).reshape(n, 3, H, W)
                assert np.array_equal(got, M.rgb_to444(x, W, H, layout, matrix)), (layout, matrix)
                for k, rgb in enumerate(KNOWN):
                    assert tuple(got[1, :, 0, k]) == KNOWN[rgb][mi], (layout, matrix, rgb)
                    assert tuple(got[1, :, H - 1, W - 1 - k]) == KNOWN[rgb][mi], (layout, matrix, rgb)
        # the last chunk of a sequence in chunks of 2 frames: its third frame alone
        enc.set_option("batch_frames", 2)
        resident_encode_rgb(M, enc, x, W // 16, H // 16, 0, "rgbp", "bt709")
        got = enc.debug_read(4, n * 3 * W * H, np.uint8)
        assert got.size == 3 * W * H and np.array_equal(got.reshape(1, 3, H, W), M.rgb_to444(x[2:], W, H, "rgbp", "bt709"))
    finally:
        enc.close()


@pytest.mark.parametrize("layout,matrix", [("bgrx", "bt709")])
def test_stages_of_an_rgb_encode_equal_the_oracles(env, layout, matrix):
    """the comparison tests/gpu_util.py::compare_stages makes for 4:4:4, for an RGB encode on the debug library"""
    import gpu_util as G
    M, orc = env
    W, H, n, pf = 160, 128, 5, 4
    x = clip_rgb(M, W, H, n, layout, 680)
    ref_bytes, ref = orc.encode(M.rgb_to444(x, W, H, layout, matrix), W // 16, H // 16, pf, 7, 7, 3, 2, dump=True)
    mbs = (W // 16) * (H // 16)
    enc = M.Mpeg2Encoder(7, 7, 3, 2, debug=True)
    try:
        enc.set_option("keep_recon", 1)
        assert resident_encode_rgb(M, enc, x, W // 16, H // 16, pf, layout, matrix) == ref_bytes
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


# ---- 5: module parameters ----
def test_vector_and_q_levels_and_conformant(env):
    M, orc = env
    W, H, n, pf = 160, 128, 4, 3
    k = 0
    for VL in (1, 2, 3):
        for Q in (1, 2, 3, 4):
            layout, matrix = LAYOUTS[k % 7], MATRICES[k % 4]
            k += 1
            x = clip_rgb(M, W, H, n, layout, 690 + k)
            want = orc.encode(M.rgb_to444(x, W, H, layout, matrix), W // 16, H // 16, pf, 7, 7, VL, Q)
            assert encode_rgb(M, x, W // 16, H // 16, pf, layout, matrix, "resident", VL=VL, Q=Q) == want, (VL, Q, layout, matrix)
    x = clip_rgb(M, W, H, n, "bgrx", 699)
    want = orc.encode(M.rgb_to444(x, W, H, "bgrx", "bt709"), W // 16, H // 16, pf, 7, 7, 3, 2, conformant=True)
    assert encode_rgb(M, x, W // 16, H // 16, pf, "bgrx", "bt709", "resident", options=(("conformant", 1),)) == want
    assert encode_rgb(M, x, W // 16, H // 16, pf, "bgrx", "bt709", "pinned1", options=(("conformant", 1),)) == want


# ---- 6: fuzz ----
def test_fuzz_60_cases(env):
    """size, pframes_count, layout, matrix, path, split, batch_frames, VECTOR_LEVEL, Q_LEVEL; every case drawn is run.
    Time bound for the file's fuzz: 10 minutes (the oracle on the CPU is most of it)."""
    M, orc = env
    rng = np.random.default_rng(888)
    t0 = time.monotonic()
    for case in range(60):
        W, H = 16 * int(rng.integers(4, 17)), 16 * int(rng.integers(4, 13))
        VL, Q = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        pf = int(rng.choice([0, 1, 2, 3, 5, 8, 255]))
        n = int(rng.integers(1, 8))
        bf = int(rng.choice([1, 2, 3, 96]))
        layout = LAYOUTS[int(rng.integers(0, 7))]
        matrix = MATRICES[int(rng.integers(0, 4))]
        path = PATHS[int(rng.integers(0, 6))]                          # (begin_end has its own test)
        split = int(rng.integers(1, n + 1))
        x = clip_rgb(M, W, H, n, layout, 7000 + case, noise=bool(rng.integers(0, 2)))
        want = orc.encode(M.rgb_to444(x, W, H, layout, matrix), W // 16, H // 16, pf, 7, 7, VL, Q)
        got = encode_rgb(M, x, W // 16, H // 16, pf, layout, matrix, path, VL=VL, Q=Q, batch_frames=bf, split=split)
        assert got == want, "case %d: %dx%d n=%d pf=%d VL=%d Q=%d batch=%d %s %s %s split=%d" % (case, W, H, n, pf, VL, Q, bf, layout, matrix,
                                                                                             path, split)
    assert time.monotonic() - t0 < 600


# ---- 7: m2v_tb ----
def test_tb_bgrx_bt709_files(env, tmp_path):
    M, orc = env
    M.build()
    C = importlib.import_module(M.__name__ + ".container")
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    vids = [(288, 208, 3), (160, 96, 26)]                               # the second one crosses a GOP boundary (pframes 23)
    args, wants = [], []
    for k, (W, H, n) in enumerate(vids):
        x = clip_rgb(M, W, H, n, "bgrx", 700 + k)
        fin = tmp_path / ("v%d.bgra" % k)
        fin.write_bytes(x.tobytes() + b"\x55" * 1000)                   # a trailing partial frame is ignored (TB:220)
        args += [str(fin), str(W), str(H), str(tmp_path / ("v%d.m2v" % k))]
        wants.append(orc.encode(M.rgb_to444(x, W, H, "bgrx", "bt709"), W // 16, H // 16, 23, 7, 6, 3, 2))
    r = subprocess.run([tb, "-bgrx", "-matrix", "bt709", "-ps"] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("end of video") == 2
    for k, (W, H, n) in enumerate(vids):
        es = (tmp_path / ("v%d.m2v" % k)).read_bytes()
        assert es == wants[k], "video %d" % k
        info, pics = C.scan(es)
        assert len(pics) == n
        assert (tmp_path / ("v%d.m2v.mpg" % k)).read_bytes() == C.mux_ps(es)
    r = subprocess.run([tb, "-bgrx", "-nv12"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage:" in r.stderr


# ---- 8: the torch entry ----
def test_encode_tensor(env):
    import torch
    M, orc = env
    W, H, n, pf = 160, 128, 5, 4
    pic = pictures(M, W, H, n, 710)
    want = {m: orc.encode(M.rgb_to444(pack(pic, "rgb24"), W, H, "rgb24", m), W // 16, H // 16, pf, 7, 7, 3, 2) for m in ("bt601", "bt709f")}
    enc = M.Mpeg2Encoder(7, 7, 3, 2)
    try:
        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        hwc = dev(pic)
        got = enc.encode_tensor(hwc, pf)
        assert got.is_cuda and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want["bt601"]
        assert enc.encode_tensor(dev(pic[..., ::-1]), pf, order="bgr", matrix="bt709f").cpu().numpy().tobytes() == want["bt709f"]
        assert enc.encode_tensor(dev(pic.transpose(0, 3, 1, 2)), pf).cpu().numpy().tobytes() == want["bt601"]          # [N, 3, H, W]
        for order in ("rgbx", "bgrx", "xrgb", "xbgr"):
            t = dev(pack(pic, order, 5).reshape(n, H, W, 4))
            assert enc.encode_tensor(t, pf, order=order, matrix="bt709f").cpu().numpy().tobytes() == want["bt709f"], order
        # out=: the result is a view of it; too small is the library's overflow
        out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        got = enc.encode_tensor(hwc, pf, out=out)
        assert got.data_ptr() == out.data_ptr() and got.cpu().numpy().tobytes() == want["bt601"]
        with pytest.raises(M.M2VError):
            enc.encode_tensor(hwc, pf, out=torch.empty(64, dtype=torch.uint8, device="cuda:0"))
        assert enc.encode_tensor(hwc, pf).cpu().numpy().tobytes() == want["bt601"]                                       # the handle is usable afterwards
        # what is not such a tensor
        for bad in (hwc.permute(0, 3, 1, 2),                          # not contiguous
                    hwc[:, :, ::2],
                    hwc.cpu(),
                    torch.zeros((1, 17, 64, 3), dtype=torch.uint8, device="cuda:0"),
                    torch.zeros((1, 64, 72, 3), dtype=torch.uint8, device="cuda:0"),
                    torch.zeros((1, 4096, 64, 3), dtype=torch.uint8, device="cuda:0"),       # beyond the handle's clamp
                    hwc.float(), hwc[0], pic):
            with pytest.raises(ValueError):
                enc.encode_tensor(bad, pf)
        with pytest.raises(ValueError):
            enc.encode_tensor(hwc, pf, order="rgbx")                   # three channels, an order of four
        with pytest.raises(ValueError):
            enc.encode_tensor(hwc, pf, matrix="nosuch")
        # on a stream of the caller's: the frames are produced on it, the encode follows them there
        s = torch.cuda.Stream()
        host = torch.from_numpy(np.ascontiguousarray(pic[..., ::-1])).pin_memory()
        with torch.cuda.stream(s):
            t = host.to("cuda:0", non_blocking=True).flip(-1).contiguous()
            got = enc.encode_tensor(t, pf)
            data = got.cpu().numpy().tobytes()
        s.synchronize()
        assert data == want["bt601"]
    finally:
        enc.close()
