"""Frames of any size, the part that needs no GPU: the arithmetic (fit_size / m2v_fit_size, frame_bytes), the numpy statement of the
definition (pad_frames) that is the GPU tests' reference, the header rewrite (set_header_size) and the decoder's reading of header
sizes that are not whole macroblocks.

The module takes whole macroblocks only.  The definition (include/m2v_mi355x.h): the stream of a w x h frame is the stream of the frame
padded to W x H = 16 ceil(w / 16) x 16 ceil(h / 16) in its own format, every plane extended by its last column and its last row.

On the order of padding and chroma expansion: 4:2:0 chroma is padded in the 4:2:0 domain, before the 2 x 2 repeat.  Repeating the last
sample commutes with repeating every sample twice, so padding the 2 x 2-repeated source instead gives the SAME planes, for even and
for odd sizes alike (for odd ones the repeated source is cropped to w x h first); test_pad_420_domain holds both cases to equality.
No stream can tell the two orders apart - the statement fixes which planes are padded (cw x ch of them), not a different result."""
import ctypes

import numpy as np

import fit_cases as F
import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()


def test_fit_size():
    L = M.lib()
    for w in range(49, 131):
        for h in range(49, 131):
            xs, ys = ctypes.c_uint32(0), ctypes.c_uint32(0)
            assert L.m2v_fit_size(w, h, ctypes.byref(xs), ctypes.byref(ys)) == 0
            assert (xs.value, ys.value) == M.fit_size(w, h) == (-(-w // 16), -(-h // 16)), (w, h)
    assert L.m2v_fit_size(0, 55, None, None) < 0 and L.m2v_fit_size(71, -1, None, None) < 0
    assert M.fit_size(1920, 1080) == (120, 68) and M.fit_size(1910, 1080) == (120, 68) and M.fit_size(64, 64) == (4, 4)
    assert "m2v_set_frame_size" in M.EXPORTS and "m2v_fit_size" in M.EXPORTS


def test_frame_bytes():
    for w, h in ((71, 55), (72, 56), (65, 49), (80, 64), (1920, 1080), (1919, 1079)):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        assert M.frame_bytes(w, h, "444") == 3 * w * h
        for k in F.KINDS_420:
            assert M.frame_bytes(w, h, k) == w * h + 2 * cw * ch, (w, h, k)
        for k in F.KINDS_RGB:
            assert M.frame_bytes(w, h, k) == w * h * (4 if k in ("rgbx", "bgrx", "xrgb", "xbgr") else 3), (w, h, k)
        for k in F.KINDS:
            assert F.source(w, h, 1, k, noise=True).shape == (1, M.frame_bytes(w, h, k))


def _plane_list(w, h, kind):
    """(element bytes, columns, rows, padded columns, padded rows) of every plane of a frame, from the table of the definition"""
    W, H = F.padded(w, h)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if kind in ("444", "rgbp"):
        return [(1, w, h, W, H)] * 3
    if kind in ("i420", "yv12"):
        return [(1, w, h, W, H), (1, cw, ch, W // 2, H // 2), (1, cw, ch, W // 2, H // 2)]
    if kind in ("nv12", "nv21"):
        return [(1, w, h, W, H), (2, cw, ch, W // 2, H // 2)]
    return [(4 if kind in ("rgbx", "bgrx", "xrgb", "xbgr") else 3, w, h, W, H)]


def test_pad_frames():
    for k in F.KINDS:                                   # whole macroblocks: nothing to do
        x = F.source(80, 64, 2, k, noise=True)
        assert np.array_equal(M.pad_frames(x, 80, 64, k), x), k
    w, h, n = 71, 55, 2
    for k in F.KINDS:
        x = F.source(w, h, n, k, seed=3, noise=True)
        p = M.pad_frames(x, w, h, k)
        assert p.dtype == np.uint8 and p.shape == (n, sum(es * C * R for es, _, _, C, R in _plane_list(w, h, k))), k
        sa = da = 0
        for es, c, r, C, R in _plane_list(w, h, k):
            s = x[:, sa:sa + es * c * r].reshape(n, r, c, es)
            d = p[:, da:da + es * C * R].reshape(n, R, C, es)
            sa, da = sa + es * c * r, da + es * C * R
            assert np.array_equal(d[:, :r, :c], s), k                                                  # the source in the top-left
            assert np.array_equal(d[:, :r, c:], np.broadcast_to(s[:, :, c - 1:c], (n, r, C - c, es))), k   # its last column to the right
            assert np.array_equal(d[:, r:], np.broadcast_to(d[:, r - 1:r], (n, R - r, C, es))), k      # the last (padded) row below
        assert sa == x.shape[1] and da == p.shape[1]


def test_pad_420_domain():
    """padding the cw x ch chroma planes and then repeating 2 x 2 == repeating 2 x 2 (cropped to w x h) and then padding: the two
    commute, for even and for odd sizes (see the module's docstring)"""
    for w, h in ((70, 54), (71, 55), (66, 49), (65, 50)):
        W, H = F.padded(w, h)
        cw, ch = (w + 1) // 2, (h + 1) // 2
        x = F.source(w, h, 2, "i420", seed=5, noise=True)
        a = M.to444(M.pad_frames(x, w, h, "i420"), W, H, "i420")
        y = x[:, :w * h].reshape(2, 1, h, w)
        c = x[:, w * h:].reshape(2, 2, ch, cw).repeat(2, axis=2).repeat(2, axis=3)[:, :, :h, :w]
        b = M.pad_frames(np.concatenate([y, c], axis=1), w, h, "444").reshape(2, 3, H, W)
        assert np.array_equal(a, b), (w, h)
        assert np.array_equal(a, F.planes(x, w, h, "i420"))


def test_set_header_size():
    W, H, n, pf = 80, 64, 3, 2
    clip = M.synth.clip(W, H, n, clip_index=11, scene_len=4)
    es = orc.encode(clip, W // 16, H // 16, pf, 6, 6, 3, 2)
    ts = M.set_header_size(es, 71, 55)
    assert isinstance(ts, bytes) and len(ts) == len(es)
    diff = [i for i in range(len(es)) if es[i] != ts[i]]
    assert diff and set(diff) <= {4, 5, 6, 30, 31, 32, 33}, diff
    assert int.from_bytes(ts[4:7], "big") == (71 << 12) | 55
    assert int.from_bytes(ts[30:34], "big") >> 3 == (71 << 15) | (1 << 14) | 55
    assert M.set_header_size(ts, W, H) == es
    assert M.set_header_size(es, W, H) == es
    full, crop = M.decoder.decode(es), M.decoder.decode(ts)
    assert (full.width, full.height) == (W, H) and (crop.width, crop.height) == (71, 55)
    assert len(full.frames) == len(crop.frames) == n
    for a, b in zip(full.frames, crop.frames):
        assert a[0].shape == (H, W) and b[0].shape == (55, 71) and b[1].shape == b[2].shape == (28, 36)
        assert np.array_equal(b[0], a[0][:55, :71]) and np.array_equal(b[1], a[1][:28, :36]) and np.array_equal(b[2], a[2][:28, :36])
    assert crop.mbs == full.mbs
