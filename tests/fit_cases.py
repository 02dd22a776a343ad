"""Source frames of any size in every input format, and the planes / the stream the encoder must make of them: shared by
tests/test_input_fit.py and tests/test_gpu_input_fit.py.  Everything here goes through the package's numpy statements of the
definitions (pad_frames, to444, rgb_to444) and the oracle; nothing here looks at what the library computes."""
import functools

import numpy as np

import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()
KINDS_420 = ("i420", "yv12", "nv12", "nv21")
KINDS_RGB = ("rgb24", "bgr24", "rgbx", "bgrx", "xrgb", "xbgr", "rgbp")
KINDS = ("444",) + KINDS_420 + KINDS_RGB
_RGB = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgbx": (4, (0, 1, 2)), "bgrx": (4, (2, 1, 0)), "xrgb": (4, (1, 2, 3)), "xbgr": (4, (3, 2, 1))}


def padded(w, h):
    return 16 * ((w + 15) // 16), 16 * ((h + 15) // 16)


@functools.lru_cache(maxsize=None)
def _base(w, h, n, seed, noise):
    """three w x h planes per frame [n, 3, h, w]: a synthetic clip cropped, or white noise"""
    if noise:
        a = np.random.default_rng(seed).integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    else:
        W, H = padded(w, h)
        a = np.ascontiguousarray(M.synth.clip(W, H, n, clip_index=seed, scene_len=4)[:, :, :h, :w])
    a.setflags(write=False)
    return a


def source(w, h, n, kind, seed=0, noise=False, base=None):
    """n source frames of w x h in `kind`, [n, frame bytes] uint8: the three planes of _base (or of `base` [n, 3, h, w]) as Y, U, V
    (chroma: every second sample of every second row) or as R, G, B; the ignored byte of the 32-bit layouts is noise"""
    p = _base(w, h, n, seed, noise) if base is None else base
    assert p.shape == (n, 3, h, w)
    if kind in ("444", "rgbp"):
        return np.ascontiguousarray(p).reshape(n, -1)
    if kind in KINDS_420:
        y, a, b = p[:, 0].reshape(n, -1), p[:, 1, ::2, ::2].reshape(n, -1), p[:, 2, ::2, ::2].reshape(n, -1)
        if kind in ("yv12", "nv21"):
            a, b = b, a
        c = np.concatenate([a, b], axis=1) if kind in ("i420", "yv12") else np.stack([a, b], axis=2).reshape(n, -1)
        return np.ascontiguousarray(np.concatenate([y, c], axis=1))
    bpp, where = _RGB[kind]
    px = np.random.default_rng(seed + 977).integers(0, 256, (n, h, w, bpp), dtype=np.uint8)
    for c in range(3):
        px[..., where[c]] = p[:, c]
    return px.reshape(n, -1)


def planes(x, w, h, kind, matrix="bt601"):
    """the planar 4:4:4 frames [n, 3, H, W] the encoder is to make of the w x h frames x of `kind`, by the definitions"""
    W, H = padded(w, h)
    p = M.pad_frames(x, w, h, kind)
    if kind == "444":
        return p.reshape(-1, 3, H, W)
    if kind in KINDS_420:
        return M.to444(p, W, H, kind)
    return M.rgb_to444(p, W, H, kind, matrix)


def want_stream(x, w, h, kind, pf, params, matrix="bt601"):
    """the oracle's stream for those frames"""
    W, H = padded(w, h)
    return orc.encode(planes(x, w, h, kind, matrix), W // 16, H // 16, pf, *params)
