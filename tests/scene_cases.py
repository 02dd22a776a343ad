"""Where GOPs start (m2v_set_gop_starts, option "scene_cut"): what the encoder must produce - shared by tests/test_scene_cases.py,
tests/test_gpu_gop_starts.py and tests/test_gpu_scene_cut.py.  GOPs are closed, an I picture resets temporal_reference and the GOP
header's time code is a function of the frame number alone, so the stream of a sequence whose GOPs are [s, s + L) is a splice of the
oracle's streams of the frames of each GOP encoded alone: the sequence header, then for every GOP the bytes of GOP 0 of that stream
with the four bytes behind the group_start_code replaced by the time code of frame s, then the end code and the final-word padding.
Everything here comes from the oracle and from numpy; nothing looks at what the library computes."""
import numpy as np

import gop_cases as G

M = G.M
FIRST, CADENCE, LIST, CUT = 1, 2, 4, 8


def time_code(n):
    """the four bytes behind 00 00 01 B8 for a GOP that starts at frame n (put_gop_header: 24 frames/s, hours saturate at 63,
    closed_gop = 1, broken_link = 0 and five zero bits)"""
    pic, sec, mnt, hour = n % 24, (n // 24) % 60, (n // 1440) % 60, min(n // 86400, 63)
    v = (hour << 26) | (mnt << 20) | (1 << 19) | (sec << 13) | (pic << 7) | (2 << 5)
    return v.to_bytes(4, "big")


def layout(nframes, pf, starts, cuts=()):
    """the rule, frame by frame -> [flags]: frame n starts a GOP iff flags[n] != 0"""
    pf &= 0xFF
    starts, cuts = set(starts or ()), set(cuts)
    flags, s = [], 0
    for n in range(nframes):
        fl = 0
        if n == 0:
            fl |= FIRST
        elif n - s == pf + 1:
            fl |= CADENCE
        if n in starts:
            fl |= LIST
        if n in cuts:
            fl |= CUT
        if fl:
            s = n
        flags.append(fl)
    return flags


def gops(nframes, pf, starts, cuts=()):
    """[(s, L)] of every GOP"""
    at = [n for n, fl in enumerate(layout(nframes, pf, starts, cuts)) if fl] + [nframes]
    return [(a, b - a) for a, b in zip(at, at[1:])]


def expected(frames, W, H, pf, gop_starts, levels=None, cuts=(), Q=2, **params):
    """the stream of the frames with GOPs per layout(len(frames), pf, gop_starts, cuts); levels: a schedule by GOP ordinal (else
    every GOP at Q); params: VL, conformant"""
    gs = gops(len(frames), pf, gop_starts, cuts)
    lv = G.per_gop(levels, len(gs)) if levels else [Q] * len(gs)
    body = None
    for (s, L), q in zip(gs, lv):
        head, g = G.cut(G.encoded(frames[s:s + L], W, H, pf, q, **params)[0])
        assert len(g) == 1 and g[0][:4] == G.GOP_CODE
        if body is None:
            body = head
        body += g[0][:4] + time_code(s) + g[0][8:]
    return G.finish(body)


def records(nframes, pf, starts, cuts=(), diffs=None):
    """what m2v_scene_report must hand out: (n, flags, D(n) or 0)"""
    r = np.zeros(nframes, M.SCENE_STAT_DTYPE)
    r["frame"] = np.arange(nframes)
    r["flags"] = layout(nframes, pf, starts, cuts)
    if diffs is not None:
        r["diff"] = diffs
    return r


def mb_sums(frames):
    """[n, 3, H, W] planar 4:4:4 (H, W whole macroblocks) -> [n, mbh, mbw] int64: the luma sum of every macroblock"""
    y = np.asarray(frames)[:, 0].astype(np.int64)
    n, H, W = y.shape
    return y.reshape(n, H // 16, 16, W // 16, 16).sum(axis=(2, 4))


def diffs(frames):
    """[n] int64: D(0) = 0, D(n) = the sum over the macroblocks of |S_n - S_(n-1)|"""
    s = mb_sums(frames)
    d = np.zeros(len(s), np.int64)
    d[1:] = np.abs(s[1:] - s[:-1]).sum(axis=(1, 2))
    return d


def cuts_of(frames, T):
    """the frames the detector flags at threshold T: D(n) > T * mbs"""
    s = mb_sums(frames)
    return [int(n) for n in np.nonzero(diffs(frames) > T * s.shape[1] * s.shape[2])[0]]
