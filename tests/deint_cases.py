"""Woven 4:2:0 clips for the deinterlacer (m2v_deinterlace_device) and what must come of them: shared by tests/test_deint_cases.py and
tests/test_gpu_deinterlace.py.  The expected frames come from the package's numpy statement of the definition (deinterlace_frames) and
from literals; nothing here looks at what the library computes - except host(), which is the library's own arithmetic
(csrc/m2v_deint_kernels.hpp) compiled for the CPU with g++ and walked tile by tile as k_deint walks (tools/deint_host.hpp).

cases() is a seeded greedy covering array over size x frames x layout x mode x rate x order in which every legal pair of levels occurs
("blend" with rate "field" is the one illegal pair)."""
import ctypes
import functools
import itertools
import os
import random
import subprocess
import tempfile

import numpy as np

import m2v_load

M = m2v_load.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
LAYOUTS = ("i420", "yv12", "nv12", "nv21")
MODES = ("line", "adaptive", "blend")
RATES = ("frame", "field")
ORDERS = ("tff", "bff")
NFRAMES = (1, 2, 3, 5)
SMALL_SIZES = [(1, 2), (2, 3), (1, 5), (17, 5), (35, 9), (16, 16), (48, 32)]
TILE = (256, 8)           # m2v_deinterlace_tile, as csrc/m2v_deint_kernels.hpp has it: tests/test_deint_cases.py holds the library to it


def tile_sizes(tile=TILE):
    C, R = tile
    return [(w, h) for w in (C - 1, C, C + 1, 2 * C + 3) for h in (R - 1, R, R + 1, 2 * R + 1)]


def sizes():
    return SMALL_SIZES + tile_sizes()


def legal(c):
    return not (c["mode"] == "blend" and c["rate"] == "field")


def factors():
    return [("size", sizes()), ("nframes", list(NFRAMES)), ("layout", list(LAYOUTS)), ("mode", list(MODES)), ("rate", list(RATES)), ("order", list(ORDERS))]


def pairs_of(c, fs):
    lv = [(i, levels.index(c[name])) for i, (name, levels) in enumerate(fs)]
    return set(itertools.combinations(lv, 2))


@functools.lru_cache(maxsize=None)
def _covering(seed=20271, tries=40):
    fs = factors()
    rng = random.Random(seed)
    want = set()
    for (i, (ni, li)), (j, (nj, lj)) in itertools.combinations(enumerate(fs), 2):
        for a in range(len(li)):
            for b in range(len(lj)):
                if {ni: li[a], nj: lj[b]} != {"mode": "blend", "rate": "field"}:        # (the one illegal pair: every other pair has a legal row)
                    want.add(((i, a), (j, b)))
    left, rows = set(want), []
    while left:
        best, gain = None, -1
        seedpair = sorted(left)[rng.randrange(len(left))]
        for _ in range(tries):
            c = {name: levels[rng.randrange(len(levels))] for name, levels in fs}
            for i, a in seedpair:
                c[fs[i][0]] = fs[i][1][a]
            if not legal(c):
                continue
            g = len(pairs_of(c, fs) & left)
            if g > gain:
                best, gain = c, g
        assert best is not None and gain > 0
        rows.append(best)
        left -= pairs_of(best, fs)
    return tuple(tuple(sorted(r.items())) for r in rows), frozenset(want)


def cases():
    """the rows of the covering array, each a dict: size (w, h), nframes, layout, mode, rate, order"""
    return [dict(r) for r in _covering()[0]]


def all_pairs():
    return set(_covering()[1])


def name_of(c):
    return "%dx%d-n%d-%s-%s-%s-%s" % (c["size"][0], c["size"][1], c["nframes"], c["layout"], c["mode"], c["rate"], c["order"])


def clip(w, h, n, layout, seed):
    """n woven frames [n, frame_bytes]: a still picture under every frame; a quarter of every frame's samples nudged by a few levels, a
    quarter random - so the clamp of "adaptive" is open, shut and in between, on both of its sides"""
    rng = np.random.default_rng(seed)
    fb = M.frame_bytes(w, h, layout)
    base = rng.integers(0, 256, fb, dtype=np.int64)
    out = np.empty((n, fb), np.uint8)
    for k in range(n):
        kind = rng.integers(0, 4, fb)
        nudged = np.clip(base + rng.integers(-9, 10, fb), 0, 255)
        out[k] = np.where(kind < 2, base, np.where(kind == 2, nudged, rng.integers(0, 256, fb))).astype(np.uint8)
    return out


def source(c):
    w, h = c["size"]
    return clip(w, h, c["nframes"], c["layout"], seed=1000 + 31 * w + 7 * h + c["nframes"])


def expected(c, x=None):
    w, h = c["size"]
    return M.deinterlace_frames(source(c) if x is None else x, w, h, c["layout"], c["mode"], c["rate"], c["order"])


def column(rows, layout="i420"):
    """frames of width 1 whose luma column is `rows` (a list per frame), chroma 128 -> [n, frame_bytes]"""
    h = len(rows[0])
    fb = M.frame_bytes(1, h, layout)
    out = np.full((len(rows), fb), 128, np.uint8)
    out[:, :h] = np.asarray(rows, np.uint8)
    return out


# the literals of the header's definition: (frames' luma columns, mode, rate, order, the outputs' luma columns)
RAMP = [0, 2, 4, 6, 8, 10, 12, 14]
THREE = [[10, 100, 30, 0], [20, 60, 40, 0], [50, 80, 20, 0]]
LITERALS = [
    ([RAMP], "line", "frame", "tff", [[0, 2, 4, 6, 8, 10, 12, 12]]),
    ([RAMP], "line", "frame", "bff", [[2, 2, 4, 6, 8, 10, 12, 14]]),
    ([RAMP], "blend", "frame", "tff", [[1, 2, 4, 6, 8, 10, 12, 14]]),
    (THREE, "adaptive", "frame", "tff", [[10, 90, 30, 10], [20, 55, 40, 20], [50, 45, 20, 20]]),
    (THREE, "adaptive", "field", "tff", [[10, 90, 30, 10], [55, 100, 50, 0], [20, 55, 40, 20], [60, 60, 30, 0], [50, 45, 20, 20], [70, 80, 30, 0]]),
]


# ---- the library's arithmetic on the CPU ----
_HARNESS = r"""
#include "deint_host.hpp"
extern "C" int deint_host_run(const uint8_t *src, unsigned long long nframes, int w, int h, int layout, int mode, int rate, int order, uint8_t *dst,
                              unsigned long long cap, unsigned max_blocks)
{
    return deint_host::run(src, nframes, w, h, layout, mode, rate, order, dst, cap, max_blocks);
}
extern "C" int deint_host_check(unsigned long long src, unsigned long long nframes, int w, int h, int layout, int mode, int rate, int order,
                                unsigned long long dst, unsigned long long cap)
{
    return m2v::deint::check_args(src, nframes, w, h, layout, mode, rate, order, dst, cap, nullptr);
}
extern "C" unsigned long long deint_host_bound(int w, int h, unsigned long long nframes, int rate) { return m2v::deint::bound(w, h, nframes, rate); }
extern "C" void deint_host_tile(int *c, int *r) { *c = m2v::deint::kTileCols; *r = m2v::deint::kTileRows; }
"""
_host = {}


def host_lib():
    """the harness above over tools/deint_host.hpp and csrc/m2v_deint_kernels.hpp, compiled with g++ (no HIP)"""
    if "lib" not in _host:
        d = tempfile.mkdtemp(prefix="m2v_deint_host_")
        src, so = os.path.join(d, "deint_host.cpp"), os.path.join(d, "libdeint_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        ci, ull, vp = ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p
        L.deint_host_run.argtypes = [vp, ull, ci, ci, ci, ci, ci, ci, vp, ull, ctypes.c_uint]
        L.deint_host_check.argtypes = [ull, ull, ci, ci, ci, ci, ci, ci, ull, ull]
        L.deint_host_bound.restype = ull
        L.deint_host_bound.argtypes = [ci, ci, ull, ci]
        L.deint_host_tile.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci)]
        _host["lib"] = L
    return _host["lib"]


def host(x, w, h, layout="i420", mode="adaptive", rate="frame", order="tff", max_blocks=0):
    """the frames [n or 2 n, frame_bytes] the library's arithmetic makes of the woven frames x, on max_blocks blocks at most (0: the
    kernel's cap).  A guard of 0xA5 lies around the output: the walk may not touch it."""
    fb = M.frame_bytes(w, h, layout)
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, fb)
    n = len(x)
    nout = n * (2 if rate == "field" else 1)
    guard = 64
    buf = np.full(nout * fb + 2 * guard, 0xA5, np.uint8)
    r = host_lib().deint_host_run(x.ctypes.data, n, w, h, M.LAYOUTS_420[layout], M.DEINT_MODES[mode], M.DEINT_RATES[rate], M.DEINT_ORDERS[order],
                                  buf[guard:].ctypes.data, nout * fb, max_blocks)
    assert r == 0, (r, w, h, layout, mode, rate, order)
    assert (buf[:guard] == 0xA5).all() and (buf[guard + nout * fb:] == 0xA5).all()
    return buf[guard:guard + nout * fb].reshape(nout, fb).copy()


def pack_cases(items):
    """the file tools/deint_host_check.cpp reads: items of (case, frames, blocks at most)"""
    out = []
    for c, x, blocks in items:
        w, h = c["size"]
        out.append(np.asarray([w, h, len(x), M.LAYOUTS_420[c["layout"]], M.DEINT_MODES[c["mode"]], M.DEINT_RATES[c["rate"]], M.DEINT_ORDERS[c["order"]], blocks],
                              np.int32).tobytes())
        out.append(np.ascontiguousarray(x, np.uint8).tobytes())
    return b"".join(out)
