"""Source frames of another size (m2v_set_source_size) in every input format, and the planes / the stream the encoder must make of them:
shared by tests/test_input_scale.py and tests/test_gpu_scale.py, built on tests/fit_cases.py.  Everything here goes through the
package's numpy statements of the definitions (scale_frames, pad_frames, to444, rgb_to444) and the oracle; nothing here looks at what the
library computes - except host(), which is the library's own arithmetic (csrc/m2v_scale_kernels.hpp) compiled for the CPU with g++ and
walked tile by tile as k_scale walks, with or without one textual fault."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import fit_cases as F

M = F.M
FILTERS = ("triangle", "area")
PASS_KINDS = ("444", "i420", "nv12", "rgb24", "bgrx", "rgbp")
# (source size, picture size) of the pass alone: exactly 2 : 1 with odd chroma on both sides; no integer ratio; exactly 8 : 1 (16 taps,
# taps past both edges); enlarging, twice; identity in one dimension only
PASS_FIRST = [((142, 98), (71, 49)), ((97, 131), (71, 55)), ((568, 392), (71, 49)), ((36, 25), (71, 49)), ((9, 7), (72, 56)), ((71, 131), (71, 55))]
# ... and every count of padded columns and rows, every place of the last column and row in a tile
PASS_SIZES = PASS_FIRST + [((131, 77), (w, 49)) for w in range(65, 81)] + [((100, 121), (72, h)) for h in range(49, 65)]
# src and dst of the tap tables: the issue's sources, against 46 destinations
TAP_SRC = list(range(1, 140)) + [1080, 1920, 4096, 15360]
TAP_DST = list(range(1, 41)) + [49, 64, 71, 135, 360, 720]


def scaled(x, sw, sh, w, h, kind, filter="triangle"):
    """the w x h frames of `kind` the sw x sh frames x become, by the definition"""
    return M.scale_frames(x, sw, sh, w, h, kind, filter)


def planes(x, sw, sh, w, h, kind, filter="triangle", matrix="bt601"):
    """the planar 4:4:4 frames [n, 3, H, W] the encoder is to make of the sw x sh frames x of `kind` at picture size w x h"""
    return F.planes(scaled(x, sw, sh, w, h, kind, filter), w, h, kind, matrix)


# ---- the library's arithmetic on the CPU ----
_HARNESS = r"""
#include "m2v_scale_kernels.hpp"
#include <algorithm>
#include <vector>
using namespace m2v::scale;
// one frame at src (64 spare bytes behind it) -> the padded frame at dst, as k_scale walks: plane by plane, tile by tile, the horizontal
// pass over the tile's source rows into the tile's 16-bit rows, the vertical pass out of them.  A row of zeros lies in front of and
// behind the tile's rows, so that a span cut short reads zeros and nothing else.
extern "C" int scale_host(int filter, int form, int es, int sw, int sh, int w, int h, int W, int H, const uint8_t *src, uint8_t *dst)
{
    const int dims[4][2] = {{sw, w}, {sh, h}, {chroma(sw), chroma(w)}, {chroma(sh), chroma(h)}};
    std::vector<Taps> tabs((size_t)w + h + chroma(w) + chroma(h));
    Taps *t = tabs.data();
    for (auto &d : dims)
        for (int x = 0; x < d[1]; ++x)
            if (build_taps(filter, d[0], d[1], x, *t++) < 1) return -1;
    const Run run = make_run(form, es, sw, sh, w, h, W, H);
    std::vector<uint16_t> tile((kMaxSpan + 2) * kTileCols);
    uint16_t *tt = tile.data() + kTileCols;
    for (uint32_t k = 0; k < run.nplanes; ++k) {
        const Plane &p = run.p[k];
        const uint32_t srow = p.scols * p.es, drow = p.COLS * p.es;
        const Taps *ht = tabs.data() + p.htab, *vt = tabs.data() + p.vtab;
        for (uint32_t y0 = 0; y0 < p.ROWS; y0 += kTileRows)
            for (uint32_t xb0 = 0; xb0 < drow; xb0 += kTileCols) {
                int rlo, rhi;
                tile_span(vt, y0, p.h, p.srows, rlo, rhi);
                if (rhi < rlo || rhi - rlo >= kMaxSpan) return -2;
                std::fill(tile.begin(), tile.end(), (uint16_t)0);
                for (uint32_t col = 0; col < (uint32_t)kTileCols && xb0 + col < drow; ++col) {
                    uint32_t xo, b;
                    column(xb0 + col, p.es, p.w, xo, b);
                    for (int r = rlo; r <= rhi; ++r) tt[(r - rlo) * kTileCols + col] = (uint16_t)hpass(src + p.soff + (uint32_t)r * srow, p.es, b, ht[xo], p.scols);
                    for (uint32_t ry = 0; ry < (uint32_t)kTileRows; ++ry)
                        dst[p.doff + (y0 + ry) * drow + xb0 + col] = (uint8_t)vpass(tt + col, kTileCols, rlo, vt[row_of(y0 + ry, p.h)], p.srows);
                }
            }
    }
    return 0;
}
extern "C" int taps_host(int filter, int src, int dst, int x, int *first, uint16_t *c)
{
    Taps t{};
    const int n = build_taps(filter, src, dst, x, t);
    if (n > 0) { *first = t.first; for (int k = 0; k < kMaxTaps; ++k) c[k] = t.c[k]; }
    return n;
}
"""

# one fault each, as (text of csrc/m2v_scale_kernels.hpp, what stands there instead): every text occurs exactly once
FAULTS = {
    "rounding constant 127 for 128": ("uint32_t acc = 128u;", "uint32_t acc = 127u;"),
    "clamp to src for src - 1": ("(int)scols - 1) * es + b]", "(int)scols) * es + b]"),
    "remainder on the first tap": ("t.c[best] = (uint16_t)(t.c[best] + ", "t.c[0] = (uint16_t)(t.c[0] + "),
    "< for <= in the triangle's support": ("hi = floordiv(P + R - 1, D);\n        for (long long i = lo; i <= hi; ++i) {",
                                            "hi = floordiv(P + R - 1, D);\n        for (long long i = lo; i < hi; ++i) {"),
    "chroma sw / 2 for (sw + 1) / 2": ("scw = chroma(sw)", "scw = (uint32_t)sw / 2"),
    "span one short at the top": ("rlo = clampi(a.first, ", "rlo = clampi(a.first + 1, "),
    "span one short at the bottom": ("rhi = clampi(b.first + (int)b.n - 1, ", "rhi = clampi(b.first + (int)b.n - 2, "),
}
_host = {}


def host_lib(fault=None):
    """the harness above and csrc/m2v_scale_kernels.hpp (with one of FAULTS in it, if named), compiled with g++ (no HIP)"""
    if fault not in _host:
        d = tempfile.mkdtemp(prefix="m2v_scale_host_")
        csrc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        with open(os.path.join(csrc, "m2v_scale_kernels.hpp")) as f:
            hpp = f.read()
        if fault is not None:
            old, new = FAULTS[fault]
            assert hpp.count(old) == 1, "the text of fault %r occurs %d times in m2v_scale_kernels.hpp" % (fault, hpp.count(old))
            hpp = hpp.replace(old, new)
        src, so = os.path.join(d, "scale_host.cpp"), os.path.join(d, "libscale_host.so")
        with open(os.path.join(d, "m2v_scale_kernels.hpp"), "w") as f:
            f.write(hpp)
        with open(src, "w") as f:
            f.write(_HARNESS)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", d, "-o", so, src])
        L = ctypes.CDLL(so)
        L.scale_host.argtypes = [ctypes.c_int] * 9 + [ctypes.c_void_p, ctypes.c_void_p]
        L.taps_host.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint16)]
        _host[fault] = L
    return _host[fault]


def _form(kind):
    """(form, bytes of a packed pixel) of m2v_scale_kernels.hpp's make_run"""
    if kind in ("444", "rgbp"):
        return 0, 1
    if kind in ("i420", "yv12"):
        return 1, 1
    if kind in ("nv12", "nv21"):
        return 2, 1
    return 3, M.rgb_bytes_per_pixel(kind)


def host(x, sw, sh, w, h, kind, filter="triangle", fault=None):
    """the padded W x H frames [n, bytes] of `kind` that the library's arithmetic makes of the sw x sh frames x (with a fault: or None,
    where the faulty arithmetic refuses the sizes)"""
    W, H = F.padded(w, h)
    L = host_lib(fault)
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, M.frame_bytes(sw, sh, kind))
    out = np.zeros((len(x), M.frame_bytes(W, H, kind)), np.uint8)
    form, es = _form(kind)
    for k in range(len(x)):
        src = np.concatenate([x[k], np.zeros(64, np.uint8)])
        r = L.scale_host(M.SCALE_FILTERS[filter], form, es, sw, sh, w, h, W, H, src.ctypes.data, out[k].ctypes.data)
        if r != 0 and fault is not None:
            return None                                 # (the fault leaves a sample without taps, or a tile with too many rows)
        assert r == 0, (r, sw, sh, w, h, kind, filter)
    return out
