"""CPU: the definition of m2v_set_source_size (include/m2v_mi355x.h) in its three statements - scale_taps / scale_frames (numpy, written
from the definition), m2v_scale_taps (the library's tables) and csrc/m2v_scale_kernels.hpp compiled with g++ and walked tile by tile as
the kernel walks - held against each other, and the properties the definition promises.  Every comparison is exact."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import scale_cases as S

M, F = S.M, S.F
E_PARAM = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_taps(L, filter, src, dst, x):
    first, co = ctypes.c_int(0), (ctypes.c_uint16 * M.SCALE_MAXTAPS)()
    n = L.m2v_scale_taps(filter, src, dst, x, ctypes.byref(first), co)
    return n, first.value, list(co)


@pytest.mark.parametrize("filter", [0, 1])
def test_tables_against_the_definition(filter):
    """m2v_scale_taps against scale_taps for every x of every legal (src, dst); sums of 2^14, tap counts within 16 and 9, the taps
    contiguous, first and last never moving backwards (what tile_span relies on)"""
    L = M.lib()
    most = 0
    pairs = [(s, d) for s in S.TAP_SRC for d in S.TAP_DST] + [(1920, 1280), (1080, 720), (1280, 1920), (540, 360)]
    for src, dst in pairs:
        if src > 8 * dst:
            assert L.m2v_scale_taps(filter, src, dst, 0, None, None) == E_PARAM
            with pytest.raises(ValueError):
                M.scale_taps(filter, src, dst, 0)
            continue
        last = (-10 ** 9, -10 ** 9)
        for x in range(dst):
            n, first, co = c_taps(L, filter, src, dst, x)
            want_first, c = M.scale_taps(filter, src, dst, x)
            assert (n, first, co) == (len(c), want_first, c + [0] * (M.SCALE_MAXTAPS - len(c))), (src, dst, x)
            assert sum(c) == 1 << 14 and min(c) >= 0
            assert first >= last[0] and first + n - 1 >= last[1]
            last = (first, first + n - 1)
            most = max(most, n)
    assert most <= (16 if filter == 0 else 9)
    assert most == (16 if filter == 0 else 9)          # (the lists reach the bound)


def test_tables_by_hand():
    for f in ("triangle", "area"):
        for n in (1, 7, 71, 1080):
            assert all(M.scale_taps(f, n, n, x) == (x, [1 << 14]) for x in range(n)), "equal sizes are the identity"
    # 2 : 4 gives 1/4, 3/4; 4 : 2 gives 1/8, 3/8, 3/8, 1/8
    assert M.scale_taps("triangle", 2, 4, 0) == (-1, [4096, 12288]) and M.scale_taps("triangle", 2, 4, 1) == (0, [12288, 4096])
    assert M.scale_taps("triangle", 2, 4, 3) == (1, [12288, 4096])
    assert M.scale_taps("triangle", 4, 2, 0) == (-1, [2048, 6144, 6144, 2048]) and M.scale_taps("triangle", 4, 2, 1) == (1, [2048, 6144, 6144, 2048])
    assert M.scale_taps("area", 4, 2, 1) == (2, [8192, 8192]) and M.scale_taps("area", 2, 4, 1) == (0, [16384])
    # 3 : 2 by area: 2/3, 1/3 - the remainder of 2^14 goes onto the larger weight
    assert M.scale_taps("area", 3, 2, 0) == (0, [10923, 5461]) and M.scale_taps("area", 3, 2, 1) == (1, [5461, 10923])
    # equal weights: the remainder goes onto the lowest index
    assert M.scale_taps("area", 3, 1, 0) == (0, [5462, 5461, 5461])


def test_errors_of_the_table_function():
    L = M.lib()
    co = (ctypes.c_uint16 * M.SCALE_MAXTAPS)()
    first = ctypes.c_int(0)
    for args in ((0, 9, 1, 0), (1, 17, 2, 0), (0, 0, 4, 0), (0, 4, 0, 0), (0, -3, 4, 0), (0, 4, -1, 0), (2, 4, 4, 0), (-1, 4, 4, 0), (0, 4, 4, 4), (0, 4, 4, -1),
                 (0, 16385, 4096, 0), (0, 4, 16385, 0)):
        assert L.m2v_scale_taps(*args, ctypes.byref(first), co) == E_PARAM, args
    assert L.m2v_scale_taps(0, 8, 1, 0, None, None) == 16 and L.m2v_scale_taps(1, 16384, 2048, 2047, None, None) == 8
    for bad in (("cubic", 4, 4, 0), (0, 9, 1, 0), (0, 0, 1, 0), (0, 4, 4, 4), (True, 4, 4, 0)):
        with pytest.raises(ValueError):
            M.scale_taps(*bad)


def test_flat_planes_and_shapes():
    """a flat plane keeps its value; planes of the right shape for every kind at odd sw, sh, w, h; equal sizes return the frames"""
    for kind in F.KINDS:
        for f in S.FILTERS:
            for (sw, sh), (w, h) in (((11, 7), (5, 9)), ((5, 9), (11, 7)), ((9, 9), (9, 5))):
                x = np.full((2, M.frame_bytes(sw, sh, kind)), 93, np.uint8)
                y = M.scale_frames(x, sw, sh, w, h, kind, f)
                assert y.shape == (2, M.frame_bytes(w, h, kind)) and y.dtype == np.uint8 and (y == 93).all(), (kind, f)
        x = F.source(13, 11, 2, kind, seed=3, noise=True)
        assert np.array_equal(M.scale_frames(x, 13, 11, 13, 11, kind), x)
    with pytest.raises(ValueError):
        M.scale_frames(np.zeros((1, 27), np.uint8), 3, 3, 5, 5, "444", "cubic")


def test_bound_against_exact_fractions():
    """scale_frames against the same taps a(i) / A in exact fractions, on random planes: the deviation stays under the derived 1.45
    (0.467 per pass of coefficient error, 1 / 128 and 1 / 2 of rounding).  Measured maximum over these 14 planes: 0.5000 (an exact tie, rounded up)."""
    rng = np.random.default_rng(11)

    def weights(f, src, dst, x):
        if f == "triangle":
            P, R = (2 * x + 1) * src - dst, 2 * max(src, dst)
            a = {i: R - abs(2 * dst * i - P) for i in range(-20, src + 20)}
        else:
            a = {i: min((i + 1) * dst, (x + 1) * src) - max(i * dst, x * src) for i in range(-2, src + 2)}
        a = {i: v for i, v in a.items() if v > 0}
        A = sum(a.values())
        return [(min(max(i, 0), src - 1), Fraction(v, A)) for i, v in a.items()]

    worst = Fraction(0)
    for f in S.FILTERS:
        for (sw, sh), (w, h) in (((9, 7), (4, 3)), ((5, 6), (9, 11)), ((16, 8), (2, 3)), ((7, 5), (7, 3)), ((12, 10), (5, 4)), ((3, 3), (8, 8)), ((17, 9), (3, 2))):
            p = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
            p[rng.integers(0, sh), :] = 255 * rng.integers(0, 2)
            got = M.scale_frames(np.stack([p] * 3).reshape(1, -1), sw, sh, w, h, "444", f).reshape(3, h, w)[0]
            for y in range(h):
                wy = weights(f, sh, h, y)
                for x in range(w):
                    wx = weights(f, sw, w, x)
                    exact = sum(dy * dx * int(p[j, i]) for j, dy in wy for i, dx in wx)
                    worst = max(worst, abs(exact - int(got[y, x])))
    print("largest deviation from exact fractions: %.4f" % float(worst))
    assert worst < Fraction(145, 100)


@pytest.mark.parametrize("kind", S.PASS_KINDS)
def test_host_build_reproduces_the_definition(kind):
    """csrc/m2v_scale_kernels.hpp compiled with g++ and walked tile by tile: pad_frames(scale_frames(x)) for every element size at the
    sizes of the pass alone, both filters"""
    for (sw, sh), (w, h) in S.PASS_SIZES:
        x = F.source(sw, sh, 1, kind, seed=500 + sw + w + 7 * h, noise=True)
        for f in S.FILTERS:
            want = M.pad_frames(M.scale_frames(x, sw, sh, w, h, kind, f), w, h, kind)
            got = S.host(x, sw, sh, w, h, kind, f)
            assert np.array_equal(got, want), (kind, f, sw, sh, w, h)
        t = S.host_lib()
        first, co = ctypes.c_int(0), (ctypes.c_uint16 * M.SCALE_MAXTAPS)()
        assert t.taps_host(0, sw, w, w - 1, ctypes.byref(first), co) == len(M.scale_taps(0, sw, w, w - 1)[1])


@pytest.mark.parametrize("fault", sorted(S.FAULTS) + ["V before H"])
def test_single_faults_change_the_result(fault):
    """the sizes of the pass alone reach the code: each fault changes the host build's result at one of them at least"""
    hit = []
    for (sw, sh), (w, h) in S.PASS_FIRST:
        for kind in ("444", "i420", "rgb24"):
            x = F.source(sw, sh, 1, kind, seed=600 + sw + w, noise=True)
            for f in S.FILTERS:
                want = M.pad_frames(M.scale_frames(x, sw, sh, w, h, kind, f), w, h, kind)
                if fault == "V before H":
                    if kind != "444":
                        continue
                    # the first pass along the columns: the transposed planes through the same code, and back
                    xt = np.ascontiguousarray(x.reshape(3, sh, sw).transpose(0, 2, 1)).reshape(1, -1)
                    got = M.scale_frames(xt, sh, sw, h, w, "444", f).reshape(3, w, h).transpose(0, 2, 1).reshape(1, -1)
                    got = M.pad_frames(np.ascontiguousarray(got), w, h, "444")
                else:
                    got = S.host(x, sw, sh, w, h, kind, f, fault)
                if got is None or not np.array_equal(got, want):
                    hit.append(((sw, sh), (w, h), kind, f))
    print("%s: %d of the cases differ" % (fault, len(hit)))
    assert hit, fault


def test_export_header_and_null_handle():
    L = M.lib()
    assert "m2v_set_source_size" in M.EXPORTS and "m2v_scale_taps" in M.EXPORTS
    assert L.m2v_set_source_size(None, 64, 64, 0) == E_PARAM
    with open(os.path.join(ROOT, "include", "m2v_mi355x.h")) as f:
        hdr = f.read()
    assert re.search(r"^int m2v_set_source_size\(m2v_enc \*e, int src_width, int src_height, int filter\);", hdr, re.M)
    assert re.search(r"^int m2v_scale_taps\(int filter, int src, int dst, int x, int \*first, uint16_t coeff\[M2V_SCALE_MAXTAPS\]\);", hdr, re.M)
    assert re.search(r"^enum \{ M2V_SCALE_TRIANGLE = 0, M2V_SCALE_AREA = 1 \};", hdr, re.M) and re.search(r"^#define M2V_SCALE_MAXTAPS 16$", hdr, re.M)
    assert M.SCALE_FILTERS == {"triangle": 0, "area": 1} and M.SCALE_MAXTAPS == 16
    assert "chroma siting is not modelled" in hdr.lower()
