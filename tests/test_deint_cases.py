"""CPU: the definition of m2v_deinterlace_device (include/m2v_mi355x.h) in its three statements - deinterlace_frames (numpy),
tests/deint_ref.py (plain Python, sample by sample) and csrc/m2v_deint_kernels.hpp compiled with g++ and walked tile by tile as the kernel
walks - held against each other and against answers that none of them made; the host build once more under AddressSanitizer and UBSan as
a stand-alone program; the arguments, the bound, the header and EXPORTS.  Every comparison is exact.  tests/test_gpu_deinterlace.py runs
the same cases on the device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deint_cases as D
import deint_ref as R

M = D.M
E_PARAM, E_OVERFLOW = -1, -6
CASES = D.cases()
# what the reference walks sample by sample in Python: the small sizes of the covering array ...
SMALL = [c for c in CASES if c["size"] in D.SMALL_SIZES]
# ... and every legal mode, rate and order at one odd size with three frames, planar and interleaved
PROBES = [dict(size=(17, 5), nframes=3, layout=l, mode=m, rate=r, order=o) for l in ("i420", "nv12") for m in D.MODES for r in D.RATES for o in D.ORDERS
          if D.legal(dict(mode=m, rate=r))]


def luma(frames, h):
    return [list(map(int, f[:h])) for f in frames]


def test_covering_array():
    fs = D.factors()
    seen = set()
    for c in CASES:
        assert D.legal(c)
        seen |= D.pairs_of(c, fs)
    print("%d rows, %d pairs of levels" % (len(CASES), len(D.all_pairs())))
    assert seen == D.all_pairs()
    assert {c["size"] for c in CASES} == set(D.sizes()) and len(D.sizes()) == 23
    # the one pair left out is the one the definition refuses
    i, j = [n for n, _ in fs].index("mode"), [n for n, _ in fs].index("rate")
    n_all = sum(len(a[1]) * len(b[1]) for k, a in enumerate(fs) for b in fs[k + 1:])
    assert len(D.all_pairs()) == n_all - 1 and ((i, D.MODES.index("blend")), (j, D.RATES.index("field"))) not in D.all_pairs()


def test_tile_is_the_kernels():
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    D.host_lib().deint_host_tile(ctypes.byref(c), ctypes.byref(r))
    assert (c.value, r.value) == D.TILE == M.deinterlace_tile()


@pytest.mark.parametrize("k", range(len(D.LITERALS)))
def test_literals_of_the_definition(k):
    rows, mode, rate, order, want = D.LITERALS[k]
    h = len(rows[0])
    for layout in D.LAYOUTS:
        x = D.column(rows, layout)
        assert luma(M.deinterlace_frames(x, 1, h, layout, mode, rate, order), h) == want
        assert luma(D.host(x, 1, h, layout, mode, rate, order), h) == want
        got = np.frombuffer(R.deinterlace(x.tobytes(), 1, h, layout, mode, rate, order), np.uint8).reshape(len(want), -1)
        assert luma(got, h) == want


@pytest.mark.parametrize("c", CASES, ids=D.name_of)
def test_host_build_reproduces_the_definition(c):
    """csrc/m2v_deint_kernels.hpp compiled with g++ and walked as k_deint walks, on the kernel's grid and on grids of one and of three
    blocks (every item then comes out of the grid-stride loop)"""
    w, h = c["size"]
    x, want = D.source(c), D.expected(c)
    assert want.shape == (c["nframes"] * (2 if c["rate"] == "field" else 1), M.frame_bytes(w, h, c["layout"]))
    for blocks in (0, 1, 3):
        got = D.host(x, w, h, c["layout"], c["mode"], c["rate"], c["order"], max_blocks=blocks)
        assert np.array_equal(got, want), (D.name_of(c), blocks, int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0]))


@pytest.mark.parametrize("c", SMALL + PROBES, ids=D.name_of)
def test_reference_agrees(c):
    w, h = c["size"]
    x = D.source(c)
    assert R.deinterlace(x.tobytes(), w, h, c["layout"], c["mode"], c["rate"], c["order"]) == D.expected(c, x).tobytes()


@pytest.mark.parametrize("wrong", R.WRONG)
def test_each_wrong_form_changes_a_case(wrong):
    """the cases tell every classic wrong form from the definition; the test names which"""
    hit = []
    for c in PROBES + SMALL:
        w, h = c["size"]
        x = D.source(c)
        if R.deinterlace(x.tobytes(), w, h, c["layout"], c["mode"], c["rate"], c["order"], wrong=wrong) != D.expected(c, x).tobytes():
            hit.append(D.name_of(c))
            if len(hit) == 3:
                break
    print("%s: changes %s" % (wrong, ", ".join(hit)))
    assert hit, wrong


def both(x, w, h, layout, mode, rate, order):
    a = M.deinterlace_frames(x, w, h, layout, mode, rate, order)
    assert np.array_equal(D.host(x, w, h, layout, mode, rate, order), a)
    return a


@pytest.mark.parametrize("n", D.NFRAMES)
def test_equal_frames_come_back_under_adaptive(n):
    """where nothing moves the other field is woven in: the frames unchanged, twice each at field rate"""
    rng = np.random.default_rng(40 + n)
    for (w, h), layout in (((35, 9), "i420"), ((48, 32), "nv12"), ((2, 3), "yv12"), ((257, 17), "nv21")):
        one = rng.integers(0, 256, M.frame_bytes(w, h, layout), dtype=np.uint8)
        x = np.stack([one] * n)
        for order in D.ORDERS:
            assert np.array_equal(both(x, w, h, layout, "adaptive", "frame", order), x)
            assert np.array_equal(both(x, w, h, layout, "adaptive", "field", order), np.repeat(x, 2, axis=0))


def test_frames_of_equal_rows_come_back():
    rng = np.random.default_rng(50)
    for (w, h), layout in (((17, 5), "i420"), ((48, 32), "nv12"), ((1, 2), "yv12")):
        for n in (1, 3):
            x = np.concatenate([np.repeat(rng.integers(0, 256, (n, 1, es * c), dtype=np.uint8), r, axis=1).reshape(n, -1) for es, c, r, _ in M._planes(w, h, layout)], axis=1)
            for mode in D.MODES:
                for rate in D.RATES:
                    if not D.legal(dict(mode=mode, rate=rate)):
                        continue
                    for order in D.ORDERS:
                        got = both(x, w, h, layout, mode, rate, order)
                        assert np.array_equal(got, np.repeat(x, 2, axis=0) if rate == "field" else x), (w, h, layout, n, mode, rate, order)


def test_adaptive_is_line_where_everything_moves():
    """the kept rows alternate all 0 and all 255 from frame to frame: t1 or t2 is 255, the clamp is open, whatever the other rows hold"""
    rng = np.random.default_rng(60)
    for (w, h), layout in (((35, 9), "i420"), ((48, 32), "nv21")):
        for n in (2, 3, 5):
            for order in D.ORDERS:
                p = D.ORDERS.index(order)
                x = rng.integers(0, 256, (n, M.frame_bytes(w, h, layout)), dtype=np.uint8)
                at = 0
                for es, c, r, _ in M._planes(w, h, layout):
                    v = x[:, at:at + es * c * r].reshape(n, r, es * c)
                    for k in range(n):
                        v[k, p::2] = 255 * (k & 1)
                    at += es * c * r
                assert np.array_equal(both(x, w, h, layout, "adaptive", "frame", order), both(x, w, h, layout, "line", "frame", order))


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(c, D.source(c), (0, 1, 3)[k % 3]) for k, c in enumerate(CASES)]
    items += [(dict(size=(1, h), nframes=len(rows), layout="i420", mode=mode, rate=rate, order=order), D.column(rows), 0)
              for rows, mode, rate, order, _ in D.LITERALS for h in [len(rows[0])]]
    path, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    path.write_bytes(D.pack_cases(items))
    exe = str(tmp_path / "deint_host_check")
    # the sanitizers' runtimes linked in: the program starts with whatever environment the test has
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", D.CSRC, "-I", os.path.join(D.ROOT, "tools"), "-o", exe,
                           os.path.join(D.ROOT, "tools", "deint_host_check.cpp")])
    p = subprocess.run([exe, str(path), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    got, at = out.read_bytes(), 0
    for (c, x, _), line in zip(items, lines):
        want = D.expected(c, x).tobytes()
        assert line == "0 %d" % len(want), (D.name_of(c), line)
        assert got[at:at + len(want)] == want, D.name_of(c)
        at += len(want)
    assert at == len(got)


# ---- the arguments ----
def test_bound_against_frame_bytes():
    L, H = M.lib(), D.host_lib()
    for w, h in D.sizes() + [(720, 576), (1920, 1080), (16384, 16384), (16383, 16383)]:
        fb = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        assert all(M.frame_bytes(w, h, l) == fb for l in D.LAYOUTS)
        for n in (0, 1, 3, 30, 1 << 20):
            for rate in (0, 1):
                assert M.deinterlace_bound(w, h, n, rate) == H.deint_host_bound(w, h, n, rate) == n * fb * (1 + rate), (w, h, n, rate)
    assert M.deinterlace_bound(720, 576, 30, "field") == 2 * 30 * 622080
    for w, h, n, rate in ((0, 16, 1, 0), (16, 1, 1, 0), (16385, 16, 1, 0), (16, 16385, 1, 0), (-1, 16, 1, 0), (16, 16, 1, 2), (16, 16, 1, -1), (16384, 16384, 1 << 62, 0)):
        assert L.m2v_deinterlace_bound(w, h, n, rate) == 0 and H.deint_host_bound(w, h, n, rate) == 0, (w, h, n, rate)


def test_every_refusal_of_the_arguments():
    """the function the entry answers with before it looks at the handle (check_args of csrc/m2v_deint_kernels.hpp; the entry itself is
    held to the same table on the device)"""
    chk = D.host_lib().deint_host_check
    fb = M.frame_bytes(48, 32, "i420")
    src, dst = 1 << 32, 1 << 33

    def a(**kw):
        d = dict(src=src, n=3, w=48, h=32, layout=0, mode=1, rate=0, order=0, dst=dst, cap=3 * fb)
        d.update(kw)
        return chk(d["src"], d["n"], d["w"], d["h"], d["layout"], d["mode"], d["rate"], d["order"], d["dst"], d["cap"])
    assert a() == 0 and a(rate=1, cap=6 * fb) == 0 and a(mode=2) == 0 and a(order=1, layout=3) == 0
    for kw in (dict(layout=4), dict(layout=-1), dict(mode=3), dict(mode=-1), dict(rate=2), dict(rate=-1), dict(order=2), dict(order=-1), dict(mode=2, rate=1, cap=6 * fb),
               dict(w=0), dict(h=1), dict(w=16385), dict(h=16385), dict(h=0), dict(w=-5)):
        assert a(**kw) == E_PARAM, kw
    assert a(h=2, w=1) == 0 and a(w=16384, h=16384, cap=1 << 40) == 0
    # the ranges: touching is legal, one byte in common is not, whichever lies first; at field rate the output is twice as long
    assert a(dst=src + 3 * fb) == 0 and a(dst=src + 3 * fb - 1) == E_PARAM and a(dst=src) == E_PARAM
    assert a(dst=src - 3 * fb) == 0 and a(dst=src - 3 * fb + 1) == E_PARAM
    assert a(rate=1, cap=6 * fb, dst=src - 6 * fb) == 0 and a(rate=1, cap=6 * fb, dst=src - 6 * fb + 1) == E_PARAM
    assert a(src=0) == E_PARAM and a(dst=0) == E_PARAM
    # cap
    assert a(cap=3 * fb - 1) == E_OVERFLOW and a(cap=0) == E_OVERFLOW and a(rate=1, cap=6 * fb - 1) == E_OVERFLOW
    # a refusal of the arguments goes before the capacity; no frames need no pointers and no room
    assert a(cap=0, mode=7) == E_PARAM and a(cap=0, dst=src) == E_PARAM
    assert a(n=0, cap=0, src=0, dst=0) == 0 and a(n=0, cap=0, layout=9) == E_PARAM


def test_export_header_and_null_handle():
    L = M.lib()
    for name in ("m2v_deinterlace_device", "m2v_deinterlace_bound", "m2v_deinterlace_tile"):
        assert name in M.EXPORTS and hasattr(L, name)
    assert L.m2v_deinterlace_device(None, None, 0, 48, 32, 0, 0, 0, 0, None, 0, None) == E_PARAM
    with open(os.path.join(D.ROOT, "include", "m2v_mi355x.h")) as f:
        hdr = f.read()
    assert re.search(r"^enum \{ M2V_DEINT_LINE = 0, M2V_DEINT_ADAPTIVE = 1, M2V_DEINT_BLEND = 2 \};", hdr, re.M)
    assert re.search(r"^enum \{ M2V_DEINT_FRAME_RATE = 0, M2V_DEINT_FIELD_RATE = 1 \};", hdr, re.M)
    assert re.search(r"^enum \{ M2V_DEINT_TFF = 0, M2V_DEINT_BFF = 1 \};", hdr, re.M)
    assert re.search(r"^int m2v_deinterlace_device\(m2v_enc \*e, const void \*d_src, size_t nframes, int width, int height, int layout,\n"
                     r"\s+int mode, int rate, int order, void \*d_dst, size_t cap, void \*hip_stream\);", hdr, re.M)
    assert re.search(r"^unsigned long long m2v_deinterlace_bound\(int width, int height, size_t nframes, int rate\);", hdr, re.M)
    assert re.search(r"^int m2v_deinterlace_tile\(int \*cols, int \*rows\);", hdr, re.M)
    assert M.DEINT_MODES == {"line": 0, "adaptive": 1, "blend": 2} and M.DEINT_RATES == {"frame": 0, "field": 1} and M.DEINT_ORDERS == {"tff": 0, "bff": 1}
    for word in ("pulldown", "edge-directed", "top_field_first", "batch entries"):
        assert word in hdr, word
    with pytest.raises(ValueError):
        M.deinterlace_frames(np.zeros((1, M.frame_bytes(4, 4, "i420")), np.uint8), 4, 4, "i420", "blend", "field")
    with pytest.raises(ValueError):
        M.deinterlace_frames(np.zeros((1, M.frame_bytes(4, 4, "i420")), np.uint8), 4, 4, "i420", "bob")
