"""RGB input, the part that needs no GPU: what "encoding an RGB frame" means, the numpy helper that is the GPU tests' reference, the
coefficient table in its three places, and the five entry points of the C-ABI.

The module has no RGB port.  The definition (include/m2v_mi355x.h): the stream of an RGB frame is the stream of the planar 4:4:4 frame
obtained by an integer transform (3 x 3 integers of scale 2^14, a luma offset, round, clamp); the module's own two-stage mean2 then
makes the 4:2:0 chroma from those planes as for any 4:4:4 caller."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("rgb24", "bgr24", "rgbx", "bgrx", "xrgb", "xbgr", "rgbp")
MATRICES = ("bt601", "bt709", "bt601f", "bt709f")

# the table of the definition: T row by row (Y, U, V x R, G, B), luma offset
TABLE = {
    "bt601": ((4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170), 16),
    "bt709": ((2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660), 16),
    "bt601f": ((4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332), 0),
    "bt709f": ((3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751), 0),
}
# what the definition is built from: Kr, Kb, luma scale, chroma scale
BASIS = {
    "bt601": (Fraction(299, 1000), Fraction(114, 1000), Fraction(219, 255), Fraction(224, 255)),
    "bt709": (Fraction(2126, 10000), Fraction(722, 10000), Fraction(219, 255), Fraction(224, 255)),
    "bt601f": (Fraction(299, 1000), Fraction(114, 1000), Fraction(1), Fraction(1)),
    "bt709f": (Fraction(2126, 10000), Fraction(722, 10000), Fraction(1), Fraction(1)),
}
# known answers (Y, U, V), in the order of MATRICES
KNOWN = {
    (0, 0, 0): ((16, 128, 128), (16, 128, 128), (0, 128, 128), (0, 128, 128)),
    (255, 255, 255): ((235, 128, 128), (235, 128, 128), (255, 128, 128), (255, 128, 128)),
    (128, 128, 128): ((126, 128, 128), (126, 128, 128), (128, 128, 128), (128, 128, 128)),
    (255, 0, 0): ((81, 90, 240), (63, 102, 240), (76, 85, 255), (54, 99, 255)),
    (0, 255, 0): ((145, 54, 34), (173, 42, 26), (150, 44, 21), (182, 30, 12)),
    (0, 0, 255): ((41, 240, 110), (32, 240, 118), (29, 255, 107), (18, 255, 116)),
}


def pack(rgb, layout, rng=None):
    """[n, H, W, 3] RGB pictures -> frames [n, W*H*bpp] in `layout`; the ignored byte of the 32-bit layouts is noise when rng is given"""
    n, H, W, _ = rgb.shape
    if layout == "rgbp":
        return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2)).reshape(n, -1)
    bpp, where = {"rgb24": (3, (0, 1, 2)), "bgr24": (3, (2, 1, 0)), "rgbx": (4, (0, 1, 2)), "bgrx": (4, (2, 1, 0)), "xrgb": (4, (1, 2, 3)),
                  "xbgr": (4, (3, 2, 1))}[layout]
    px = np.zeros((n, H, W, bpp), np.uint8) if rng is None else rng.integers(0, 256, (n, H, W, bpp), dtype=np.uint8)
    for c in range(3):
        px[..., where[c]] = rgb[..., c]
    return px.reshape(n, -1)


def r14(x):
    """floor(x * 2^14 + 1/2), exact"""
    return (x * 2 ** 14 + Fraction(1, 2)).__floor__()


def test_the_table_in_its_three_places_and_its_derivation():
    M.build()
    L = M.lib()
    assert tuple(M.MATRICES_RGB) == MATRICES
    for code, name in enumerate(MATRICES):
        T, yo = TABLE[name]
        c, o = (ctypes.c_int * 9)(), ctypes.c_int(-1)
        assert L.m2v_rgb_matrix(code, c, ctypes.byref(o)) == 0
        assert (tuple(c), o.value) == (T, yo), name
        assert M.MATRICES_RGB[name] == (code, T, yo), name
        Kr, Kb, sy, sc = BASIS[name]
        t00, t02 = r14(Kr * sy), r14(Kb * sy)
        t12, t10 = r14(sc / 2), r14(-Kr * sc / (2 * (1 - Kb)))
        t20, t22 = r14(sc / 2), r14(-Kb * sc / (2 * (1 - Kr)))
        assert T == (t00, r14(sy) - t00 - t02, t02, t10, -t10 - t12, t12, t20, -t20 - t22, t22), name
        assert yo == (16 if sy != 1 else 0)
        assert sum(T[3:6]) == 0 and sum(T[6:9]) == 0 and sum(T[0:3]) == r14(sy)
    for bad in (-1, 4, 99):
        assert L.m2v_rgb_matrix(bad, None, None) == -1            # M2V_E_PARAM
    assert L.m2v_rgb_matrix(0, None, None) == 0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_known_answers_in_every_layout(layout):
    for rgb, answers in KNOWN.items():
        pic = np.empty((1, 16, 16, 3), np.uint8)
        pic[...] = rgb
        x = pack(pic, layout)
        for k, name in enumerate(MATRICES):
            got = M.rgb_to444(x, 16, 16, layout, name)
            assert got.shape == (1, 3, 16, 16) and got.dtype == np.uint8
            for c in range(3):
                assert (got[0, c] == answers[k][c]).all(), (rgb, name, c, int(got[0, c, 0, 0]), answers[k][c])
            assert np.array_equal(got, M.rgb_to444(x, 16, 16, M.LAYOUTS_RGB[layout], k))       # names and codes are interchangeable


@pytest.mark.parametrize("name", MATRICES)
def test_exhaustive_against_the_real_valued_transform(name, capsys):
    """all 2^24 inputs, one red value at a time (a 256 x 256 frame of every green x blue)"""
    T, yo = TABLE[name]
    Kr, Kb, sy, sc = (float(v) for v in BASIS[name])
    Kg = 1.0 - Kr - Kb
    studio = yo == 16
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    frame = np.empty((256, 256, 3), np.uint8)
    frame[..., 1], frame[..., 2] = g, b
    g, b = g.astype(np.float64), b.astype(np.float64)
    worst = 0.0
    for r in range(256):
        frame[..., 0] = r
        got = M.rgb_to444(frame, 256, 256, "rgb24", name)[0].astype(np.int64)
        luma = Kr * r + Kg * g + Kb * b
        real = (sy * luma + yo, sc * (b - luma) / (2 * (1 - Kb)) + 128, sc * (r - luma) / (2 * (1 - Kr)) + 128)
        ri, gi, bi = r, frame[..., 1].astype(np.int64), frame[..., 2].astype(np.int64)
        for c in range(3):
            worst = max(worst, float(np.abs(got[c] - np.clip(real[c], 0, 255)).max()))
            raw = ((T[3 * c] * ri + T[3 * c + 1] * gi + T[3 * c + 2] * bi + 8192) >> 14) + (yo if c == 0 else 128)
            assert np.abs(T[3 * c] * ri + T[3 * c + 1] * gi + T[3 * c + 2] * bi + 8192).max() < 2 ** 23       # every sum fits 24 bits, signed
            if studio:                                         # no clamp ever acts, and the ranges are the studio ones
                assert raw.min() >= 16 and raw.max() <= (235 if c == 0 else 240), (name, r, c)
            else:
                assert raw.min() >= 0 and raw.max() <= (255 if c == 0 else 256), (name, r, c)
            assert np.array_equal(np.clip(raw, 0, 255), got[c]), (name, r, c)
        grey = got[:, r, r]
        assert grey[1] == 128 and grey[2] == 128, (name, r)
    with capsys.disabled():
        print("%s: largest distance from the real-valued transform over 2^24 inputs: %.4f" % (name, worst))
    assert worst <= 0.508, (name, worst)


@pytest.mark.parametrize("W,H", [(64, 64), (80, 112)])
def test_seven_layouts_of_one_picture_give_one_result(W, H):
    rng = np.random.default_rng(W + H)
    pic = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    for name in MATRICES:
        want = M.rgb_to444(pack(pic, "rgb24"), W, H, "rgb24", name)
        for layout in LAYOUTS:
            a = pack(pic, layout, np.random.default_rng(1))
            b = pack(pic, layout, np.random.default_rng(2))        # another ignored byte
            assert a.shape[1] == W * H * M.rgb_bytes_per_pixel(layout)
            assert np.array_equal(M.rgb_to444(a, W, H, layout, name), want), (layout, name)
            assert np.array_equal(M.rgb_to444(b, W, H, layout, name), want), (layout, name)
            if a.shape[1] == W * H * 4:
                assert not np.array_equal(a, b)
    assert M.LAYOUTS_RGB == {"rgb24": 0, "bgr24": 1, "rgbx": 2, "bgrx": 3, "xrgb": 4, "xbgr": 5, "rgbp": 6}


@pytest.mark.parametrize("W,H", [(64, 64), (80, 112)])
def test_definition_the_oracle_applies_the_modules_own_down_conversion(W, H):
    """the oracle's 4:2:0 dump (what it goes on to encode) of the converted clip is to420 of it: mean2 twice, nothing else"""
    rng = np.random.default_rng(W * 1000 + H)
    x = rng.integers(0, 256, (4, W * H * 3), dtype=np.uint8)
    for layout, name in (("rgb24", "bt601"), ("rgbp", "bt709f")):
        y = M.rgb_to444(x, W, H, layout, name)
        _, dumps = orc.encode(y, W // 16, H // 16, 3, dump=True)
        assert np.array_equal(dumps["yuv420"].reshape(4, -1), M.to420(y, "i420")), (layout, name)


def test_abi_exports_header_and_null_handle():
    M.build()
    L = M.lib()
    names = ["m2v_rgb_matrix", "m2v_push_rgb", "m2v_push_rgb_pull", "m2v_encode_resident_rgb", "m2v_encode_resident_rgb_begin"]
    txt = open(os.path.join(ROOT, "include", "m2v_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in names:
        assert n in M.EXPORTS, n
        assert hasattr(L, n), "missing export " + n
        assert re.fullmatch(r"m2v_[a-z_]+", n)
        assert re.search(r"\b%s\s*\(" % n, code), n
    enums = [("M2V_RGB_BT601", 0), ("M2V_RGB_BT709", 1), ("M2V_RGB_BT601F", 2), ("M2V_RGB_BT709F", 3),
             ("M2V_RGB_RGB24", 0), ("M2V_RGB_BGR24", 1), ("M2V_RGB_RGBX32", 2), ("M2V_RGB_BGRX32", 3), ("M2V_RGB_XRGB32", 4),
             ("M2V_RGB_XBGR32", 5), ("M2V_RGB_RGBP", 6)]
    for name, k in enums:
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, k), code), name
    buf = ctypes.create_string_buffer(64)
    E_PARAM = -1
    assert L.m2v_push_rgb(None, 4, 4, 0, buf, 0, 0, 0) == E_PARAM
    assert L.m2v_push_rgb_pull(None, 4, 4, 0, buf, 0, 0, 0, buf, 64, None) == E_PARAM
    assert L.m2v_encode_resident_rgb(None, 4, 4, 0, None, 0, 0, 0, None, 0, None, None) == E_PARAM
    assert L.m2v_encode_resident_rgb_begin(None, 4, 4, 0, None, 0, 0, 0, None, 0, None) == E_PARAM
    assert "#include <hip" not in code and "torch" not in code and "hipStream_t" not in code and 'extern "C"' in code
    # the definition is in the header: the formula's constants and every coefficient of the table
    for T, _ in TABLE.values():
        for c in T:
            assert re.search(r"(?<![0-9])%d(?![0-9])" % c, txt), c
    assert "8192" in txt and ">> 14" in txt and "sequence_display_extension" in txt


@pytest.mark.parametrize("opts", [("-rgb24", "-nv12"), ("-rgb24", "-bgr24"), ("-rgbp", "-xbgr"), ("-i420", "-bgrx"),
                                  ("-rgb24", "-matrix", "nosuch"), ("-matrix", "nosuch")])
def test_tb_usage_errors_before_any_device(tmp_path, opts):
    """exit status 2 and the usage text, before m2v_create (which would fail here with another message)"""
    M.build()
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    f = tmp_path / "x.rgb"
    f.write_bytes(b"\0" * 64)
    r = subprocess.run([tb] + list(opts) + [str(f), "64", "64", str(tmp_path / "x.m2v")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage:" in r.stderr and "-matrix" in r.stderr and "m2v_create" not in r.stderr
    assert not (tmp_path / "x.m2v").exists()
