"""4:2:0 input (I420, YV12, NV12, NV21), the part that needs no GPU: what "encoding a 4:2:0 frame" means, the numpy helpers that are
the GPU tests' reference, and the four entry points of the C-ABI.

The module has no 4:2:0 port.  The definition (include/m2v_mi355x.h): the stream of a 4:2:0 frame is the stream of the 4:4:4 frame whose
chroma planes are the 4:2:0 planes with every sample repeated 2 x 2 - the module's own down-conversion, two stages of mean2, then
returns exactly the planes the caller handed in."""
import ctypes
import os
import re

import numpy as np
import pytest

import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("i420", "yv12", "nv12", "nv21")


def mean2(a, b):
    """oracle/m2v_oracle.c's mean2, restated (RTL:1086-1089)"""
    return (a + b + 1) >> 1


def test_mean2_of_a_repeated_sample_is_the_sample():
    for a in range(256):
        assert mean2(mean2(a, a), mean2(a, a)) == a


@pytest.mark.parametrize("W,H", [(64, 64), (80, 112), (176, 144)])
def test_definition_oracle_codes_the_callers_chroma(W, H):
    """the oracle's 4:2:0 dump (what it goes on to encode) of the replicated clip IS the I420 input, in I420 order"""
    rng = np.random.default_rng(W * 1000 + H)
    x = rng.integers(0, 256, (4, W * H * 3 // 2), dtype=np.uint8)
    _, dumps = orc.encode(M.to444(x, W, H, "i420"), W // 16, H // 16, 3, dump=True)
    assert np.array_equal(dumps["yuv420"], x)


@pytest.mark.parametrize("W,H", [(64, 64), (80, 112), (176, 144)])
def test_helpers_round_trip_and_layouts_are_permutations(W, H):
    rng = np.random.default_rng(7 + W)
    x = rng.integers(0, 256, (3, W * H * 3 // 2), dtype=np.uint8)
    for l in LAYOUTS:
        up = M.to444(x, W, H, l)
        assert up.shape == (3, 3, H, W) and up.dtype == np.uint8
        assert np.array_equal(M.to420(up, l), x), l
        assert np.array_equal(up[:, 0].reshape(3, -1), x[:, :W * H]), l               # luma untouched
        for c in (1, 2):                                                              # every chroma sample 2 x 2
            p = up[:, c]
            assert np.array_equal(p[:, 0::2, 0::2], p[:, 1::2, 1::2]) and np.array_equal(p[:, 0::2, 1::2], p[:, 1::2, 0::2])
            assert np.array_equal(p[:, 0::2, 0::2], p[:, 0::2, 1::2])
    # one picture in the four layouts: the same samples in another order, and the same 4:4:4 frames
    pic = M.to444(x, W, H, "i420")
    forms = {l: M.to420(pic, l) for l in LAYOUTS}
    for l in LAYOUTS:
        assert np.array_equal(np.sort(forms[l], axis=1), np.sort(x, axis=1)), l
        assert np.array_equal(M.to444(forms[l], W, H, l), pic), l
    c = W * H // 4
    assert np.array_equal(forms["yv12"][:, W * H:W * H + c], x[:, W * H + c:])         # V first
    assert np.array_equal(forms["nv12"][:, W * H::2], x[:, W * H:W * H + c])           # U on the even bytes
    assert np.array_equal(forms["nv21"][:, W * H::2], x[:, W * H + c:])
    # names and codes are interchangeable
    assert M.LAYOUTS_420 == {"i420": 0, "yv12": 1, "nv12": 2, "nv21": 3}
    assert np.array_equal(M.to444(forms["nv21"], W, H, 3), pic)


def test_to420_is_the_modules_two_stage_mean2():
    """on chroma that is NOT 2 x 2 constant: horizontal pairs first, then vertical pairs, each rounded up"""
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (2, 3, 32, 48), dtype=np.uint8)
    got = M.to420(f, "i420")
    _, dumps = orc.encode(np.pad(f, ((0, 0), (0, 0), (0, 32), (0, 16)), mode="edge"), 4, 4, 0, dump=True)
    want = dumps["yuv420"].reshape(2, -1)
    yw = want[:, :64 * 64].reshape(2, 64, 64)[:, :32, :48]
    uw = want[:, 64 * 64:64 * 64 + 32 * 32].reshape(2, 32, 32)[:, :16, :24]
    vw = want[:, 64 * 64 + 32 * 32:].reshape(2, 32, 32)[:, :16, :24]
    assert np.array_equal(got[:, :32 * 48].reshape(2, 32, 48), yw)
    assert np.array_equal(got[:, 32 * 48:32 * 48 + 16 * 24].reshape(2, 16, 24), uw)
    assert np.array_equal(got[:, 32 * 48 + 16 * 24:].reshape(2, 16, 24), vw)


def test_abi_exports_and_header_declare_the_four_entry_points():
    M.build()
    L = M.lib()
    assert M.EXPORTS_420 == ["m2v_push_frames420", "m2v_push_frames420_pull", "m2v_encode_resident420", "m2v_encode_resident420_begin"]
    for n in M.EXPORTS_420:
        assert hasattr(L, n), "missing export " + n
    buf = ctypes.create_string_buffer(64)
    E_PARAM = -1
    assert L.m2v_push_frames420(None, 4, 4, 0, buf, 0, 0) == E_PARAM
    assert L.m2v_push_frames420_pull(None, 4, 4, 0, buf, 0, 0, buf, 64, None) == E_PARAM
    assert L.m2v_encode_resident420(None, 4, 4, 0, None, 0, 0, None, 0, None, None) == E_PARAM
    assert L.m2v_encode_resident420_begin(None, 4, 4, 0, None, 0, 0, None, 0, None) == E_PARAM
    txt = open(os.path.join(ROOT, "include", "m2v_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in M.EXPORTS_420:
        assert re.search(r"\b%s\s*\(" % n, code), n
    for k, name in enumerate(("M2V_420_I420", "M2V_420_YV12", "M2V_420_NV12", "M2V_420_NV21")):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, k), code), name
    # the header's rule (tests/test_abi.py::test_no_torch_or_hip_types_in_header) still holds
    assert "#include <hip" not in code and "torch" not in code and "hipStream_t" not in code and 'extern "C"' in code
    # m2v_debug_read's what = 4 is documented
    assert re.search(r"4 = the expanded 4:4:4 input", txt)


def test_tb_usage_error_for_two_layouts_before_any_device(tmp_path):
    """two layout options at once: exit status 2 and the usage text, before m2v_create (which would fail here with another message)"""
    import subprocess
    M.build()
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    f = tmp_path / "x.yuv"
    f.write_bytes(b"\0" * 64)
    r = subprocess.run([tb, "-i420", "-nv12", str(f), "64", "64", str(tmp_path / "x.m2v")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage:" in r.stderr and "m2v_create" not in r.stderr
    assert not (tmp_path / "x.m2v").exists()
