"""The clips of tests/stats_cases.py exercise what the picture statistics report (no GPU): every picture has an error in every plane,
a P picture mixes intra and inter macroblocks with vectors, the frame-size crop changes the sums - so the -m gpu comparisons of
tests/test_gpu_picture_stats.py are not vacuous.  Plus the host side of the feature: the PSNR helper, the record's layout, the export,
and a second opinion on the expected sums from the package's own decoder."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import stats_cases as S

M = S.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(S.CASES) + sorted(S.FIT_CASES)


def recs(name):
    return S.case(name)["records"] if name in S.CASES else S.fit_case(name)["records"]


@pytest.mark.parametrize("name", ALL)
def test_every_picture_has_error_in_every_plane(name):
    r = recs(name)
    assert len(r) == (S.CASES.get(name) or S.FIT_CASES[name])["n"]
    assert (r["sse"] > 0).all(), r["sse"]
    assert (r["mb_bits"] > 0).all() and (r["coded_blocks"] > 0).all()
    assert list(r["frame"]) == list(range(len(r)))


@pytest.mark.parametrize("name", [n for n in ALL if n != "ionly"])
def test_a_p_picture_mixes_decisions_and_has_vectors(name):
    r = recs(name)
    p = r[r["coding_type"] == 2]
    assert len(p) and ((p["intra_mbs"] > 0) & (p["inter_mbs"] > 0) & (p["mv_abs_x"] + p["mv_abs_y"] > 0)).any(), p
    i = r[r["coding_type"] == 1]
    assert (i["inter_mbs"] == 0).all() and (i["mv_abs_x"] + i["mv_abs_y"] == 0).all()


def test_i_only_case_has_no_p_picture():
    r = recs("ionly")
    assert (r["coding_type"] == 1).all() and (r["inter_mbs"] == 0).all()


@pytest.mark.parametrize("name", sorted(S.FIT_CASES))
def test_crop_changes_the_sums(name):
    c = S.fit_case(name)
    assert (c["records"]["sse"] < c["uncropped"]["sse"]).all()
    for k in ("mb_bits", "intra_mbs", "inter_mbs", "coded_blocks", "mv_abs_x", "mv_abs_y"):       # the padding is coded: counted
        assert np.array_equal(c["records"][k], c["uncropped"][k])
    assert S.samples3(c["W"], c["H"], (c["w"], c["h"])) == [c["w"] * c["h"]] + [((c["w"] + 1) // 2) * ((c["h"] + 1) // 2)] * 2
    assert (c["W"], c["H"]) == {"fit49": (64, 64)}.get(name, (112, 80))


def test_cut_frame_counts_its_fill():
    """the stop after 2 1/2 frames: the oracle's yuv420 of the last picture is black below the cut (Y = 0, U = V = 128)"""
    c = S.case("beats")
    y, u, v = S.planes420(c["dump"]["yuv420"][2], 64, 64)
    assert len(c["records"]) == 3 and (y[32:] == 0).all() and (u[16:] == 128).all() and (v[16:] == 128).all() and y[:32].any()


def test_psnr_from_sse():
    assert M.psnr_from_sse(0, 100) == math.inf
    assert M.psnr_from_sse(65025 * 100, 100) == 0.0
    assert abs(M.psnr_from_sse(100, 100) - 20 * math.log10(255)) < 1e-12             # MSE 1: 48.13 dB
    a = M.psnr_from_sse(np.array([0, 400]), np.array([100, 100]))
    assert a[0] == math.inf and abs(a[1] - (20 * math.log10(255) - 10 * math.log10(4))) < 1e-12


def test_record_layout():
    assert ctypes.sizeof(M.PictureStat) == 64 and M.PICTURE_STAT_DTYPE.itemsize == 64
    for name, _ in M.PictureStat._fields_:
        assert getattr(M.PictureStat, name).offset == M.PICTURE_STAT_DTYPE.fields[name][1], name
    # the header's struct, field by field in order
    txt = open(os.path.join(ROOT, "include", "m2v_mi355x.h")).read()
    body = re.search(r"typedef struct m2v_picture_stat \{(.*?)\} m2v_picture_stat;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in M.PictureStat._fields_]


def test_library_exports_the_entry():
    L = M.lib()
    assert hasattr(L, "m2v_picture_stats") and "m2v_picture_stats" in M.EXPORTS
    assert L.m2v_picture_stats(None, None, 0) == -1            # M2V_E_PARAM: no handle, no GPU needed


@pytest.mark.parametrize("name", ["unref", "conformant", "beats"])
def test_second_opinion_from_the_decoder(name):
    """the package's own decoder (quirks = the module's reconstruction loop; the conformant stream: a standard decoder) against the
    oracle's two-stage subsampling of the source gives the sums the records are expected to hold"""
    c = S.case(name)
    W, H = c["W"], c["H"]
    d = M.decoder.decode(c["stream"], quirks=not c.get("conformant", False))
    assert len(d.frames) == c["n"]
    frames = np.array(c["frames"])
    if name == "beats":                                         # the fill, as the module's input stage makes it (RTL:1048-1056)
        frames[2, 0].reshape(-1)[2048:] = 0
        frames[2, 1:].reshape(2, -1)[:, 2048:] = 128
    for f in range(c["n"]):
        src = [frames[f, 0]]
        for p in (1, 2):
            o = np.zeros((H // 2, W // 2), np.uint8)
            S.orc.lib().m2v_oracle_subsample(np.ascontiguousarray(frames[f, p]).ctypes.data, W, H, o.ctypes.data)
            src.append(o)
        got = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(src, d.frames[f])]
        assert got == list(c["records"]["sse"][f]), (name, f)
