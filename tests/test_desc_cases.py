"""CPU: the stream description (m2v_set_stream_desc) - the helper of tests/desc_cases.py against the oracle, the plain arithmetic the
library exports (m2v_time_code, m2v_frame_rate_code, m2v_stream_desc_module) against the helper, and the host tools that read streams
(decoder.py, m2vc_scan, m2vc_mux_ps) on described streams built from the oracle's.  No GPU: tests/test_gpu_stream_desc.py holds the
encoder against the same helper."""
import ctypes

import numpy as np
import pytest

import desc_cases as D
import gop_cases as G
import scene_cases as S

M = D.M
E_PARAM = -1


@pytest.fixture(scope="module")
def L():
    M.build()
    return M.lib()


@pytest.fixture(scope="module")
def c96():
    """the plain oracle stream of c96 at pframes_count 2: four GOPs of three pictures"""
    f, W, H = G.clip_args("c96")
    return G.encoded(f, W, H, 2, 2)[0], D.cadence(len(f), 2), W, H


EVERY_FIELD = D.desc(frame_rate_code=3, aspect_ratio_information=3, bit_rate_400=(1 << 30) - 1, vbv_buffer_size_16k=(1 << 18) - 1,
                     video_format=5, colour_primaries=1, transfer_characteristics=2, matrix_coefficients=3, display_width=16383,
                     display_height=1, repeat_headers=1)


# ---- the helper against the oracle ----
@pytest.mark.parametrize("name,pf", [("c64", 0), ("c80", 2), ("c96", 2)])
def test_seq_headers_of_the_module_are_the_oracles(name, pf):
    f, W, H = G.clip_args(name)
    st = G.encoded(f, W, H, pf, 2)[0]
    assert D.seq_headers(W, H, D.MODULE) == st[:34]
    assert D.described(st, D.cadence(len(f), pf), D.MODULE) == st


def test_time_code_at_24_is_the_oracles():
    for n in list(range(0, 3000)) + [86399, 86400, 63 * 86400 - 1, 63 * 86400, (1 << 32) - 1]:
        assert D.time_code(n, 2) == S.time_code(n) == D.time_code(n, 1)
    f, W, H = D.ionly()
    head, gops = G.cut(G.encoded(f, W, H, 0, 2)[0])
    assert len(gops) == 62
    for n, g in enumerate(gops):
        assert g[4:8] == D.time_code(n, 2), n


# ---- the library's arithmetic against the helper ----
def test_time_code_export(L):
    out = (ctypes.c_uint8 * 4)()
    for code, F in D.RATE.items():
        for n in (0, F - 1, F, 60 * F - 1, 60 * F, 3600 * F - 1, 3600 * F, 63 * 3600 * F - 1, 63 * 3600 * F, 64 * 3600 * F, (1 << 32) - 1):
            assert L.m2v_time_code(code, n, out) == 0
            assert bytes(out) == D.time_code(n, code) == M.time_code(n, code), (code, n)
    for bad in (0, 9, 255):
        assert L.m2v_time_code(bad, 0, out) == E_PARAM
    assert L.m2v_time_code(2, 0, None) == E_PARAM


def test_frame_rate_code_export(L):
    table = {1: (24000, 1001), 2: (24, 1), 3: (25, 1), 4: (30000, 1001), 5: (30, 1), 6: (50, 1), 7: (60000, 1001), 8: (60, 1)}
    for code, (n, d) in table.items():
        assert L.m2v_frame_rate_code(n, d) == code
        assert L.m2v_frame_rate_code(7 * n, 7 * d) == code                    # an equal rational
        assert M.container.frame_rate(code) == (n, d)                         # the table the multiplexers stamp PTS with
    assert L.m2v_frame_rate_code(30000, 1000) == 5 and L.m2v_frame_rate_code(48000, 2002) == 1
    assert L.m2v_frame_rate_code(4290000000, 143000000) == 5                  # 64-bit products
    for n, d in ((0, 1), (1, 0), (0, 0), (15, 1), (30000, 1002), (24001, 1001), (61, 1)):
        assert L.m2v_frame_rate_code(n, d) == E_PARAM, (n, d)


def test_module_description_and_size(L):
    d = M.StreamDesc()
    assert ctypes.sizeof(d) == 48
    L.m2v_stream_desc_module(ctypes.byref(d))
    assert {k: getattr(d, k) for k in D.FIELDS} == D.MODULE
    assert [k for k, _ in M.StreamDesc._fields_] == list(D.FIELDS)
    L.m2v_stream_desc_module(None)                                            # like free(NULL)
    assert L.m2v_set_stream_desc(None, ctypes.byref(d)) == E_PARAM


def test_python_stream_desc():
    as_dict = lambda d: {k: getattr(d, k) for k in D.FIELDS}
    assert as_dict(M.stream_desc()) == D.MODULE
    d = M.stream_desc(fps=(30000, 1001), aspect="16:9", bit_rate=8_000_001, vbv_bits=16385, video_format=0, colour="bt709", display=(100, 70),
                      repeat_headers=True)
    assert as_dict(d) == D.desc(frame_rate_code=4, aspect_ratio_information=3, bit_rate_400=20001, vbv_buffer_size_16k=2, video_format=0,
                                colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1, display_width=100, display_height=70,
                                repeat_headers=1)
    assert as_dict(M.stream_desc(colour="bt601")) == D.MODULE and as_dict(M.stream_desc(colour=(9, 16, 9))) == D.desc(
        colour_primaries=9, transfer_characteristics=16, matrix_coefficients=9)
    for fps, code in ((23.976, 1), (24, 2), (25.0, 3), (29.97, 4), (30, 5), (50, 6), (59.94, 7), (60, 8), ((50, 1), 6)):
        assert M.stream_desc(fps=fps).frame_rate_code == code
    for bad in (dict(fps=23.9), dict(fps=(15, 1)), dict(aspect="5:4"), dict(colour="bt2020")):
        with pytest.raises(ValueError):
            M.stream_desc(**bad)


# ---- the decoder ----
def same_planes(a, b):
    return len(a.frames) == len(b.frames) and all(np.array_equal(p, q) for x, y in zip(a.frames, b.frames) for p, q in zip(x, y))


@pytest.fixture(scope="module")
def plain_decode(c96):
    return M.decoder.decode(c96[0])


def test_decoder_exposes_the_modules_description(plain_decode, c96):
    s = plain_decode.sequence
    assert (s["frame_rate_code"], s["aspect"], s["bit_rate"], s["vbv"], s["video_format"]) == (2, 1, 10000, 0, 1)
    assert (s["colour_primaries"], s["transfer_characteristics"], s["matrix_coefficients"]) == (5, 5, 5)
    assert s["display_size"] == (c96[2], c96[3]) and plain_decode.repeated_headers == 0
    assert M.decoder.sequence_headers(c96[0]) == (c96[2], c96[3], s)


@pytest.mark.parametrize("d", [EVERY_FIELD, D.desc(repeat_headers=1), D.desc(bit_rate_400=1 << 18, vbv_buffer_size_16k=1024),
                               D.desc(display_width=1, display_height=16383, video_format=0)],
                         ids=["every_field", "repeat_only", "extension_bits_only", "display_1x16383"])
def test_decoder_on_described_streams(plain_decode, c96, d):
    st, first, W, H = c96
    x = D.described(st, first, d)
    assert len(x) % 32 == 0 and (len(x) > len(st) or not d["repeat_headers"])
    got = M.decoder.decode(x)
    assert same_planes(got, plain_decode) and (got.width, got.height) == (W, H)
    s = got.sequence
    assert (s["frame_rate_code"], s["aspect"], s["bit_rate"], s["vbv"], s["video_format"]) == (
        d["frame_rate_code"], d["aspect_ratio_information"], d["bit_rate_400"], d["vbv_buffer_size_16k"], d["video_format"])
    assert (s["colour_primaries"], s["transfer_characteristics"], s["matrix_coefficients"]) == (
        d["colour_primaries"], d["transfer_characteristics"], d["matrix_coefficients"])
    assert s["display_size"] == ((d["display_width"], d["display_height"]) if d["display_width"] else (W, H))
    assert got.repeated_headers == (len(first) - 1 if d["repeat_headers"] else 0)
    F = D.RATE[d["frame_rate_code"]]
    assert [(g["hours"], g["minutes"], g["seconds"], g["pictures"]) for g in got.gops] == [(0, 0, n // F, n % F) for n in first]
    assert [p["type"] for p in got.pictures] == [p["type"] for p in plain_decode.pictures]


def test_decoder_rejects_a_repeated_header_that_differs(c96):
    st, first, W, H = c96
    x = bytearray(D.described(st, first, D.desc(repeat_headers=1)))
    at = bytes(x).find(D.SEQ_CODE, 4)
    assert at > 0 and x[at + 34:at + 38] == G.GOP_CODE
    x[at + 27] = 1                                                            # colour_primaries of the second copy: 5 -> 1
    with pytest.raises(AssertionError, match="differs from the first"):
        M.decoder.decode(bytes(x))
    # ... and one that stands in front of a picture, not a GOP
    head, gops = G.cut(st)
    k = gops[0].find(b"\x00\x00\x01\x00", 16)                                 # the first P picture's header
    assert k > 0
    y = G.finish(head + gops[0][:k] + head + gops[0][k:] + b"".join(gops[1:]))
    with pytest.raises(AssertionError, match="GOP header"):
        M.decoder.decode(y)


# ---- the container scan and the multiplexers ----
def test_scan_opens_the_gop_at_the_repeated_header(c96):
    st, first, W, H = c96
    C = M.container
    info0, pics0 = C.scan(st)
    x = D.described(st, first, D.desc(repeat_headers=1))
    info, pics = C.scan(x)
    assert (info.pictures, info.gops, info.i_pictures, info.slices) == (info0.pictures, info0.gops, info0.i_pictures, info0.slices)
    assert info.bytes == info0.bytes + 34 * (len(first) - 1)
    later = 0                                                                 # repeated headers in front of the picture
    for k, (p, q) in enumerate(zip(pics, pics0)):
        opens = k in first and k > 0
        later += 34 if opens else 0
        assert p.offset == q.offset + later - (34 if opens else 0), k
        assert p.bytes == q.bytes + (34 if opens else 0), k                   # the header travels with the I picture it precedes ...
        assert (p.gop_start, p.coding_type, p.temporal_reference, p.slices) == (q.gop_start, q.coding_type, q.temporal_reference, q.slices)
        assert x[p.offset:p.offset + 4] == (D.SEQ_CODE if opens else G.GOP_CODE if k == 0 else b"\x00\x00\x01\x00"), k
    assert pics[2].bytes == pics0[2].bytes                                    # ... and not with the last P picture of the GOP before
    assert sum(p.bytes for p in pics) + 34 + 4 == info.bytes


@pytest.mark.parametrize("code,step", [(2, 3750), (3, 3600), (5, 3000), (6, 1800)])
def test_ps_pts_follow_the_frame_rate_code(c96, code, step):
    import test_container as TC
    st, first, W, H = c96
    C = M.container
    x = D.described(st, first, D.desc(frame_rate_code=code, repeat_headers=1))
    info, pics = C.scan(x)
    assert info.frame_rate_code == code
    got, stamps, scrs, rate = TC.demux_ps(C.mux_ps(x))
    assert got == x[:info.bytes] and len(stamps) == len(pics)
    for k, ((off, pts), pic) in enumerate(zip(stamps, pics)):
        assert off == (0 if k == 0 else pic.offset), k
        assert pts - stamps[0][1] == k * step, k
        # the PES packet that carries a repeated sequence header is the I picture's
        assert x[off:off + 4] == (D.SEQ_CODE if k in first else b"\x00\x00\x01\x00"), k


def test_ts_carries_the_repeated_header_with_its_i_picture(c96):
    import test_container as TC
    st, first, W, H = c96
    C = M.container
    x = D.described(st, first, D.desc(frame_rate_code=3, repeat_headers=1))
    info, pics = C.scan(x)
    got, pts, pcrs, pcr_pos = TC.demux_ts(C.mux_ts(x))
    assert got == x[:info.bytes] and len(pts) == len(pics)
    assert [t - pts[0] for t in pts] == [3600 * k for k in range(len(pics))]
