"""-m gpu: the stream description (m2v_set_stream_desc) against tests/desc_cases.py: every stream is byte for byte an expected stream
that gop_cases / scene_cases build from the oracle, with the sequence headers written from the ISO field widths, every GOP's time code
counted at the description's frame rate and, with repeat_headers, the headers again in front of every later GOP.  No tolerance
anywhere.  tests/test_desc_cases.py holds the helper against the oracle.  Nothing is longer than 62 frames; the largest picture is the
100 x 70 one of the frame-size case (112 x 80 coded), every other one at most 96 x 64."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4


@pytest.fixture(scope="module")
def env():
    import desc_cases
    import gop_cases
    import scene_cases
    return gop_cases.M, gop_cases, scene_cases, desc_cases


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def resident(enc, x, W, H, pf, kind="444", begin=False):
    """one sequence of the frames x [n, ...] through the resident entry of `kind`; begin=True: only the first half"""
    import torch
    n = x.shape[0]
    xs, ys = (W + 15) // 16, (H + 15) // 16
    d_in = dev(x.reshape(n, -1))
    d_out = torch.empty(n * 3 * 256 * xs * ys * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), xs, ys, pf)
    if begin:
        enc.encode_resident_begin(*a)
        return d_in, d_out
    if kind == "444":
        nb = enc.encode_resident(*a)
    else:
        nb = enc.encode_resident420(*a, kind)
    return d_out[:nb].cpu().numpy().tobytes()


def encoder(M, D, d=None, Q=2, options=(), starts=None, levels=None):
    enc = M.Mpeg2Encoder(6, 6, 3, Q)
    for k, v in options:
        enc.set_option(k, v)
    if starts is not None:
        enc.set_gop_starts(starts)
    if levels is not None:
        enc.set_gop_levels(levels)
    if d is not None:
        enc.set_stream_desc(D.struct(d))
    return enc


def same_records(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


def c96_pf2(G, D):
    """(frames, W, H, the plain oracle stream at pframes_count 2, the first frames of its four GOPs)"""
    f, W, H = G.clip_args("c96")
    return f, W, H, G.encoded(f, W, H, 2, 2)[0], D.cadence(len(f), 2)


# ---- 1. the module's description, and clearing a setting ----
def test_module_description_and_clearing(env):
    M, G, S, D = env
    f, W, H = G.clip_args("c80")
    plain = G.encoded(f, W, H, 2, 2)[0]
    other = D.desc(frame_rate_code=3, colour_primaries=1, repeat_headers=1)
    enc = encoder(M, D, D.MODULE)
    try:
        assert resident(enc, f, W, H, 2) == plain
        assert enc.encode(f, W // 16, H // 16, 2) == plain                    # the port path
        enc.set_stream_desc(M.stream_desc())
        assert resident(enc, f, W, H, 2) == plain
        enc.set_stream_desc(D.struct(other))
        want = D.described(plain, D.cadence(len(f), 2), other)
        assert want != plain and resident(enc, f, W, H, 2) == want
        assert enc.encode(f, W // 16, H // 16, 2) == want
        enc.reset()                                                           # the setting survives m2v_reset
        assert resident(enc, f, W, H, 2) == want
        enc.set_stream_desc(None)
        assert resident(enc, f, W, H, 2) == plain
        assert enc.encode(f, W // 16, H // 16, 2) == plain
    finally:
        enc.close()


# ---- 2. every field alone at a non-module value, and the extremes ----
ALONE = [dict(bit_rate_400=1), dict(bit_rate_400=1 << 18), dict(bit_rate_400=(1 << 30) - 1),
         dict(vbv_buffer_size_16k=1023), dict(vbv_buffer_size_16k=1024), dict(vbv_buffer_size_16k=(1 << 18) - 1),
         dict(aspect_ratio_information=4), dict(video_format=0), dict(video_format=5),
         dict(colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1),
         dict(colour_primaries=255, transfer_characteristics=255, matrix_coefficients=255),
         dict(colour_primaries=9), dict(transfer_characteristics=16), dict(matrix_coefficients=9),
         dict(display_width=16383, display_height=1), dict(display_width=1, display_height=16383)]


def test_every_field_alone(env):
    M, G, S, D = env
    f, W, H = G.clip_args("c80")
    plain = G.encoded(f, W, H, 2, 2)[0]
    first = D.cadence(len(f), 2)
    enc = encoder(M, D)
    try:
        for fields in ALONE:
            d = D.desc(**fields)
            enc.set_stream_desc(D.struct(d))
            got = resident(enc, f, W, H, 2)
            assert got == D.described(plain, first, d), fields
            assert got[34:] == plain[34:] and got[:34] != plain[:34], fields  # nothing but the head differs
    finally:
        enc.close()


# ---- 3. the frame-rate codes: 62 time codes across the second's rollover at every F ----
@pytest.mark.parametrize("repeat", [0, 1], ids=["once", "repeat_headers"])
def test_frame_rate_codes(env, repeat):
    """62 GOPs of one picture; with repeat_headers 61 more copies of the headers"""
    M, G, S, D = env
    f, W, H = D.ionly()
    plain = G.encoded(f, W, H, 0, 2)[0]
    first = D.cadence(len(f), 0)
    assert len(first) == 62
    enc = encoder(M, D)
    try:
        for code in range(1, 9) if not repeat else (3, 8):
            d = D.desc(frame_rate_code=code, repeat_headers=repeat)
            enc.set_stream_desc(D.struct(d))
            got = resident(enc, f, W, H, 0)
            assert got == D.described(plain, first, d), code
            assert len(got) >= len(plain) + repeat * 34 * 61 - 31
    finally:
        enc.close()


# ---- 4. repeat_headers, however the sequence is chunked or submitted ----
@pytest.mark.parametrize("options", [(("batch_frames", 3),), (("batch_frames", 4),), (("batch_frames", 1),), (("batch_frames", 96),),
                                     (("split_streams", 1),), (("profile", 1),)], ids=lambda o: "%s%d" % o[0])
def test_repeat_launch_shapes(env, options):
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    d = D.desc(repeat_headers=1)
    want = D.described(plain, first, d)
    assert want.count(D.SEQ_CODE) == 4 and len(want) > len(plain)
    enc = encoder(M, D, d, options=options)
    try:
        assert resident(enc, f, W, H, 2) == want
        assert M.decoder.decode(want).repeated_headers == 3
    finally:
        enc.close()


@pytest.mark.parametrize("async_", [1, 0])
def test_repeat_port_path_frame_by_frame(env, async_):
    """a pull after every push, chunks of 4 frames against GOPs of 3: a GOP's repeated header opens a chunk, or stands inside one"""
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    d = D.desc(repeat_headers=1, frame_rate_code=6)
    enc = encoder(M, D, d, options=(("batch_frames", 4), ("async", async_)))
    try:
        out = []
        for k in range(len(f)):
            enc.push_frames(W // 16, H // 16, 2, f[k:k + 1])
            out.append(enc.pull()[0])
        enc.sequence_stop()
        out.append(enc.pull_all())
        assert b"".join(out) == D.described(plain, first, d)
    finally:
        enc.close()


# ---- 5. with the other features, repeat_headers on ----
REPEAT = dict(repeat_headers=1, frame_rate_code=5, colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1)


def test_with_list_and_scene_cut(env):
    """[5] and "scene_cut" 3000 at pframes_count 3: GOPs start at 0, 4, 5, 8 - cadence | cut, list, cut"""
    M, G, S, D = env
    f, W, H = G.clip_args("c96")
    d = D.desc(**REPEAT)
    want = S.expected(f, W, H, 3, [5], cuts=[4, 8])
    assert [s for s, _ in S.gops(len(f), 3, [5], [4, 8])] == [0, 4, 5, 8]
    enc = encoder(M, D, d, options=(("scene_cut", 3000),), starts=[5])
    try:
        assert resident(enc, f, W, H, 3) == D.described(want, [0, 4, 5, 8], d)
        same_records(enc.scene_report(), S.records(len(f), 3, [5], [4, 8], S.diffs(f)))
    finally:
        enc.close()


def test_with_a_level_schedule(env):
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    d = D.desc(**REPEAT)
    enc = encoder(M, D, d, levels=G.SCHEDULE)
    try:
        assert resident(enc, f, W, H, 2) == D.described(G.splice(f, W, H, 2, G.SCHEDULE), first, d)
    finally:
        enc.close()


def test_with_the_cap(env):
    """the cap's records - GOP sizes, levels, verdicts - do not count the repeated headers"""
    M, G, S, D = env
    c = G.cap_case("b3500")
    d = D.desc(**REPEAT)
    enc = encoder(M, D, d, Q=c["Q"], options=(("gop_bytes_max", c["B"]),))
    try:
        got = resident(enc, c["frames"], c["W"], c["H"], c["pf"])
        same_records(enc.gop_report(), c["records"])
        assert got == D.described(c["stream"], D.cadence(len(c["frames"]), c["pf"]), d)
    finally:
        enc.close()


def test_with_stats(env):
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    d = D.desc(**REPEAT)
    enc = encoder(M, D, options=(("stats", 1),))
    try:
        assert resident(enc, f, W, H, 2) == plain
        without = enc.picture_stats()
        enc.set_stream_desc(D.struct(d))
        assert resident(enc, f, W, H, 2) == D.described(plain, first, d)
        same_records(enc.picture_stats(), without)
        assert len(without) == len(f) and without["mb_bits"].all()
    finally:
        enc.close()


def test_with_recon_out(env):
    import torch
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    d = D.desc(**REPEAT)
    nbytes = len(f) * M.frame_bytes(W, H, "i420")
    a, b = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    enc = encoder(M, D)
    try:
        enc.set_recon_out(a.data_ptr(), nbytes, "i420")
        assert resident(enc, f, W, H, 2) == plain
        enc.set_recon_out(b.data_ptr(), nbytes, "i420")
        enc.set_stream_desc(D.struct(d))
        assert resident(enc, f, W, H, 2) == D.described(plain, first, d)
        assert torch.equal(a, b) and bool(a.any())
        enc.set_recon_out(None, 0)
    finally:
        enc.close()


@pytest.mark.parametrize("display", [(0, 0), (96, 64)], ids=["display_follows", "display_given"])
def test_with_a_true_size_header(env, display):
    """100 x 70 frames, padded to 112 x 80, M2V_HEADER_TRUE: a display size of 0 follows the printed 100 x 70, a given one is printed"""
    import fit_cases as F
    M, G, S, D = env
    w, h, n, pf = 100, 70, 5, 2
    x = F.source(w, h, n, "444", seed=9)
    want = M.set_header_size(G.encoded(F.planes(x, w, h, "444"), 112, 80, pf, 2)[0], w, h)
    d = D.desc(display_width=display[0], display_height=display[1], **REPEAT)
    enc = encoder(M, D, d)
    try:
        enc.set_frame_size(w, h, "true")
        got = resident(enc, x, w, h, pf)
        assert got == D.described(want, D.cadence(n, pf), d, size=(w, h))
        s = M.decoder.sequence_headers(got)
        assert s[:2] == (w, h) and s[2]["display_size"] == (display if display[0] else (w, h))
        assert got.count(D.SEQ_CODE + got[4:34]) == 2                         # the repeated copy: the same printed and display sizes
    finally:
        enc.close()


def test_with_i420_input(env):
    M, G, S, D = env
    f, W, H = G.clip_args("c80")
    x = M.to420(f, "i420")
    d = D.desc(**REPEAT)
    enc = encoder(M, D, d)
    try:
        want = D.described(G.encoded(M.to444(x, W, H, "i420"), W, H, 2, 2)[0], D.cadence(len(f), 2), d)
        assert resident(enc, x, W, H, 2, "i420") == want
    finally:
        enc.close()


def test_encode_tensor_desc(env):
    """encode_tensor(matrix="bt709", desc=...) on a planar RGB tensor: the label is the caller's; the handle's own setting is back afterwards"""
    M, G, S, D = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, D)
    try:
        t = dev(np.ascontiguousarray(f))
        got = enc.encode_tensor(t, 2, matrix="bt709", desc=M.stream_desc(fps=(30000, 1001), colour="bt709")).cpu().numpy().tobytes()
        d = D.desc(frame_rate_code=4, colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1)
        assert got == D.described(G.encoded(M.rgb_to444(f, W, H, "rgbp", "bt709"), W, H, 2, 2)[0], D.cadence(len(f), 2), d)
        assert enc.encode_tensor(t, 2).cpu().numpy().tobytes() == G.encoded(M.rgb_to444(f, W, H, "rgbp", "bt601"), W, H, 2, 2)[0]
        own = D.desc(repeat_headers=1)
        enc.set_stream_desc(D.struct(own))
        enc.encode_tensor(t, 2, desc=M.stream_desc(fps=25))
        want = D.described(G.encoded(M.rgb_to444(f, W, H, "rgbp", "bt601"), W, H, 2, 2)[0], D.cadence(len(f), 2), own)
        assert enc.encode_tensor(t, 2).cpu().numpy().tobytes() == want
    finally:
        enc.close()


# ---- 6. two handles ----
def test_begin_end_on_two_handles_taking_turns(env):
    import torch
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    da, db = D.desc(frame_rate_code=3, repeat_headers=1), D.desc(frame_rate_code=8, bit_rate_400=1 << 18, video_format=0)
    ea, eb = encoder(M, D, da), encoder(M, D, db)
    try:
        for _ in range(2):
            ka = resident(ea, f, W, H, 2, begin=True)
            kb = resident(eb, f, W, H, 2, begin=True)
            assert ea._L.m2v_set_stream_desc(ea._h, None) == E_STATE          # busy: the setting stays
            na, nb = ea.encode_resident_end(), eb.encode_resident_end()
            assert ka[1][:na].cpu().numpy().tobytes() == D.described(plain, first, da)
            assert kb[1][:nb].cpu().numpy().tobytes() == D.described(plain, first, db)
        torch.cuda.synchronize()
    finally:
        ea.close()
        eb.close()


# ---- 7. refusals ----
INVALID = [dict(frame_rate_code=0), dict(frame_rate_code=9), dict(aspect_ratio_information=0), dict(aspect_ratio_information=5),
           dict(bit_rate_400=0), dict(bit_rate_400=1 << 30), dict(vbv_buffer_size_16k=1 << 18), dict(video_format=6),
           dict(colour_primaries=0), dict(colour_primaries=256), dict(transfer_characteristics=0), dict(transfer_characteristics=256),
           dict(matrix_coefficients=0), dict(matrix_coefficients=256), dict(display_width=0, display_height=64),
           dict(display_width=96, display_height=0), dict(display_width=16384, display_height=64), dict(display_width=96, display_height=16384),
           dict(repeat_headers=2), dict(reserved=1)]


def test_refusals(env):
    import torch
    M, G, S, D = env
    f, W, H, plain, first = c96_pf2(G, D)
    xs, ys = W // 16, H // 16
    held = D.desc(frame_rate_code=3, repeat_headers=1)
    want = D.described(plain, first, held)
    enc = encoder(M, D, held)
    try:
        L, hd = enc._L, enc._h
        # each invalid value: M2V_E_PARAM, and the previous setting stays
        for fields in INVALID:
            bad = D.struct(dict(D.MODULE, **fields))
            assert L.m2v_set_stream_desc(hd, ctypes.byref(bad)) == E_PARAM, fields
            assert b"m2v_set_stream_desc" in L.m2v_last_error(hd)
        with pytest.raises(M.M2VError, match=r"\(-1\)"):
            enc.set_stream_desc(D.struct(D.desc(frame_rate_code=15)))
        assert resident(enc, f, W, H, 2) == want
        # between _begin and _end
        keep = resident(enc, f, W, H, 2, begin=True)
        module = M.stream_desc()
        assert L.m2v_set_stream_desc(hd, ctypes.byref(module)) == E_STATE and L.m2v_set_stream_desc(hd, None) == E_STATE
        assert keep[1][:enc.encode_resident_end()].cpu().numpy().tobytes() == want
        # during a port sequence
        enc.push_frames(xs, ys, 2, f[:4])
        assert L.m2v_set_stream_desc(hd, None) == E_STATE
        enc.push_frames(xs, ys, 2, f[4:])
        enc.sequence_stop()
        assert L.m2v_set_stream_desc(hd, None) == E_STATE                     # not pulled to `last` yet
        assert enc.pull_all() == want and not enc.busy
        # strips: refused with a description that differs from the module's ...
        d_in = dev(f.reshape(len(f), -1))
        out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        assert L.m2v_strip_begin(hd, xs, ys, 2, d_in.data_ptr(), len(f), 0, ys, None) == E_STATE
        assert b"m2v_set_stream_desc" in L.m2v_last_error(hd)
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            enc.strip_encode(None, 0, 1, d_in.data_ptr(), len(f), xs, ys, 2, out.data_ptr(), out.numel())
        assert resident(enc, f, W, H, 2) == want                              # the handle is as usable as ever
        # ... and as before with the module's, or none
        for d in (module, None):
            enc.set_stream_desc(d)
            nb = enc.strip_encode(None, 0, 1, d_in.data_ptr(), len(f), xs, ys, 2, out.data_ptr(), out.numel())
            assert out[:nb].cpu().numpy().tobytes() == plain
    finally:
        enc.close()


# ---- 8. m2v_tb ----
def test_tb_flags(env, tmp_path):
    """all six flags through the port path against the expected file; a bad -fps is refused with the usage text"""
    import os
    import subprocess
    M, G, S, D = env
    tb = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "m2v_tb")
    f, W, H, plain, first = c96_pf2(G, D)
    (tmp_path / "c96.yuv").write_bytes(f.tobytes())
    args = [str(tmp_path / "c96.yuv"), str(W), str(H), str(tmp_path / "c96.m2v")]
    head = [tb, "-XL", "6", "-YL", "6", "-p", "2"]
    flags = ["-fps", "30000/1001", "-aspect", "16:9", "-bitrate", "7999999", "-vbv", "112", "-colour", "1,13,6", "-repeat-headers"]
    out = subprocess.run(head + flags + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    d = D.desc(frame_rate_code=4, aspect_ratio_information=3, bit_rate_400=20000, vbv_buffer_size_16k=112, colour_primaries=1,
               transfer_characteristics=13, matrix_coefficients=6, repeat_headers=1)
    assert (tmp_path / "c96.m2v").read_bytes() == D.described(plain, first, d)
    bad = subprocess.run(head + ["-fps", "15/1"] + args, capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "usage" in bad.stderr and "-fps" in bad.stderr
