"""-m gpu: GOP starts from the caller's list (m2v_set_gop_starts) against tests/scene_cases.py: every stream is byte for byte the splice
of the oracle's streams of each GOP encoded alone (time code patched), every record of m2v_scene_report the rule's flags.  No
tolerance anywhere.  tests/test_scene_cases.py shows what the cases reach.  Nothing is larger than 96 x 64 or longer than 12 frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4


@pytest.fixture(scope="module")
def env():
    import gop_cases
    import scene_cases
    return gop_cases.M, gop_cases, scene_cases


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
    elif kind == "rgb24":
        nb = enc.encode_resident_rgb(*a, kind)
    else:
        nb = enc.encode_resident420(*a, kind)
    return d_out[:nb].cpu().numpy().tobytes()


def encoder(M, Q=2, VL=3, options=(), starts=None, levels=None):
    enc = M.Mpeg2Encoder(6, 6, VL, Q)
    for k, v in options:
        enc.set_option(k, v)
    if starts is not None:
        enc.set_gop_starts(starts)
    if levels is not None:
        enc.set_gop_levels(levels)
    return enc


def same_records(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


# ---- the list, resident ----
@pytest.mark.parametrize("name,pf,starts,vl", [("c96", 3, [5], 3), ("c96", 255, [1, 2, 3], 3), ("c64", 0, [2, 4], 3), ("c96", 3, [5], 1)],
                         ids=["one_picture_gop", "pf255", "pf0", "vl1"])
def test_list_resident(env, name, pf, starts, vl):
    """[5] against GOPs of 4: GOPs at 0, 4, 5, 9 - a one-picture GOP, and a cadence that starts again behind the forced start"""
    M, G, S = env
    f, W, H = G.clip_args(name)
    enc = encoder(M, VL=vl, starts=starts)
    try:
        got = resident(enc, f, W, H, pf)
        assert got == S.expected(f, W, H, pf, starts, VL=vl)
        d = M.decoder.decode(got)
        assert [p["type"] for p in d.pictures] == [1 if x else 2 for x in S.layout(len(f), pf, starts)]
        same_records(enc.scene_report(), S.records(len(f), pf, starts))
    finally:
        enc.close()


def test_list_of_cadence_positions_changes_nothing(env):
    """[0, 3, 6, 100] at GOPs of 3: 0, cadence positions and an entry past the end - the bytes of a handle with no list"""
    M, G, S = env
    f, W, H = G.clip_args("c80")
    plain = G.encoded(f, W, H, 2, 2)[0]
    enc, none = encoder(M, starts=[0, 3, 6, 100]), encoder(M)
    try:
        got = resident(enc, f, W, H, 2)
        assert got == plain == resident(none, f, W, H, 2) == S.expected(f, W, H, 2, [0, 3, 6, 100])
        same_records(enc.scene_report(), S.records(len(f), 2, [0, 3, 6, 100]))
        assert len(none.scene_report()) == 0
    finally:
        enc.close()
        none.close()


# ---- the same stream however the sequence is chunked or submitted ----
@pytest.mark.parametrize("options", [(("batch_frames", 1),), (("batch_frames", 3),), (("batch_frames", 5),), (("batch_frames", 96),),
                                     (("split_streams", 1),), (("split_streams", 2),), (("profile", 1),)], ids=lambda o: "%s%d" % o[0])
def test_list_launch_shapes(env, options):
    M, G, S = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, options=options, starts=[5])
    try:
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5])
        same_records(enc.scene_report(), S.records(len(f), 3, [5]))
    finally:
        enc.close()


def test_list_begin_end(env):
    import torch
    M, G, S = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, starts=[5])
    try:
        for _ in range(2):
            d_in, d_out = resident(enc, f, W, H, 3, begin=True)
            nb = enc.encode_resident_end()
            assert d_out[:nb].cpu().numpy().tobytes() == S.expected(f, W, H, 3, [5])
            same_records(enc.scene_report(), S.records(len(f), 3, [5]))
        torch.cuda.synchronize()
    finally:
        enc.close()


@pytest.mark.parametrize("async_", [1, 0])
def test_list_port_path(env, async_):
    """push_frames in calls of 1, 5 and 6 frames, chunks of 3 frames against GOPs at 0, 4, 5, 9, pulled to `last`"""
    M, G, S = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, options=(("batch_frames", 3), ("async", async_)), starts=[5])
    try:
        out = []
        for a, b in ((0, 1), (1, 6), (6, 12)):
            enc.push_frames(W // 16, H // 16, 3, f[a:b])
            out.append(enc.pull()[0])
        enc.sequence_stop()
        out.append(enc.pull_all())
        assert b"".join(out) == S.expected(f, W, H, 3, [5])
        same_records(enc.scene_report(), S.records(len(f), 3, [5]))
    finally:
        enc.close()


# ---- other inputs ----
def test_list_i420(env):
    M, G, S = env
    f, W, H = G.clip_args("c80")
    x = M.to420(f, "i420")
    planes = M.to444(x, W, H, "i420")
    enc = encoder(M, starts=[4])
    try:
        assert resident(enc, x, W, H, 2, "i420") == S.expected(planes, W, H, 2, [4])
    finally:
        enc.close()


@pytest.mark.parametrize("header", ["module", "true"])
def test_list_rgb24_padded(env, header):
    """72 x 60 RGB frames, padded to 80 x 64 and converted on the device"""
    import fit_cases as F
    M, G, S = env
    w, h, n, pf = 72, 60, 8, 2
    x = F.source(w, h, n, "rgb24", seed=5)
    planes = F.planes(x, w, h, "rgb24")
    assert np.array_equal(planes, M.rgb_to444(M.pad_frames(x, w, h, "rgb24"), 80, 64, "rgb24", "bt601").reshape(planes.shape))
    want = S.expected(planes, 80, 64, pf, [4])
    if header == "true":
        want = M.set_header_size(want, w, h)
    enc = encoder(M, starts=[4])
    try:
        enc.set_frame_size(w, h, header)
        assert resident(enc, x, w, h, pf, "rgb24") == want
        same_records(enc.scene_report(), S.records(n, pf, [4]))
    finally:
        enc.close()


# ---- with a level schedule: by GOP ordinal ----
def test_list_with_a_level_schedule(env):
    """GOPs at 0, 4, 5, 9 with [1, 4, 3]: levels 1, 4, 3, 3"""
    M, G, S = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, starts=[5], levels=[1, 4, 3])
    try:
        got = resident(enc, f, W, H, 3)
        assert got == S.expected(f, W, H, 3, [5], levels=[1, 4, 3])
        lv = [1] * 4 + [4] + [3] * 4 + [3] * 3
        assert M.decoder.decode(got).slice_qcodes == [[1 << q] * (H // 16) for q in lv]
    finally:
        enc.close()


# ---- with "stats" ----
@pytest.mark.parametrize("options", [(), (("batch_frames", 3),)], ids=["one_chunk", "chunks_of_3"])
def test_list_with_stats(env, options):
    import stats_cases as P
    M, G, S = env
    f, W, H = G.clip_args("c96")
    fl = S.layout(len(f), 3, [5])
    want = np.zeros(len(f), P.DTYPE)
    for s, L in S.gops(len(f), 3, [5]):
        want[s:s + L] = P.records(G.encoded(f[s:s + L], W, H, 3, 2)[1], W, H, 3)
    want["frame"] = np.arange(len(f))
    assert want["coding_type"].tolist() == [1 if x else 2 for x in fl]
    enc = encoder(M, options=options + (("stats", 1),), starts=[5])
    try:
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5])
        got = enc.picture_stats()
        for k in want.dtype.names:
            assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    finally:
        enc.close()


# ---- state and refusals ----
def test_setting_survives_reset_and_is_cleared(env):
    M, G, S = env
    f, W, H = G.clip_args("c96")
    plain = G.encoded(f, W, H, 3, 2)[0]
    enc = encoder(M, starts=[5])
    try:
        enc.reset()
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5])
        assert len(enc.scene_report()) == len(f)
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5])
        enc.reset()
        assert len(enc.scene_report()) == 0               # dropped at m2v_reset
        enc.set_gop_starts([])
        assert resident(enc, f, W, H, 3) == plain
        assert len(enc.scene_report()) == 0               # a sequence without list or detector leaves none
        enc.set_gop_starts([5])
        enc.set_gop_starts(None)
        assert resident(enc, f, W, H, 3) == plain
    finally:
        enc.close()


def test_refusals(env):
    import torch
    M, G, S = env
    f, W, H = G.clip_args("c96")
    xs, ys = W // 16, H // 16
    enc = encoder(M, starts=[5])
    try:
        L, hd = enc._L, enc._h
        # a descending list, a repeated entry: M2V_E_PARAM, and the previous setting stays
        for bad in ([7, 3], [3, 3], [1, 5, 5, 9]):
            with pytest.raises(M.M2VError, match=r"\(-1\)"):
                enc.set_gop_starts(bad)
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5])
        d = dev(f.reshape(len(f), -1))
        out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        # strips with a list
        assert L.m2v_strip_begin(hd, xs, ys, 3, d.data_ptr(), len(f), 0, ys, None) == E_STATE
        assert b"m2v_set_gop_starts" in L.m2v_last_error(hd)
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            enc.strip_encode(None, 0, 1, d.data_ptr(), len(f), xs, ys, 3, out.data_ptr(), out.numel())
        # the cap together with a list: nothing starts
        enc.set_option("gop_bytes_max", 3000)
        with pytest.raises(M.M2VError, match=r"\(-4\).*gop_bytes_max"):
            resident(enc, f, W, H, 3)
        assert not enc.busy
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            resident(enc, f, W, H, 3, begin=True)
        assert not enc.busy
        enc.set_option("gop_bytes_max", 0)
        # the handle is as usable as ever
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5])
        enc.set_gop_starts(None)
        nb = enc.strip_encode(None, 0, 1, d.data_ptr(), len(f), xs, ys, 3, out.data_ptr(), out.numel())
        assert out[:nb].cpu().numpy().tobytes() == G.encoded(f, W, H, 3, 2)[0]
    finally:
        enc.close()


# ---- the report ----
def test_report_pops_oldest_first(env):
    M, G, S = env
    f, W, H = G.clip_args("c96")
    want = S.records(len(f), 3, [5])
    assert want["flags"].tolist() == [1, 0, 0, 0, 2, 4, 0, 0, 0, 2, 0, 0] and not want["diff"].any()
    enc = encoder(M, starts=[5])
    try:
        resident(enc, f, W, H, 3)
        assert enc._L.m2v_scene_report(enc._h, None, 0) == len(f)
        same_records(enc.scene_report(5), want[:5])
        same_records(enc.scene_report(), want[5:])
        assert len(enc.scene_report()) == 0
        enc.set_gop_starts(None)
        resident(enc, f, W, H, 3)
        assert enc._L.m2v_scene_report(enc._h, None, 0) == 0
    finally:
        enc.close()


def test_encode_tensor_gop_starts(env):
    """encode_tensor(gop_starts=...) on a planar RGB tensor; the handle's own setting (none) is back afterwards"""
    M, G, S = env
    f, W, H = G.clip_args("c96")
    planes = M.rgb_to444(f, W, H, "rgbp", "bt601")
    enc = encoder(M)
    try:
        t = dev(np.ascontiguousarray(f))
        assert enc.encode_tensor(t, 3, gop_starts=[5]).cpu().numpy().tobytes() == S.expected(planes, W, H, 3, [5])
        same_records(enc.scene_report(), S.records(len(f), 3, [5]))
        assert enc.encode_tensor(t, 3).cpu().numpy().tobytes() == G.encoded(planes, W, H, 3, 2)[0]
    finally:
        enc.close()


def test_tb_istart_and_scenecut(env, tmp_path):
    """m2v_tb -istart 5 (the port path) and -scenecut 3000 (the file staged in device memory, one resident call); a bad list is refused"""
    import os
    import subprocess
    M, G, S = env
    tb = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "m2v_tb")
    f, W, H = G.clip_args("c96")
    (tmp_path / "c96.yuv").write_bytes(f.tobytes())
    args = [str(tmp_path / "c96.yuv"), str(W), str(H), str(tmp_path / "c96.m2v")]
    head = [tb, "-XL", "6", "-YL", "6"]
    out = subprocess.run(head + ["-p", "3", "-istart", "5"] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "c96.m2v").read_bytes() == S.expected(f, W, H, 3, [5])
    out = subprocess.run(head + ["-p", "7", "-scenecut", "3000"] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "c96.m2v").read_bytes() == S.expected(f, W, H, 7, [4, 8])
    bad = subprocess.run(head + ["-p", "3", "-istart", "9,5"] + args, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "m2v_set_gop_starts" in bad.stderr
