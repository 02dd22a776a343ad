"""-m gpu: option "scene_cut", the cut detector on the device (k_mbsum, k_scene_judge), against tests/scene_cases.py: D(n) of every
record is numpy's, exactly; every stream is the splice of the oracle's streams of the GOPs the definition gives.  No tolerance
anywhere.  Nothing is longer than 12 frames; nothing but the detector's own shapes is larger than 96 x 80."""
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


def resident(enc, x, W, H, pf, kind="444", begin=False, odd=False):
    """one sequence of the frames x [n, ...] through the resident entry of `kind`; begin=True: only the first half; odd=True: the
    frames start one byte into their allocation"""
    import torch
    n = x.shape[0]
    xs, ys = (W + 15) // 16, (H + 15) // 16
    flat = dev(x.reshape(-1))
    if odd:
        buf = torch.empty(flat.numel() + 1, dtype=torch.uint8, device="cuda:0")
        buf[1:].copy_(flat)
        flat = buf[1:]
        assert flat.data_ptr() % 2 == 1
    d_out = torch.empty(n * 3 * 256 * xs * ys * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (flat.data_ptr(), n, d_out.data_ptr(), d_out.numel(), xs, ys, pf)
    if begin:
        enc.encode_resident_begin(*a)
        return flat, d_out
    nb = enc.encode_resident(*a) if kind == "444" else enc.encode_resident420(*a, kind)
    return d_out[:nb].cpu().numpy().tobytes()


def encoder(M, T, XL=6, options=(), starts=None):
    enc = M.Mpeg2Encoder(XL, 6, 3, 2)
    for k, v in options:
        enc.set_option(k, v)
    enc.set_option("scene_cut", T)
    if starts is not None:
        enc.set_gop_starts(starts)
    return enc


def same_records(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


def noise(n, H, W, seed):
    """white noise in all three planes: every macroblock's sum is its own"""
    return np.random.default_rng(seed).integers(0, 256, (n, 3, H, W), dtype=np.uint8)


def flat_y(values, W=64, H=64):
    f = np.full((len(values), 3, H, W), 128, np.uint8)
    for k, v in enumerate(values):
        f[k, 0] = v
    return f


# ---- D(n) against numpy, shape by shape: mbw 4, 5, 6 (five rows), 17 (one lane past a 256-column unit), 21, 128 ----
T_NOISE = 1300      # (noise against noise gives D / mbs around 1330: both answers occur, and numpy says which)


@pytest.mark.parametrize("W,H,XL", [(64, 64, 6), (80, 64, 6), (96, 80, 6), (272, 64, 6), (336, 64, 6), (2048, 64, 7)])
def test_diff_shapes(env, W, H, XL):
    M, G, S = env
    f = noise(3, H, W, W + H)
    want = S.records(3, 2, None, S.cuts_of(f, T_NOISE), S.diffs(f))
    enc = encoder(M, T_NOISE, XL=XL)
    try:
        resident(enc, f, W, H, 2)
        same_records(enc.scene_report(), want, (W, H))
    finally:
        enc.close()


def test_diff_input_at_an_odd_address(env):
    M, G, S = env
    W, H = 336, 64
    f = noise(3, H, W, 77)
    want = S.records(3, 2, None, S.cuts_of(f, T_NOISE), S.diffs(f))
    enc = encoder(M, T_NOISE)
    try:
        resident(enc, f, W, H, 2, odd=True)
        same_records(enc.scene_report(), want)
    finally:
        enc.close()


def test_diff_i420(env):
    M, G, S = env
    f, W, H = G.clip_args("c80")
    x = M.to420(f, "i420")
    planes = M.to444(x, W, H, "i420")
    cuts = S.cuts_of(planes, 3000)
    enc = encoder(M, 3000)
    try:
        assert resident(enc, x, W, H, 7, "i420") == S.expected(planes, W, H, 7, None, cuts=cuts)
        same_records(enc.scene_report(), S.records(len(f), 7, None, cuts, S.diffs(planes)))
    finally:
        enc.close()


def test_diff_measures_the_padding(env):
    """70 x 50 frames padded to 80 x 64: S is of the picture as coded"""
    import fit_cases as F
    M, G, S = env
    w, h = 70, 50
    x = F.source(w, h, 3, "444", seed=9, noise=True)
    planes = F.planes(x, w, h, "444")
    assert planes.shape[2:] == (64, 80)
    inner = np.zeros_like(planes)
    inner[:, :, :h, :w] = planes[:, :, :h, :w]
    assert S.diffs(inner).tolist() != S.diffs(planes).tolist()
    enc = encoder(M, T_NOISE)
    try:
        enc.set_frame_size(w, h)
        resident(enc, x, w, h, 2)
        same_records(enc.scene_report(), S.records(3, 2, None, S.cuts_of(planes, T_NOISE), S.diffs(planes)))
    finally:
        enc.close()


# ---- extremes and the threshold's edge ----
def test_extremes(env):
    """Y all 0, all 255, all 0: D = 65280 * 16 twice.  T = 65280: no cut, the stream of a handle with the option off; 65279: cuts"""
    M, G, S = env
    f = flat_y([0, 255, 0])
    assert S.diffs(f).tolist() == [0, 65280 * 16, 65280 * 16]
    plain = G.encoded(f, 64, 64, 2, 2)[0]
    off = M.Mpeg2Encoder(6, 6, 3, 2)
    enc = encoder(M, 65280)
    try:
        got = resident(enc, f, 64, 64, 2)
        assert got == plain == resident(off, f, 64, 64, 2)
        same_records(enc.scene_report(), S.records(3, 2, None, (), S.diffs(f)))
        enc.set_option("scene_cut", 65279)
        assert resident(enc, f, 64, 64, 2) == S.expected(f, 64, 64, 2, None, cuts=[1, 2])
        same_records(enc.scene_report(), S.records(3, 2, None, [1, 2], S.diffs(f)))
    finally:
        enc.close()
        off.close()


def test_threshold_edge(env):
    """Y constant 100, then 110: D = 2560 * mbs exactly.  "More than T": 2560 does not cut, 2559 does"""
    M, G, S = env
    f = flat_y([100, 110])
    assert S.diffs(f).tolist() == [0, 2560 * 16]
    enc = encoder(M, 2560)
    try:
        assert resident(enc, f, 64, 64, 2) == G.encoded(f, 64, 64, 2, 2)[0]
        same_records(enc.scene_report(), S.records(2, 2, None, (), S.diffs(f)))
        enc.set_option("scene_cut", 2559)
        assert resident(enc, f, 64, 64, 2) == S.expected(f, 64, 64, 2, None, cuts=[1])
        same_records(enc.scene_report(), S.records(2, 2, None, [1], S.diffs(f)))
    finally:
        enc.close()


# ---- streams ----
@pytest.mark.parametrize("name", ["c64", "c80", "c96"])
def test_streams_cut_at_the_scene_changes(env, name):
    M, G, S = env
    f, W, H = G.clip_args(name)
    sl = G.CLIPS[name]["scene_len"]
    cuts = [n for n in range(1, len(f)) if n % sl == 0]
    want = S.records(len(f), 7, None, cuts, S.diffs(f))
    assert want["flags"].tolist() == [S.FIRST if n == 0 else S.CUT if n % sl == 0 else 0 for n in range(len(f))]
    enc = encoder(M, 3000)
    try:
        assert resident(enc, f, W, H, 7) == S.expected(f, W, H, 7, cuts)
        same_records(enc.scene_report(), want)
    finally:
        enc.close()


@pytest.mark.parametrize("options", [(("batch_frames", 4),), (("batch_frames", 3),), (("batch_frames", 1),), (("split_streams", 1),),
                                     (("batch_frames", 4), ("split_streams", 1)), (("profile", 1),)],
                         ids=["b4", "b3", "b1", "one_stream", "b4_one_stream", "profile"])
def test_chunk_boundaries(env, options):
    """c96 cuts at 4 and 8: with chunks of 4 each cut is a chunk's first frame and its D crosses the carry"""
    M, G, S = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, 3000, options=options)
    try:
        assert resident(enc, f, W, H, 7) == S.expected(f, W, H, 7, [4, 8])
        same_records(enc.scene_report(), S.records(len(f), 7, None, [4, 8], S.diffs(f)))
        if options[0][0] == "profile":
            assert enc._L.m2v_kernel_stats(enc._h, 5, None, None) == 1          # k_mbsum + k_scene_judge: one timed interval per chunk
    finally:
        enc.close()


def test_cut_and_list_together(env):
    """pf 3, T = 3000, [5]: frame 4 is CADENCE | CUT, 5 LIST, 8 CUT alone (three frames behind the I picture at 5)"""
    M, G, S = env
    f, W, H = G.clip_args("c96")
    want = S.records(len(f), 3, [5], [4, 8], S.diffs(f))
    assert want["flags"].tolist() == [1, 0, 0, 0, 10, 4, 0, 0, 8, 0, 0, 0]
    enc = encoder(M, 3000, starts=[5])
    try:
        assert resident(enc, f, W, H, 3) == S.expected(f, W, H, 3, [5], cuts=[4, 8])
        same_records(enc.scene_report(), want)
    finally:
        enc.close()


def test_begin_end_and_two_sequences_in_a_row(env):
    """_begin / _end with the option on; then a second sequence that starts in another scene: its frame 0 has D = 0, nothing of the
    first sequence's last frame comes through the carry"""
    import torch
    M, G, S = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, 3000, options=(("batch_frames", 5),))
    try:
        keep = resident(enc, f[:7], W, H, 7, begin=True)
        nb = enc.encode_resident_end()
        assert keep[1][:nb].cpu().numpy().tobytes() == S.expected(f[:7], W, H, 7, [4])
        same_records(enc.scene_report(), S.records(7, 7, None, [4], S.diffs(f[:7])))
        g = f[8:]
        assert S.diffs(g)[0] == 0 and np.abs(S.mb_sums(g[:1]) - S.mb_sums(f[6:7])).sum() > 3000 * (W // 16) * (H // 16)
        assert resident(enc, g, W, H, 7) == S.expected(g, W, H, 7, None)
        same_records(enc.scene_report(), S.records(len(g), 7, None, (), S.diffs(g)))
        torch.cuda.synchronize()
    finally:
        enc.close()


def test_encode_tensor_scene_cut(env):
    M, G, S = env
    f, W, H = G.clip_args("c96")
    planes = M.rgb_to444(f, W, H, "rgbp", "bt601")
    cuts = S.cuts_of(planes, 3000)
    enc = M.Mpeg2Encoder(6, 6, 3, 2)
    try:
        t = dev(np.ascontiguousarray(f))
        assert enc.encode_tensor(t, 7, scene_cut=3000).cpu().numpy().tobytes() == S.expected(planes, W, H, 7, None, cuts=cuts)
        same_records(enc.scene_report(), S.records(len(f), 7, None, cuts, S.diffs(planes)))
        assert enc.encode_tensor(t, 7).cpu().numpy().tobytes() == G.encoded(planes, W, H, 7, 2)[0]
        assert len(enc.scene_report()) == 0
    finally:
        enc.close()


# ---- refusals ----
def test_refusals(env):
    import torch
    M, G, S = env
    f, W, H = G.clip_args("c96")
    xs, ys = W // 16, H // 16
    enc = encoder(M, 3000)
    try:
        L, hd = enc._L, enc._h
        with pytest.raises(M.M2VError, match=r"\(-4\).*scene_cut"):
            enc.push_frames(xs, ys, 3, f[:1])
        y = np.zeros(16, np.uint8)
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            enc.push_beats(xs, ys, 3, y, y, y)
        assert not enc.busy
        for bad in (65281, -1, 1 << 40):
            assert L.m2v_set_option(hd, b"scene_cut", bad) == E_PARAM
        d = dev(f.reshape(len(f), -1))
        assert L.m2v_strip_begin(hd, xs, ys, 3, d.data_ptr(), len(f), 0, ys, None) == E_STATE
        enc.set_option("gop_bytes_max", 3000)
        with pytest.raises(M.M2VError, match=r"\(-4\).*gop_bytes_max"):
            resident(enc, f, W, H, 3)
        assert not enc.busy
        enc.set_option("gop_bytes_max", 0)
        # between _begin and _end
        keep = resident(enc, f, W, H, 7, begin=True)
        assert L.m2v_set_option(hd, b"scene_cut", 0) == E_STATE
        nb = enc.encode_resident_end()
        assert keep[1][:nb].cpu().numpy().tobytes() == S.expected(f, W, H, 7, [4, 8])
        # ... and during a port sequence (the option off, so that one starts)
        enc.set_option("scene_cut", 0)
        enc.push_frames(xs, ys, 3, f[:1])
        assert L.m2v_set_option(hd, b"scene_cut", 3000) == E_STATE
        enc.reset()
        # the handle is as usable as ever
        assert enc.encode(f, xs, ys, 3) == G.encoded(f, W, H, 3, 2)[0]
        enc.set_option("scene_cut", 3000)
        assert resident(enc, f, W, H, 7) == S.expected(f, W, H, 7, [4, 8])
        torch.cuda.synchronize()
    finally:
        enc.close()
