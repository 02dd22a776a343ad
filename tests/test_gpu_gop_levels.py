"""-m gpu: a level per GOP - the caller's schedule (m2v_set_gop_levels) and the byte cap the device holds (option "gop_bytes_max") -
against tests/gop_cases.py: every stream is byte for byte the splice of the oracle's streams at the GOPs' levels, every record of
m2v_gop_report the oracle's size at the level the rule picks.  No tolerance anywhere.  tests/test_gop_cases.py shows what the cases
reach.  Nothing is larger than 96 x 64 or longer than 12 frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4


@pytest.fixture(scope="module")
def env():
    import gop_cases
    return gop_cases.M, gop_cases


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
    nb = enc.encode_resident(*a) if kind == "444" else enc.encode_resident420(*a, kind)
    return d_out[:nb].cpu().numpy().tobytes()


def encoder(M, Q=2, VL=3, options=(), levels=None):
    enc = M.Mpeg2Encoder(6, 6, VL, Q)
    for k, v in options:
        enc.set_option(k, v)
    if levels is not None:
        enc.set_gop_levels(levels)
    return enc


def same_records(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


# ---- the schedule ----
@pytest.mark.parametrize("name,pf,n", [("c96", 2, 12), ("c64", 0, 7), ("c80", 2, 8)])
def test_schedule_resident(env, name, pf, n):
    """[1, 4, 3]: whole GOPs of 3, seven one-picture GOPs (the fourth and later ones at the last entry), and 8 frames whose last GOP
    is cut short"""
    M, G = env
    f, W, H = G.clip_args(name, n)
    enc = encoder(M, levels=G.SCHEDULE)
    try:
        got = resident(enc, f, W, H, pf)
        assert got == G.splice(f, W, H, pf, G.SCHEDULE)
        assert M.decoder.decode(got).slice_qcodes == G.expected_qcodes(n, H, pf, G.SCHEDULE)
    finally:
        enc.close()


@pytest.mark.parametrize("levels", [[1, 3], [4, 2, 1, 3, 2, 2]])
def test_schedule_shorter_and_longer_than_the_sequence(env, levels):
    """four GOPs: a schedule of two entries (the last one holds for the rest) and one of six (the entries past the last GOP are ignored)"""
    M, G = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, levels=levels)
    try:
        assert resident(enc, f, W, H, 2) == G.splice(f, W, H, 2, levels)
    finally:
        enc.close()


def test_schedule_equal_to_the_handles_level_and_cleared(env):
    """a schedule of the handle's own level is the plain stream - the oracle's, and the same handle's without a schedule -, and a
    schedule cleared again gives the plain stream again"""
    M, G = env
    f, W, H = G.clip_args("c96")
    plain = G.encoded(f, W, H, 2, 2)[0]
    enc = encoder(M, Q=2)
    try:
        none = resident(enc, f, W, H, 2)
        enc.set_gop_levels([2, 2])
        eq = resident(enc, f, W, H, 2)
        assert none == plain and eq == plain
        enc.set_gop_levels(G.SCHEDULE)
        assert resident(enc, f, W, H, 2) == G.splice(f, W, H, 2, G.SCHEDULE)
        enc.set_gop_levels(None)
        assert resident(enc, f, W, H, 2) == plain
        enc.set_gop_levels(G.SCHEDULE)
        enc.set_gop_levels([])
        assert resident(enc, f, W, H, 2) == plain
    finally:
        enc.close()


@pytest.mark.parametrize("vl", [1, 3])
def test_schedule_vector_levels(env, vl):
    M, G = env
    f, W, H = G.clip_args("c96", 9)
    enc = encoder(M, VL=vl, levels=G.SCHEDULE)
    try:
        assert resident(enc, f, W, H, 2) == G.splice(f, W, H, 2, G.SCHEDULE, VL=vl)
    finally:
        enc.close()


def test_schedule_conformant(env):
    M, G = env
    f, W, H = G.clip_args("c96", 9)
    enc = encoder(M, options=(("conformant", 1),), levels=G.SCHEDULE)
    try:
        assert resident(enc, f, W, H, 2) == G.splice(f, W, H, 2, G.SCHEDULE, conformant=True)
    finally:
        enc.close()


@pytest.mark.parametrize("options", [(("split_streams", 1),), (("split_streams", 2),), (("batch_frames", 3),), (("batch_frames", 4),),
                                     (("profile", 1),)], ids=lambda o: "%s%d" % o[0])
def test_schedule_launch_shapes(env, options):
    """12 frames in GOPs of 3: one and two group streams; chunks of one GOP; chunks of 4 frames, where a GOP straddles two chunks and
    keeps its level"""
    M, G = env
    f, W, H = G.clip_args("c96")
    levels = [1, 4, 3, 2]
    enc = encoder(M, options=options, levels=levels)
    try:
        assert resident(enc, f, W, H, 2) == G.splice(f, W, H, 2, levels)
    finally:
        enc.close()


def test_schedule_port_frame_by_frame(env):
    """the port path: one frame per m2v_push_frames call, chunks of 4 frames against GOPs of 3"""
    M, G = env
    f, W, H = G.clip_args("c96")
    enc = encoder(M, options=(("batch_frames", 4),), levels=G.SCHEDULE)
    try:
        out = []
        for k in range(len(f)):
            enc.push_frames(W // 16, H // 16, 2, f[k:k + 1])
            out.append(enc.pull()[0])
        enc.sequence_stop()
        out.append(enc.pull_all())
        assert b"".join(out) == G.splice(f, W, H, 2, G.SCHEDULE)
    finally:
        enc.close()


def test_schedule_port_stop_inside_a_frame(env):
    """beats, and the stop after 7 1/2 frames: the eighth frame is black-filled, and its GOP (the third) is at the third level"""
    M, G = env
    f, W, H = G.clip_args("c80")
    nbeats = 7 * (W * H // 4) + W * H // 8
    enc = encoder(M, levels=G.SCHEDULE)
    try:
        assert enc.encode(f, W // 16, H // 16, 2, nbeats=nbeats) == G.splice(f, W, H, 2, G.SCHEDULE, nbeats=nbeats)
    finally:
        enc.close()


def test_schedule_tb(env, tmp_path):
    """m2v_tb -qgop 1,4,3 (the port path), two videos back to back: the schedule starts again with every video; a bad list is refused"""
    import os
    import subprocess
    M, G = env
    tb = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "m2v_tb")
    args, want = [], []
    for name in ("c96", "c80"):
        f, W, H = G.clip_args(name)
        (tmp_path / (name + ".yuv")).write_bytes(f.tobytes())
        args += [str(tmp_path / (name + ".yuv")), str(W), str(H), str(tmp_path / (name + ".m2v"))]
        want.append(G.splice(f, W, H, 2, G.SCHEDULE))
    head = [tb, "-XL", "6", "-YL", "6", "-p", "2"]
    out = subprocess.run(head + ["-qgop", "1,4,3"] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [(tmp_path / (n + ".m2v")).read_bytes() for n in ("c96", "c80")] == want
    bad = subprocess.run(head + ["-qgop", "1,5"] + args, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "m2v_set_gop_levels" in bad.stderr


def test_schedule_encode_tensor_rgb_padded(env):
    """encode_tensor(gop_levels=...) on 100 x 70 RGB frames, padded on the device; the handle's own setting (none) is back afterwards"""
    import fit_cases as F
    import stats_cases as S
    M, G = env
    c = S.fit_case("fitrgb")
    planes = F.planes(c["x"], c["w"], c["h"], c["kind"])
    enc = encoder(M)
    try:
        t = dev(c["x"].reshape(c["n"], c["h"], c["w"], 3))
        got = enc.encode_tensor(t, 0, header="module", gop_levels=G.SCHEDULE).cpu().numpy().tobytes()
        assert got == G.splice(planes, c["W"], c["H"], 0, G.SCHEDULE)
        assert enc.encode_tensor(t, 0, header="module").cpu().numpy().tobytes() == G.encoded(planes, c["W"], c["H"], 0, 2)[0]
    finally:
        enc.close()


def test_schedule_i420_padded(env):
    import fit_cases as F
    import stats_cases as S
    M, G = env
    c = S.fit_case("fit420")
    planes = F.planes(c["x"], c["w"], c["h"], c["kind"])
    enc = encoder(M, levels=G.SCHEDULE)
    try:
        enc.set_frame_size(c["w"], c["h"])
        assert resident(enc, c["x"], c["w"], c["h"], 0, "i420") == G.splice(planes, c["W"], c["H"], 0, G.SCHEDULE)
    finally:
        enc.close()


# ---- the cap ----
def check_cap(M, G, name, options=()):
    c = G.cap_case(name)
    enc = encoder(M, Q=c["Q"], options=options + (("gop_bytes_max", c["B"]),), levels=c["sched"])
    try:
        got = resident(enc, c["frames"], c["W"], c["H"], c["pf"])
        assert enc._L.m2v_gop_report(enc._h, None, 0) == len(c["records"])
        rec = enc.gop_report()
        same_records(rec, c["records"], name)
        assert got == c["stream"], (name, options)
        assert M.decoder.decode(got).slice_qcodes == G.expected_qcodes(len(c["frames"]), c["H"], c["pf"], c["levels"])
        assert len(enc.gop_report()) == 0
        return got
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["b3500", "b3552", "b3551", "b800", "q4"])
def test_cap(env, name):
    check_cap(*env, name)


def test_cap_raises_a_schedules_start_levels(env):
    check_cap(*env, "sched")


@pytest.mark.parametrize("options", [(("batch_frames", 3),), (("split_streams", 1),), (("split_streams", 3), ("cu_pack", 0))],
                         ids=["chunk_per_gop", "one_stream", "three_streams"])
def test_cap_does_not_depend_on_the_launch_shape(env, options):
    """every GOP in a chunk of its own; one stream; three"""
    check_cap(*env, "b3500", options)


def test_cap_off_again_and_plan_cache(env):
    """the same handle, the same clip: cap on (the device raises levels in the plan it keeps), then off - the plain stream, and no records"""
    M, G = env
    c = G.cap_case("b3500")
    enc = encoder(M, Q=1)
    try:
        plain = G.encoded(c["frames"], c["W"], c["H"], c["pf"], 1)[0]
        assert resident(enc, c["frames"], c["W"], c["H"], c["pf"]) == plain
        enc.set_option("gop_bytes_max", c["B"])
        for _ in range(2):
            assert resident(enc, c["frames"], c["W"], c["H"], c["pf"]) == c["stream"]
            same_records(enc.gop_report(), c["records"])
        enc.set_option("gop_bytes_max", 0)
        assert resident(enc, c["frames"], c["W"], c["H"], c["pf"]) == plain
        assert len(enc.gop_report()) == 0
    finally:
        enc.close()


def test_cap_begin_end_on_two_handles_taking_turns(env):
    M, G = env
    import torch
    ca, cb = G.cap_case("b3500"), G.cap_case("b800")
    ea = encoder(M, Q=1, options=(("gop_bytes_max", ca["B"]),))
    eb = encoder(M, Q=1, options=(("gop_bytes_max", cb["B"]),))
    try:
        for _ in range(2):
            ka = resident(ea, ca["frames"], ca["W"], ca["H"], ca["pf"], begin=True)
            kb = resident(eb, cb["frames"], cb["W"], cb["H"], cb["pf"], begin=True)
            na, nb = ea.encode_resident_end(), eb.encode_resident_end()
            assert ka[1][:na].cpu().numpy().tobytes() == ca["stream"] and kb[1][:nb].cpu().numpy().tobytes() == cb["stream"]
            same_records(ea.gop_report(), ca["records"])
            same_records(eb.gop_report(), cb["records"])
        torch.cuda.synchronize()
    finally:
        ea.close()
        eb.close()


@pytest.mark.parametrize("options", [(), (("split_streams", 1),)], ids=["groups", "one_stream"])
def test_cap_with_stats(env, options):
    """the picture records of a GOP that went again are those of its final level"""
    import stats_cases as S
    M, G = env
    c = G.cap_case("b3500")
    f, W, H, pf = c["frames"], c["W"], c["H"], c["pf"]
    want = np.zeros(len(f), S.DTYPE)
    for k in range(len(f)):
        want[k] = S.records(G.encoded(f, W, H, pf, c["levels"][k // (pf + 1)])[1], W, H, pf)[k]
    enc = encoder(M, Q=1, options=options + (("stats", 1), ("gop_bytes_max", c["B"])))
    try:
        assert resident(enc, f, W, H, pf) == c["stream"]
        got = enc.picture_stats()
        for k in want.dtype.names:
            assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
        same_records(enc.gop_report(), c["records"])
    finally:
        enc.close()


def test_encode_tensor_cap(env):
    """encode_tensor(gop_bytes_max=...) on a planar RGB tensor: the stream of the converted planes under the cap; the cap is off again
    afterwards and the records still wait"""
    M, G = env
    c = G.cap_case("b3500")
    f, W, H, pf = c["frames"], c["W"], c["H"], c["pf"]
    planes = M.rgb_to444(f, W, H, "rgbp", "bt601")               # (the clip's three planes taken as R, G, B)
    B = sorted(G.gop_sizes(planes, W, H, pf)[1])[1]               # the median GOP size of level 2: from level 1, at least one GOP stops at 2
    want, levels = G.report(planes, W, H, pf, [1], B)
    assert len(set(levels)) > 1
    enc = encoder(M, Q=1)
    try:
        t = dev(np.ascontiguousarray(f))
        got = enc.encode_tensor(t, pf, gop_bytes_max=B).cpu().numpy().tobytes()
        assert got == G.splice(planes, W, H, pf, levels)
        same_records(enc.gop_report(), want)
        assert enc.encode_tensor(t, pf).cpu().numpy().tobytes() == G.encoded(planes, W, H, pf, 1)[0]
        assert len(enc.gop_report()) == 0
    finally:
        enc.close()


# ---- refusals: the stated code, and the handle stays usable ----
def test_refusals(env):
    M, G = env
    f, W, H = G.clip_args("c96")
    plain = G.encoded(f, W, H, 2, 2)[0]
    xs, ys = W // 16, H // 16
    enc = encoder(M, Q=2)
    try:
        L, h = enc._L, enc._h
        d = dev(f.reshape(len(f), -1))
        import torch
        out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        # a level of 0 or 5: M2V_E_PARAM, and the previous setting stays
        enc.set_gop_levels(G.SCHEDULE)
        for bad in ([1, 0, 2], [5], [2, 2, 200]):
            with pytest.raises(M.M2VError, match=r"\(-1\)"):
                enc.set_gop_levels(bad)
        assert resident(enc, f, W, H, 2) == G.splice(f, W, H, 2, G.SCHEDULE)
        # strips with a schedule
        assert L.m2v_strip_begin(h, xs, ys, 2, d.data_ptr(), len(f), 0, ys, None) == E_STATE
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            enc.strip_encode(None, 0, 1, d.data_ptr(), len(f), xs, ys, 2, out.data_ptr(), out.numel())
        enc.set_gop_levels(None)
        # ... and with a cap
        enc.set_option("gop_bytes_max", 3000)
        assert L.m2v_strip_begin(h, xs, ys, 2, d.data_ptr(), len(f), 0, ys, None) == E_STATE
        # a port-path start with the cap set
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            enc.push_frames(xs, ys, 2, f[:1])
        y = np.zeros(16, np.uint8)
        with pytest.raises(M.M2VError, match=r"\(-4\)"):
            enc.push_beats(xs, ys, 2, y, y, y)
        assert not enc.busy
        # a GOP longer than batch_frames
        enc.set_option("batch_frames", 2)
        with pytest.raises(M.M2VError, match=r"\(-1\).*batch_frames"):
            resident(enc, f, W, H, 2)
        with pytest.raises(M.M2VError, match=r"\(-1\)"):
            enc.set_option("gop_bytes_max", -1)
        enc.set_option("batch_frames", 96)
        enc.set_option("gop_bytes_max", 0)
        # the handle is as usable as ever: the plain stream, on the port path and resident, and strips again
        assert enc.encode(f, xs, ys, 2) == plain
        assert resident(enc, f, W, H, 2) == plain
        nb = enc.strip_encode(None, 0, 1, d.data_ptr(), len(f), xs, ys, 2, out.data_ptr(), out.numel())
        assert out[:nb].cpu().numpy().tobytes() == plain
    finally:
        enc.close()
