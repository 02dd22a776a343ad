"""-m gpu: the per-picture statistics of option "stats" (m2v_picture_stats) against the records tests/stats_cases.py derives from the
oracle's dumps.  In every case the stream with the option on is byte for byte the stream with it off and the oracle's, and the records
equal the expected ones field for field (exact integers: no tolerance anywhere).  tests/test_stats_cases.py shows the clips are not
vacuous.  The sizes are the smallest at which each piece can still go wrong; what each case is for is in its docstring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE = -1, -4
FIELDS = ("frame", "coding_type", "sse", "mb_bits", "intra_mbs", "inter_mbs", "coded_blocks", "mv_abs_x", "mv_abs_y", "reserved")


@pytest.fixture(scope="module")
def env():
    import stats_cases
    return stats_cases.M, stats_cases


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def same(got, want, what=""):
    """field for field, with the first field that differs in the message"""
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())
    assert got.tobytes() == want.tobytes(), what


def resident(enc, x, xs, ys, pf, kind="444", begin=False):
    """one sequence of the frames x [n, bytes] through the resident entry of `kind`; begin=True: only the first half"""
    import torch
    n = x.shape[0]
    d_in = dev(x.reshape(n, -1))
    d_out = torch.empty(n * 3 * 256 * xs * ys * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), xs, ys, pf)
    if begin:
        assert kind == "444"
        enc.encode_resident_begin(*a)
        return d_in, d_out
    nb = enc.encode_resident(*a) if kind == "444" else enc.encode_resident420(*a, kind) if kind == "i420" else enc.encode_resident_rgb(*a, kind)
    return d_out[:nb].cpu().numpy().tobytes()


def both(M, c, options=(), frames=None, size=None, kind="444"):
    """the case's sequence with the option off, then on, on one handle: (stream off, stream on, records)"""
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        for k, v in options:
            enc.set_option(k, v)
        if size:
            enc.set_frame_size(*size)
        x = c["frames"] if frames is None else frames
        xs, ys = c["W"] // 16, c["H"] // 16
        off = resident(enc, x, xs, ys, c["pf"], kind)
        assert len(enc.picture_stats()) == 0                     # the option is off: nothing waits
        enc.set_option("stats", 1)
        on = resident(enc, x, xs, ys, c["pf"], kind)
        assert enc._L.m2v_picture_stats(enc._h, None, 0) == x.shape[0]
        return off, on, enc.picture_stats()
    finally:
        enc.close()


def check_case(M, S, name, options=()):
    c = S.case(name)
    off, on, got = both(M, c, options)
    assert off == c["stream"] and on == c["stream"], (name, options)
    same(got, c["records"], (name, options))
    return got


def test_unreferenced_frames(env):
    """64 x 64, 5 frames, GOPs of 1 + 2: the last frame of each GOP and the final frame are referenced by nobody and have no
    reconstruction slot without the option"""
    check_case(*env, "unref")


def test_i_only(env):
    """pframes_count 0: without the option there is no reconstruction pool at all"""
    check_case(*env, "ionly")


def test_chunk_boundaries(env):
    """160 x 128 (two units of eight tiles per tile row, the second one partial), 7 frames, GOPs of 1 + 4: chunks of 96, 2 and 3 frames put
    chunk boundaries nowhere, inside a GOP (the reference persists into the next chunk) and on a GOP's last frame"""
    M, S = env
    got = [check_case(M, S, "chunks", opts) for opts in ((), (("batch_frames", 2),), (("batch_frames", 3),))]
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_group_streams(env):
    """7 frames in GOPs of 1 + 2 are three segments: two group streams by default; then one stream, then the in-band timers of "profile" """
    M, S = env
    for opts in ((), (("split_streams", 1),), (("profile", 1),), (("split_streams", 3), ("cu_pack", 0))):
        check_case(M, S, "groups", opts)


@pytest.mark.parametrize("vl", [1, 2, 3])
@pytest.mark.parametrize("q", [1, 4])
def test_parameter_matrix(env, vl, q):
    check_case(*env, "vl%dq%d" % (vl, q))


@pytest.mark.parametrize("name", ["fit444", "fit420", "fitrgb", "fit49"])
def test_frame_size(env, name):
    """100 x 70 is coded as 112 x 80 (49 x 49 as 64 x 64): the padding is coded and counted in bits and decisions, and not measured -
    luma 100 x 70, chroma 50 x 35 (25 x 25: the odd size rounds up)"""
    M, S = env
    c = S.fit_case(name)
    off, on, got = both(M, c, frames=c["x"], size=(c["w"], c["h"]), kind=c["kind"])
    assert off == c["stream"] and on == c["stream"]
    same(got, c["records"], name)


def test_encode_tensor_stats(env):
    import torch
    M, S = env
    c = S.fit_case("fitrgb")
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        t = dev(c["x"].reshape(c["n"], c["h"], c["w"], 3))
        stream, got = enc.encode_tensor(t, c["pf"], header="module", stats=True)
        assert isinstance(stream, torch.Tensor) and stream.cpu().numpy().tobytes() == c["stream"]
        same(got, c["records"])
        assert enc.encode_tensor(t, c["pf"], header="module").cpu().numpy().tobytes() == c["stream"]      # the option is off again
        assert len(enc.picture_stats()) == 0
    finally:
        enc.close()


def test_conformant(env):
    """option "conformant": the records are the oracle's for its conformant loop - and what a standard decoder makes of the stream"""
    M, S = env
    c = S.case("conformant")
    off, on, got = both(M, c, (("conformant", 1),))
    assert off == c["stream"] and on == c["stream"]
    same(got, c["records"])
    d = M.decoder.decode(on, quirks=False)
    W, H = c["W"], c["H"]
    for f in range(c["n"]):
        src = S.planes420(c["dump"]["yuv420"][f], W, H)
        sse = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(src, d.frames[f])]
        assert sse == got["sse"][f].tolist(), f


def test_port_frames(env):
    """m2v_push_frames in two calls and the stop, chunks of 2 frames: a chunk's records arrive with its words"""
    M, S = env
    c = S.case("port")
    xs, ys, x = c["W"] // 16, c["H"] // 16, c["frames"].reshape(c["n"], -1)
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        enc.set_option("batch_frames", 2)
        enc.set_option("stats", 1)
        waiting = lambda: enc._L.m2v_picture_stats(enc._h, None, 0)
        enc.set_option("async", 0)                               # a chunk is complete when the push that filled it returns
        enc.push_frames(xs, ys, c["pf"], x[:3])
        assert waiting() == 2
        enc.push_frames(xs, ys, c["pf"], x[3:])
        assert waiting() == 4
        enc.sequence_stop()
        assert enc.pull_all() == c["stream"] and waiting() == 5
        first = enc.picture_stats(2)                             # oldest first, the rest keeps waiting
        assert first["frame"].tolist() == [0, 1] and waiting() == 3
        same(np.concatenate([first, enc.picture_stats()]), c["records"], "async 0")
        enc.set_option("async", 1)                               # two chunks in flight: everything is there once the stop has been pulled
        enc.push_frames(xs, ys, c["pf"], x[:3])
        enc.push_frames(xs, ys, c["pf"], x[3:])
        enc.sequence_stop()
        assert enc.pull_all() == c["stream"]
        same(enc.picture_stats(), c["records"], "async 1")
    finally:
        enc.close()


@pytest.mark.parametrize("form", ["beats", "packed"])
def test_port_stop_inside_a_frame(env, form):
    """2 1/2 frames of 64 x 64, then the stop: the last record counts the black fill.  Beats on three arrays are filled on the host,
    packed samples by the kernels (FrameJob::valid_beats)"""
    M, S = env
    c = S.case("beats")
    nb = c["nbeats"]
    y, u, v = (c["frames"][:, p].reshape(-1)[:4 * nb] for p in range(3))
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        enc.set_option("stats", 1)
        if form == "beats":
            enc.push_beats(4, 4, c["pf"], y, u, v, stop_with_last=True)
        else:
            enc.push_packed(4, 4, c["pf"], np.stack([y, u, v], axis=1), "yuv24", stop_with_last=True)
        assert enc.pull_all() == c["stream"]
        same(enc.picture_stats(), c["records"], form)
    finally:
        enc.close()


def test_two_handles_in_flight(env):
    M, S = env
    a, b = S.case("unref"), S.case("vl3q1")
    ea, eb = M.Mpeg2Encoder(*a["params"]), M.Mpeg2Encoder(*b["params"])
    try:
        ea.set_option("stats", 1)
        eb.set_option("stats", 1)
        ka = resident(ea, a["frames"], a["W"] // 16, a["H"] // 16, a["pf"], begin=True)
        kb = resident(eb, b["frames"], b["W"] // 16, b["H"] // 16, b["pf"], begin=True)
        na, nb = ea.encode_resident_end(), eb.encode_resident_end()
        assert ka[1][:na].cpu().numpy().tobytes() == a["stream"] and kb[1][:nb].cpu().numpy().tobytes() == b["stream"]
        same(ea.picture_stats(), a["records"], "a")
        same(eb.picture_stats(), b["records"], "b")
    finally:
        ea.close()
        eb.close()


def test_two_sequences_on_one_handle(env):
    """the first sequence's records unread: the second starts again at frame 0 and the old ones are gone; m2v_reset drops them too"""
    M, S = env
    a, b = S.case("unref"), S.case("ionly")
    enc = M.Mpeg2Encoder(*a["params"])
    try:
        enc.set_option("stats", 1)
        assert resident(enc, a["frames"], 4, 4, a["pf"]) == a["stream"]
        assert resident(enc, b["frames"], 4, 4, b["pf"]) == b["stream"]
        same(enc.picture_stats(), b["records"])
        assert resident(enc, a["frames"], 4, 4, a["pf"]) == a["stream"]
        enc.reset()
        assert len(enc.picture_stats()) == 0
        assert resident(enc, a["frames"], 4, 4, a["pf"]) == a["stream"]
        same(enc.picture_stats(), a["records"])
    finally:
        enc.close()


def test_errors(env):
    import torch
    M, S = env
    c = S.case("unref")
    x = c["frames"].reshape(c["n"], -1)
    enc = M.Mpeg2Encoder(*c["params"])
    L, hd = enc._L, enc._h
    try:
        # the option is set only while the handle is idle
        enc.push_frames(4, 4, c["pf"], x[:1])
        assert enc.busy and L.m2v_set_option(hd, b"stats", 1) == E_STATE and b"idle" in L.m2v_last_error(hd)
        enc.push_frames(4, 4, c["pf"], x[1:])
        enc.sequence_stop()
        assert enc.pull_all() == c["stream"]
        assert L.m2v_picture_stats(hd, None, 0) == 0             # ... and it was refused: off
        d_in, d_out = resident(enc, c["frames"], 4, 4, c["pf"], begin=True)
        assert L.m2v_set_option(hd, b"stats", 1) == E_STATE
        nb = enc.encode_resident_end()
        assert d_out[:nb].cpu().numpy().tobytes() == c["stream"]
        rec = (M.PictureStat * 8)()
        assert L.m2v_picture_stats(hd, rec, 8) == 0 and L.m2v_picture_stats(None, rec, 8) == E_PARAM
        # strips hold part of a picture: refused while the option is on, and the handle works on
        enc.set_option("stats", 1)
        assert L.m2v_strip_begin(hd, 4, 4, c["pf"], d_in.data_ptr(), 1, 0, 4, None) == E_STATE
        assert b"stats" in L.m2v_last_error(hd) and not enc.busy
        assert resident(enc, c["frames"], 4, 4, c["pf"]) == c["stream"]
        assert L.m2v_picture_stats(hd, rec, 2) == 2 and (rec[0].frame, rec[1].frame, rec[1].coding_type) == (0, 1, 2)
        same(np.concatenate([np.frombuffer(rec, M.PICTURE_STAT_DTYPE, 2), enc.picture_stats()]), c["records"])
        enc.set_option("stats", 0)
        assert resident(enc, c["frames"], 4, 4, c["pf"]) == c["stream"]
        assert L.m2v_picture_stats(hd, None, 0) == 0
        torch.cuda.synchronize()
    finally:
        enc.close()


def test_tb_stats(env, tmp_path):
    """m2v_tb -stats: one line per picture and the summary, from the encoder's records"""
    import os
    import re
    import subprocess
    M, S = env
    c = S.case("unref")
    tb = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fpga-mpeg2-encoder_amd", "m2v_tb")
    assert os.path.exists(tb), "m2v_tb is built by __graft_entry__.build()"
    fin, fout = tmp_path / "in.yuv", tmp_path / "out.m2v"
    fin.write_bytes(c["frames"].tobytes())
    r = subprocess.run([tb, "-XL", "6", "-YL", "6", "-p", str(c["pf"]), "-stats", str(fin), "64", "64", str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert fout.read_bytes() == c["stream"]
    lines = re.findall(r"stats video 1 frame +(\d+) ([IP])  PSNR Y +([\d.]+|inf) U +([\d.]+|inf) V +([\d.]+|inf)  intra +(\d+) inter +(\d+)  mb bits +(\d+)  bytes +(\d+)",
                       r.stdout)
    want = c["records"]
    assert len(lines) == len(want), r.stdout
    n = S.samples3(64, 64)
    for ln, w in zip(lines, want):
        assert (int(ln[0]), ln[1], int(ln[5]), int(ln[6]), int(ln[7])) == (w["frame"], "IP"[w["coding_type"] - 1], w["intra_mbs"], w["inter_mbs"], w["mb_bits"])
        for k in range(3):
            assert abs(float(ln[2 + k]) - M.psnr_from_sse(int(w["sse"][k]), n[k])) <= 0.005 + 1e-9
    assert sum(int(ln[8]) for ln in lines) <= len(c["stream"])
    mean = re.search(r"stats video 1: mean PSNR Y +([\d.]+)", r.stdout)
    assert mean and abs(float(mean.group(1)) - np.mean([M.psnr_from_sse(int(w["sse"][0]), n[0]) for w in want])) <= 0.005 + 1e-9
