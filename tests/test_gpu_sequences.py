"""-m gpu: a batch of sequences in one resident call (m2v_set_sequences) against tests/seq_cases.py: the bytes at
[off[b], off[b + 1]) are byte for byte the oracle's stream of clip b encoded alone, and m2v_sequence_report hands out those offsets.
No tolerance anywhere.  tests/test_seq_cases.py shows what the cases reach.  Nothing is larger than 160 x 128; the longest call is
1100 one-frame sequences of 64 x 64."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE, E_OVERFLOW = -1, -4, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import seq_cases
    return seq_cases.M, seq_cases


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def encoder(M, Q=2, VL=3, options=(), lengths=None):
    enc = M.Mpeg2Encoder(6, 6, VL, Q)
    for k, v in options:
        enc.set_option(k, v)
    if lengths is not None:
        enc.set_sequences(lengths)
    return enc


def begin(enc, x, w, h, pf, kind="444", cap=None):
    """the first half of a resident call of `kind` over the frames x [n, ...]: -> what has to stay alive until the second"""
    import torch
    n = x.shape[0]
    xs, ys = (w + 15) // 16, (h + 15) // 16
    d_in = dev(x.reshape(n, -1))
    room = n * (3 * 256 * xs * ys + 128) + (1 << 16)
    d_out = torch.full((room,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (d_in.data_ptr(), n, d_out.data_ptr(), room if cap is None else cap, xs, ys, pf)
    if kind == "444":
        enc.encode_resident_begin(*a)
    elif kind == "rgb24":
        enc.encode_resident_rgb_begin(*a, kind)
    else:
        enc.encode_resident420_begin(*a, kind)
    return d_in, d_out


def resident(enc, x, w, h, pf, kind="444", cap=None):
    """one blocking resident call -> the bytes written"""
    import torch
    n = x.shape[0]
    xs, ys = (w + 15) // 16, (h + 15) // 16
    d_in = dev(x.reshape(n, -1))
    room = n * (3 * 256 * xs * ys + 128) + (1 << 16)
    d_out = torch.full((room,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (d_in.data_ptr(), n, d_out.data_ptr(), room if cap is None else cap, xs, ys, pf)
    if kind == "444":
        nb = enc.encode_resident(*a)
    elif kind == "rgb24":
        nb = enc.encode_resident_rgb(*a, kind)
    else:
        nb = enc.encode_resident420(*a, kind)
    out = d_out.cpu().numpy()
    assert (out[nb:] == 0xEE).all()                    # nothing behind off[n] is touched
    return out[:nb].tobytes()


def same_records(got, want, what=""):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


def check(Q, enc, got, want, off, lengths, pf, what=""):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        m = min(a.size, b.size)
        d = np.nonzero(a[:m] != b[:m])[0]
        raise AssertionError("%s: %d bytes, expected %d, first difference at %s (offsets %r)" % (what, a.size, b.size, d[0] if d.size else m, off))
    same_records(enc.sequence_report(), Q.records(lengths, off, pf), what)
    assert len(enc.sequence_report()) == 0             # popped


# ---- parity: every chunking gives the oracle's bytes ----
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("chunk", [96, 4, 5])
@pytest.mark.parametrize("name", ["mixed_pf2", "mixed_pf3", "fives_pf4"])
def test_parity(env, name, chunk, split):
    M, Q = env
    c = Q.parity(name)
    want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
    enc = encoder(M, options=(("batch_frames", chunk), ("split_streams", split)), lengths=c["lengths"])
    try:
        check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"], "%s chunk %d split %d" % (name, chunk, split))
    finally:
        enc.close()


@pytest.mark.parametrize("VL,QL", [(1, 4), (3, 1), (1, 1), (3, 4)])
def test_parity_levels_of_the_module(env, VL, QL):
    M, Q = env
    c = Q.parity("fives_pf4")
    want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"], Q=QL, VL=VL)
    enc = encoder(M, Q=QL, VL=VL, options=(("batch_frames", 4),), lengths=c["lengths"])
    try:
        check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"])
    finally:
        enc.close()


def test_begin_end_on_two_handles_taking_turns(env):
    import torch
    M, Q = env
    a, b = Q.parity("mixed_pf2"), Q.parity("fives_pf4")
    ea, eb = encoder(M, options=(("batch_frames", 5),), lengths=a["lengths"]), encoder(M, lengths=b["lengths"])
    try:
        for _ in range(2):
            ka = begin(ea, a["frames"], a["W"], a["H"], a["pf"])
            kb = begin(eb, b["frames"], b["W"], b["H"], b["pf"])
            for enc, c, keep in ((ea, a, ka), (eb, b, kb)):
                nb = enc.encode_resident_end()
                want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
                check(Q, enc, keep[1][:nb].cpu().numpy().tobytes(), want, off, c["lengths"], c["pf"])
        torch.cuda.synchronize()
    finally:
        ea.close()
        eb.close()


def test_remainders_of_the_final_word(env):
    """clips whose bytes in front of the end code are 0, 27, 28, 29 and 31 over a whole word, in one chunk and cut by a grid of 2"""
    M, Q = env
    c = Q.remainder_case()
    want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
    for chunk in (96, 2):
        enc = encoder(M, options=(("batch_frames", chunk),), lengths=c["lengths"])
        try:
            check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"], "chunk %d" % chunk)
        finally:
            enc.close()


# ---- the scan's own trip points ----
@pytest.mark.parametrize("name", ["below", "above_all"])
def test_scan_trip_points(env, name):
    """one-frame I-only sequences of 64 x 64 in ONE chunk: 1024 items (one a thread), and 4400 items of 1100 sequences - past a
    thread's cached items and past one sequence a thread"""
    M, Q = env
    c = Q.trip_case(name)
    enc = encoder(M, options=(("batch_frames", 2048),), lengths=c["lengths"])
    try:
        check(Q, enc, resident(enc, c["frames"], 64, 64, 0), c["stream"], c["offsets"], c["lengths"], 0, name)
    finally:
        enc.close()


# ---- composition, one case each ----
@pytest.mark.parametrize("kind", ["i420", "rgb24"])
def test_input_kinds(env, kind):
    import fit_cases as F
    M, Q = env
    c = Q.comp()
    W, H, pf, ln = c["W"], c["H"], c["pf"], c["lengths"]
    x = F.source(W, H, sum(ln), kind, seed=45)
    want, off = Q.expected(F.planes(x, W, H, kind), ln, W, H, pf)
    enc = encoder(M, options=(("batch_frames", 3),), lengths=ln)
    try:
        check(Q, enc, resident(enc, x, W, H, pf, kind), want, off, ln, pf, kind)
    finally:
        enc.close()


@pytest.mark.parametrize("header", ["module", "true"])
def test_frame_size_100x70(env, header):
    import fit_cases as F
    M, Q = env
    w, h, pf, ln = 100, 70, 2, [2, 4, 1]
    W, H = F.padded(w, h)
    x = F.source(w, h, sum(ln), "444", seed=46)
    s = Q.streams(F.planes(x, w, h, "444"), ln, W, H, pf)
    if header == "true":
        s = [M.set_header_size(b, w, h) for b in s]
    enc = encoder(M, options=(("batch_frames", 3),), lengths=ln)
    try:
        enc.set_frame_size(w, h, header)
        check(Q, enc, resident(enc, x, w, h, pf), b"".join(s), Q.lengths_offsets(s), ln, pf, header)
    finally:
        enc.close()


def test_conformant(env):
    M, Q = env
    c = Q.comp()
    want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"], conformant=True)
    enc = encoder(M, options=(("conformant", 1),), lengths=c["lengths"])
    try:
        check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"])
    finally:
        enc.close()


def test_level_schedule_goes_by_the_gop_inside_its_sequence(env):
    M, Q = env
    c = Q.comp()
    levels = [1, 4, 3]
    want, off = Q.levels_expected(levels)
    assert want != Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"], Q=1)[0]
    enc = encoder(M, Q=1, options=(("batch_frames", 4),), lengths=c["lengths"])
    try:
        enc.set_gop_levels(levels)
        check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"])
    finally:
        enc.close()


def test_description_with_repeated_headers(env):
    """30000/1001 and repeat_headers: every clip's time codes start at 0, its headers stand in front of each of its GOPs"""
    M, Q = env
    c = Q.comp()
    d = Q.D.desc(frame_rate_code=4, repeat_headers=1)
    want, off = Q.desc_expected(d)
    enc = encoder(M, options=(("batch_frames", 4),), lengths=c["lengths"])
    try:
        enc.set_stream_desc(Q.D.struct(d))
        check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"])
    finally:
        enc.close()


def test_stats_are_the_records_of_each_clip_alone(env):
    M, Q = env
    c = Q.comp()
    want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
    enc = encoder(M, options=(("stats", 1), ("batch_frames", 4)), lengths=c["lengths"])
    try:
        check(Q, enc, resident(enc, c["frames"], c["W"], c["H"], c["pf"]), want, off, c["lengths"], c["pf"])
        same_records(enc.picture_stats(), Q.stats_expected())
    finally:
        enc.close()


def test_recon_buffer_in_call_frame_order(env):
    import torch
    M, Q = env
    c = Q.comp()
    W, H, n = c["W"], c["H"], sum(c["lengths"])
    want, off = Q.expected(c["frames"], c["lengths"], W, H, c["pf"])
    rec = Q.recon_expected("nv12")
    fb = M.frame_bytes(W, H, "nv12")
    assert rec.shape == (n, fb)
    for chunk in (96, 3):
        buf = torch.full((n * fb + Q.R.GUARD,), Q.R.FILL, dtype=torch.uint8, device="cuda:0")
        enc = encoder(M, options=(("batch_frames", chunk),), lengths=c["lengths"])
        try:
            enc.set_recon_out(buf.data_ptr(), n * fb, "nv12")
            check(Q, enc, resident(enc, c["frames"], W, H, c["pf"]), want, off, c["lengths"], c["pf"])
            got = buf.cpu().numpy()
            assert np.array_equal(got[:n * fb].reshape(n, fb), rec), chunk
            assert (got[n * fb:] == Q.R.FILL).all()
        finally:
            enc.close()


# ---- one entry: no batch ----
def test_one_entry_is_nothing_set(env):
    M, Q = env
    c = Q.parity("fives_pf4")
    f, n = c["frames"], len(c["frames"])
    want = Q.G.encoded(f, c["W"], c["H"], c["pf"], 2)[0]
    counts = []
    for lengths in ([n], None):
        enc = encoder(M, options=(("profile", 1), ("batch_frames", 10)), lengths=lengths)
        try:
            assert resident(enc, f, c["W"], c["H"], c["pf"]) == want
            assert len(enc.sequence_report()) == 0
            counts.append([enc.kernel_stats(k)[0] for k in range(7)])
        finally:
            enc.close()
    assert counts[0] == counts[1] and counts[0][1] > 0


# ---- refusals and errors ----
def code_of(exc):
    return int(str(exc.value).split("(")[1].split(")")[0])


def test_refusals_and_errors(env):
    M, Q = env
    c = Q.comp()
    f, W, H, pf, ln = c["frames"], c["W"], c["H"], c["pf"], c["lengths"]
    want, off = Q.expected(f, ln, W, H, pf)
    plain = Q.G.encoded(f, W, H, pf, 2)[0]
    enc = encoder(M, lengths=ln)
    try:
        def still_fine():
            enc.set_sequences(None)
            assert resident(enc, f, W, H, pf) == plain
            enc.set_sequences(ln)

        # the port and the strips carry one sequence
        with pytest.raises(M.M2VError) as e:
            enc.push_frames(W // 16, H // 16, pf, f)
        assert code_of(e) == E_STATE
        still_fine()
        with pytest.raises(M.M2VError) as e:
            enc.push_beats(W // 16, H // 16, pf, f[0, 0].reshape(-1)[:64], f[0, 1].reshape(-1)[:64], f[0, 2].reshape(-1)[:64])
        assert code_of(e) == E_STATE
        d_in = dev(f.reshape(len(f), -1))
        with pytest.raises(M.M2VError) as e:
            enc.strip_begin(d_in.data_ptr(), len(f), W // 16, H // 16, pf, 0, H // 16)
        assert code_of(e) == E_STATE
        still_fine()
        # a batch with a GOP list, the detector or the cap
        for on, off_ in ((lambda: enc.set_gop_starts([3]), lambda: enc.set_gop_starts(None)),
                         (lambda: enc.set_option("scene_cut", 100), lambda: enc.set_option("scene_cut", 0)),
                         (lambda: enc.set_option("gop_bytes_max", 100000), lambda: enc.set_option("gop_bytes_max", 0))):
            on()
            with pytest.raises(M.M2VError) as e:
                resident(enc, f, W, H, pf)
            assert code_of(e) == E_STATE
            off_()
            still_fine()
        # the list must add up to the call's frames, and hold no 0
        with pytest.raises(M.M2VError) as e:
            resident(enc, f[:-1], W, H, pf)
        assert code_of(e) == E_PARAM
        enc.set_sequences([ln[0] + ln[1], 0] + ln[2:])
        with pytest.raises(M.M2VError) as e:
            resident(enc, f, W, H, pf)
        assert code_of(e) == E_PARAM
        enc.set_sequences(ln)
        still_fine()
        # cap = off[n] is enough, 32 bytes less is not
        assert resident(enc, f, W, H, pf, cap=off[-1]) == want
        with pytest.raises(M.M2VError) as e:
            resident(enc, f, W, H, pf, cap=off[-1] - 32)
        assert code_of(e) == E_OVERFLOW
        assert len(enc.sequence_report()) == 0
        still_fine()
        # the setting survives m2v_reset; None clears it
        enc.reset()
        check(Q, enc, resident(enc, f, W, H, pf), want, off, ln, pf, "after reset")
        enc.set_sequences(None)
        assert resident(enc, f, W, H, pf) == plain and len(enc.sequence_report()) == 0
    finally:
        enc.close()


# ---- Python ----
def test_encode_batch(env):
    import torch
    M, Q = env
    rng = np.random.default_rng(47)
    B, N, H, W = 3, 4, 64, 96
    x = rng.integers(0, 256, (B, N, H, W, 3), dtype=np.uint8)
    x[:, 1:] = x[:, :1] // 2 + x[:, 1:] // 8               # (frames of a clip resemble each other: P pictures with inter macroblocks)
    enc = encoder(M)
    try:
        t = torch.from_numpy(x).to("cuda:0")
        planes = M.rgb_to444(x.reshape(B * N, -1), W, H, "rgb24", "bt601")
        stream, offsets = enc.encode_batch(t, 3)
        want, off = Q.expected(planes, [N] * B, W, H, 3)
        assert offsets == off and stream.cpu().numpy().tobytes() == want
        ragged = [1, 6, 5]
        stream, offsets = enc.encode_batch(t.reshape(B * N, H, W, 3), 3, lengths=ragged)
        want, off = Q.expected(planes, ragged, W, H, 3)
        assert offsets == off and stream.cpu().numpy().tobytes() == want
        assert getattr(enc, "_sequences", None) is None        # the handle's own setting is back
        with pytest.raises(ValueError):
            enc.encode_batch(t.reshape(B * N, H, W, 3), 3, lengths=[1, 6, 4])
        with pytest.raises(ValueError):
            enc.encode_batch(t.reshape(B * N, H, W, 3), 3, lengths=[12, 0])
        with pytest.raises(ValueError):
            enc.encode_tensor(t, 3)                            # a 5-D tensor to plain encode_tensor: as ever
    finally:
        enc.close()


# ---- plain C ----
def test_batch_caller(env, tmp_path):
    M, Q = env
    M.build()
    libdir = os.path.join(ROOT, "fpga-mpeg2-encoder_amd")
    exe = str(tmp_path / "batch_caller")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           os.path.join(ROOT, "integration", "batch_caller.c"), "-L" + libdir, "-lm2v_mi355x", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    c = Q.comp()
    (tmp_path / "in.yuv").write_bytes(c["frames"].tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.yuv"), str(c["W"]), str(c["H"]), str(tmp_path), str(c["pf"])] + [str(n) for n in c["lengths"]],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    # (the caller's handle is XL = YL = 7: the stream does not depend on them at this size)
    for b, s in enumerate(Q.streams(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])):
        assert (tmp_path / ("out_%03d.m2v" % b)).read_bytes() == s, b
