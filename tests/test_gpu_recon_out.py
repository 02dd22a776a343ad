"""-m gpu: the reconstructed pictures of m2v_set_recon_out against the buffers tests/recon_cases.py derives from the oracle's `recon`
dump.  Every comparison is byte for byte (no tolerance anywhere).  In every case the buffer is filled with 0xA5 first, with a page's
worth of guard bytes behind the last frame that must stay 0xA5, the capacity handed in is exactly nframes * frame_bytes, and the
stream with the buffer set is the stream without it and the oracle's.  tests/test_recon_cases.py shows the cases are not vacuous.
The sizes are the smallest at which each piece can still go wrong; what each case is for is in its docstring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_PARAM, E_STATE, E_OVERFLOW = -1, -4, -6


@pytest.fixture(scope="module")
def env():
    import recon_cases
    return recon_cases.M, recon_cases


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def new_buffer(R, nbytes):
    import torch
    return torch.full((nbytes + R.GUARD,), R.FILL, dtype=torch.uint8, device="cuda:0")


def resident(enc, x, xs, ys, pf, kind="444", begin=False):
    """one sequence of the frames x [n, bytes] through the resident entry of `kind` ("444", "i420", "rgb24"); begin=True: only the
    first half.  -> the stream's bytes, or (d_in, d_out) to keep alive until _end"""
    import torch
    n = x.shape[0]
    d_in = dev(x.reshape(n, -1))
    d_out = torch.empty(n * 3 * 256 * xs * ys * 2 + (1 << 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a = (d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), xs, ys, pf)
    if begin:
        {"444": enc.encode_resident_begin, "i420": enc.encode_resident420_begin, "rgb24": enc.encode_resident_rgb_begin}[kind](*a)
        return d_in, d_out
    nb = enc.encode_resident(*a) if kind == "444" else enc.encode_resident420(*a, kind) if kind == "i420" else enc.encode_resident_rgb(*a, kind)
    return d_out[:nb].cpu().numpy().tobytes()


def check_buffer(R, buf, c, layout, what=""):
    """the frames are the expected ones, the guard behind them is untouched"""
    want = R.write_layout(c["recon"], c["W"], c["H"], layout, c["region"]).reshape(-1)
    got = buf.cpu().numpy()
    assert (got[want.size:] == R.FILL).all(), (what, "guard", np.nonzero(got[want.size:] != R.FILL)[0][:8].tolist())
    bad = np.nonzero(got[:want.size] != want)[0]
    assert bad.size == 0, (what, layout, "%d bytes differ, first at" % bad.size, bad[:8].tolist(), "frame bytes", want.size // c["n"])


def run(M, R, c, layout, options=(), x=None, kind="444", size=None, setup=None, misalign=0):
    """the case's sequence on one handle with the setting off, then with a buffer set: the streams are the oracle's, the buffer the
    expected one.  misalign: the buffer starts that many bytes behind an aligned address"""
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        for k, v in options:
            enc.set_option(k, v)
        if size:
            enc.set_frame_size(*size)
        if setup:
            setup(enc)
        x = c["frames"] if x is None else x
        xs, ys = c["W"] // 16, c["H"] // 16
        w, h = c["region"] or (c["W"], c["H"])
        nbytes = c["n"] * M.frame_bytes(w, h, layout)
        off = resident(enc, x, xs, ys, c["pf"], kind)
        whole = new_buffer(R, nbytes + misalign)
        buf = whole[misalign:]
        enc.set_recon_out(buf.data_ptr(), nbytes, layout)
        on = resident(enc, x, xs, ys, c["pf"], kind)
        assert off == c["stream"] and on == c["stream"], (options, layout, len(off), len(on), len(c["stream"]))
        check_buffer(R, buf, c, layout, options)
        assert (whole[:misalign].cpu().numpy() == R.FILL).all()
        return enc, buf
    except BaseException:
        enc.close()
        raise


def check(M, R, c, layout="i420", **kw):
    enc, _ = run(M, R, c, layout, **kw)
    enc.close()


def test_unreferenced_frames(env):
    """64 x 64, 5 frames, GOPs of 1 + 2: the last frame of each GOP and the final frame are referenced by nobody and have no
    reconstruction slot without the setting; they are written too"""
    M, R = env
    check(M, R, R.case("unref"))


def test_i_only(env):
    """pframes_count 0: without the setting there is no reconstruction pool at all"""
    M, R = env
    check(M, R, R.case("ionly"), "nv12")


@pytest.mark.parametrize("layout", ["i420", "yv12", "nv12", "nv21"])
def test_layouts(env, layout):
    """80 x 112: 5 x 7 macroblocks, chroma rows of 40 bytes - 8-byte aligned only, and the third 16-byte unit of a planar row is half
    outside; the planes in either order, the interleave in either order"""
    M, R = env
    check(M, R, R.case("g80"), layout)


@pytest.mark.parametrize("layout", ["i420", "nv21"])
def test_wide(env, layout):
    """272 x 64: 18 tiles per tile row, 17 units per luma row - rows that start in the middle of a wavefront"""
    M, R = env
    check(M, R, R.case("g272"), layout)


@pytest.mark.parametrize("options", [(("batch_frames", 3),), (("batch_frames", 96),), (("split_streams", 1),), (("split_streams", 2),),
                                     (("split_streams", 3), ("batch_frames", 96)), (("profile", 1),)], ids=lambda o: "-".join("%s%d" % kv for kv in o))
def test_chunks_and_streams(env, options):
    """160 x 128, 7 frames, GOPs of 1 + 4: chunks of 3 frames put a boundary inside a GOP (the reference persists into the next chunk
    from its slot) and frame numbers count on from the sequence's start; one, two and three group streams; the in-band timers"""
    M, R = env
    enc, _ = run(M, R, R.case("chunks"), "i420", options=options)
    try:
        if options == (("profile", 1),):
            launches, ms, units = enc.kernel_stats(6)
            assert launches >= 1 and ms > 0 and units == 7 * 160 * 128
    finally:
        enc.close()


@pytest.mark.parametrize("kind", ["444", "i420", "rgb24"])
@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("size", [(100, 70), (49, 49)])
def test_frame_size(env, size, layout, kind):
    """100 x 70 is coded as 112 x 80, 49 x 49 (chroma 25 x 25) as 64 x 64: the frames are the cropped pictures, rows of 100 / 50 / 49 /
    25 bytes at unaligned addresses, cropped right and bottom, frame n + 1 right behind frame n; from every kind of source.  The
    buffer itself starts at an odd address"""
    M, R = env
    c = R.fit_case(size[0], size[1], kind)
    check(M, R, c, layout, x=c["x"], kind=kind, size=size, misalign=1)


def test_conformant(env):
    """option "conformant", 96 x 64, 4 frames in one GOP: the oracle's conformant dump - and what a standard decoder shows"""
    M, R = env
    c = R.case("conformant")
    enc, buf = run(M, R, c, "i420", options=(("conformant", 1),))
    enc.close()
    W, H = c["W"], c["H"]
    y, u, v = M.planes_of_recon(buf[:c["n"] * M.frame_bytes(W, H, "i420")].cpu().numpy(), W, H, "i420")
    d = M.decoder.decode(c["stream"], quirks=False)
    for f in range(c["n"]):
        for got, want in zip((y[f], u[f], v[f]), d.frames[f]):
            assert np.array_equal(got, want), f


def test_vector_level_and_q(env):
    """VECTOR_LEVEL 1, Q_LEVEL 4: the slot layout depends on neither"""
    M, R = env
    check(M, R, R.case("vl1q4"), "yv12")


def test_with_stats(env):
    """with option "stats" on too: the records and the pictures are both right (k_picstat and k_recon_out read the same slots)"""
    M, R = env
    c = R.case("unref")
    enc, _ = run(M, R, c, "nv12", options=(("stats", 1),))
    try:
        got = enc.picture_stats()
        assert got.tobytes() == c["records"].tobytes()
    finally:
        enc.close()


def test_with_gop_levels(env):
    """m2v_set_gop_levels: GOPs at levels 1, 4, 3 - one k_mb launch per level, one k_recon_out per list"""
    M, R = env
    c = R.levels_case()
    check(M, R, c, setup=lambda enc: enc.set_gop_levels(c["levels"]))


def test_with_gop_bytes_max(env):
    """option "gop_bytes_max": GOPs 0 and 1 are coded again (tests/recon_cases.py asserts it from the oracle's sizes), GOP 2 is left
    alone - the frames are those of each GOP's final level"""
    M, R = env
    c = R.cap_case()
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        xs, ys = c["W"] // 16, c["H"] // 16
        nbytes = c["n"] * M.frame_bytes(c["W"], c["H"], "i420")
        enc.set_option("gop_bytes_max", c["B"])
        off = resident(enc, c["frames"], xs, ys, c["pf"])
        buf = new_buffer(R, nbytes)
        enc.set_recon_out(buf.data_ptr(), nbytes, "i420")
        on = resident(enc, c["frames"], xs, ys, c["pf"])
        assert off == c["stream"] and on == c["stream"]
        assert enc.gop_report()["level"].tolist() == c["levels"]
        check_buffer(R, buf, c, "i420")
    finally:
        enc.close()


def test_with_gop_starts(env):
    """m2v_set_gop_starts, 12 frames with starts at 2 and 7 (chunks of 5 too: the next chunk's start ends a GOP early): the splice of
    the oracle's dumps of the GOPs encoded alone"""
    M, R = env
    c = R.starts_case()
    for options in ((), (("batch_frames", 5),)):
        check(M, R, c, options=options, setup=lambda enc: enc.set_gop_starts(c["starts"]))


def test_with_scene_cut(env):
    """option "scene_cut" at a threshold nothing reaches: the detector's wait per chunk in front of the plan changes nothing"""
    M, R = env
    check(M, R, R.case("unref"), options=(("scene_cut", 65280),))


def test_two_handles_in_flight(env):
    """_begin / _end on two handles taking turns, each with its own buffer and layout"""
    M, R = env
    a, b = R.case("unref"), R.case("g80")
    ea, eb = M.Mpeg2Encoder(*a["params"]), M.Mpeg2Encoder(*b["params"])
    try:
        na, nb = (c["n"] * M.frame_bytes(c["W"], c["H"], "i420") for c in (a, b))
        ba, bb = new_buffer(R, na), new_buffer(R, nb)
        ea.set_recon_out(ba.data_ptr(), na, "i420")
        eb.set_recon_out(bb.data_ptr(), nb, "nv12")
        for _ in range(2):
            ka = resident(ea, a["frames"], a["W"] // 16, a["H"] // 16, a["pf"], begin=True)
            kb = resident(eb, b["frames"], b["W"] // 16, b["H"] // 16, b["pf"], begin=True)
            assert ea._L.m2v_set_recon_out(ea._h, None, 0, 0) == E_STATE          # busy: the setting stays
            sa, sb = ea.encode_resident_end(), eb.encode_resident_end()
            assert ka[1][:sa].cpu().numpy().tobytes() == a["stream"] and kb[1][:sb].cpu().numpy().tobytes() == b["stream"]
            check_buffer(R, ba, a, "i420", "a")
            check_buffer(R, bb, b, "nv12", "b")
            ba.fill_(R.FILL)
            bb.fill_(R.FILL)
    finally:
        ea.close()
        eb.close()


def test_resident420_and_rgb_entries(env):
    """the 4:2:0 and the RGB resident entries, blocking and as _begin / _end, at whole macroblocks: the expansion or conversion runs in
    front of the chunk, the reconstruction leaves behind it"""
    M, R = env
    c = R.case("g80")
    W, H, n = c["W"], c["H"], c["n"]
    srcs = {"i420": M.to420(c["frames"], "i420"), "rgb24": np.random.default_rng(5).integers(0, 256, (n, H * W * 3), dtype=np.uint8)}
    from oracle import m2v_oracle_ctypes as orc
    for kind, x in srcs.items():
        planes = M.to444(x, W, H, "i420") if kind == "i420" else M.rgb_to444(x, W, H, "rgb24")
        stream, dump = orc.encode(planes, W // 16, H // 16, c["pf"], *c["params"], dump=True)
        want = dict(c, recon=dump["recon"], stream=stream)
        nbytes = n * M.frame_bytes(W, H, "nv21")
        enc = M.Mpeg2Encoder(*c["params"])
        try:
            buf = new_buffer(R, nbytes)
            enc.set_recon_out(buf.data_ptr(), nbytes, "nv21")
            assert resident(enc, x, W // 16, H // 16, c["pf"], kind) == stream
            check_buffer(R, buf, want, "nv21", kind)
            buf.fill_(R.FILL)
            keep = resident(enc, x, W // 16, H // 16, c["pf"], kind, begin=True)
            nb = enc.encode_resident_end()
            assert keep[1][:nb].cpu().numpy().tobytes() == stream
            check_buffer(R, buf, want, "nv21", kind + " begin/end")
        finally:
            enc.close()


def test_encode_tensor_recon(env):
    import torch
    M, R = env
    c = R.fit_case(100, 70, "rgb24")
    enc = M.Mpeg2Encoder(*c["params"])
    try:
        t = dev(c["x"].reshape(c["n"], c["h"], c["w"], 3))
        stream, rec = enc.encode_tensor(t, c["pf"], header="module", recon="nv12")
        assert isinstance(rec, torch.Tensor) and rec.device == t.device and rec.dtype == torch.uint8
        assert tuple(rec.shape) == (c["n"], M.frame_bytes(100, 70, "nv12"))
        assert stream.cpu().numpy().tobytes() == c["stream"]
        assert rec.cpu().numpy().tobytes() == R.write_layout(c["recon"], c["W"], c["H"], "nv12", c["region"]).tobytes()
        stream, records, rec = enc.encode_tensor(t, c["pf"], header="module", stats=True, recon="i420")
        assert len(records) == c["n"] and rec.cpu().numpy().tobytes() == R.write_layout(c["recon"], c["W"], c["H"], "i420", c["region"]).tobytes()
        assert enc.encode_tensor(t, c["pf"], header="module").cpu().numpy().tobytes() == c["stream"]       # the setting is off again
        with pytest.raises(ValueError):
            enc.encode_tensor(t, c["pf"], header="module", recon="rgb24")
        assert enc.frame_size is None                                # (refused before any setting of the handle was touched)
        # a buffer of the caller's own is back after a call that used another
        own = new_buffer(R, c["n"] * M.frame_bytes(112, 80, "i420"))
        enc.set_recon_out(own.data_ptr(), own.numel() - R.GUARD, "i420")
        stream, rec = enc.encode_tensor(t, c["pf"], header="module", recon="nv12")
        assert rec.cpu().numpy().tobytes() == R.write_layout(c["recon"], c["W"], c["H"], "nv12", c["region"]).tobytes()
        assert bool((own == R.FILL).all().item())
        padded = dev(M.pad_frames(c["x"], 100, 70, "rgb24"))
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
        nb = enc.encode_resident_rgb(padded.data_ptr(), c["n"], d_out.data_ptr(), d_out.numel(), 7, 5, c["pf"], "rgb24")
        assert d_out[:nb].cpu().numpy().tobytes() == c["stream"]
        check_buffer(R, own, dict(c, region=None), "i420", "the caller's own buffer")
    finally:
        enc.close()


def test_errors(env):
    import torch
    M, R = env
    c = R.case("unref")
    x = c["frames"].reshape(c["n"], -1)
    nbytes = c["n"] * M.frame_bytes(64, 64, "i420")
    enc = M.Mpeg2Encoder(*c["params"])
    L, hd = enc._L, enc._h
    try:
        buf = new_buffer(R, nbytes)
        untouched = lambda: bool((buf.cpu().numpy() == R.FILL).all())
        assert L.m2v_set_recon_out(hd, buf.data_ptr(), nbytes, 4) == E_PARAM and L.m2v_set_recon_out(hd, buf.data_ptr(), nbytes, -1) == E_PARAM
        assert L.m2v_set_recon_out(None, buf.data_ptr(), nbytes, 0) == E_PARAM
        assert resident(enc, c["frames"], 4, 4, c["pf"]) == c["stream"] and untouched()                  # (refused: nothing is set)
        # one byte short: refused before anything is launched, and the handle stays usable
        enc.set_recon_out(buf.data_ptr(), nbytes - 1, "i420")
        with pytest.raises(M.M2VError) as ei:
            resident(enc, c["frames"], 4, 4, c["pf"])
        assert "(%d)" % E_OVERFLOW in str(ei.value) and not enc.busy
        torch.cuda.synchronize()
        assert untouched()
        # ... fewer frames fit
        few = dict(c, n=4, recon=c["recon"][:4])
        resident(enc, c["frames"][:4], 4, 4, c["pf"])
        check_buffer(R, buf, few, "i420", "four frames")             # (and the fifth frame's place is untouched)
        buf.fill_(R.FILL)
        # the port and the strips: refused while a buffer is set
        enc.set_recon_out(buf.data_ptr(), nbytes, "i420")
        assert L.m2v_push_frames(hd, 4, 4, c["pf"], x.ctypes.data, 1) == E_STATE and b"m2v_set_recon_out" in L.m2v_last_error(hd) and not enc.busy
        y = np.ascontiguousarray(c["frames"][0, 0]).reshape(-1)
        assert L.m2v_push_beats(hd, 4, 4, c["pf"], y.ctypes.data, y.ctypes.data, y.ctypes.data, 16, 0) == E_STATE and not enc.busy
        d_in = dev(x)
        assert L.m2v_strip_begin(hd, 4, 4, c["pf"], d_in.data_ptr(), 1, 0, 4, None) == E_STATE and b"m2v_set_recon_out" in L.m2v_last_error(hd)
        assert not enc.busy and untouched()
        # the setter while busy: E_STATE, and the setting stays
        keep = resident(enc, c["frames"], 4, 4, c["pf"], begin=True)
        assert L.m2v_set_recon_out(hd, None, 0, 0) == E_STATE and L.m2v_set_recon_out(hd, buf.data_ptr(), nbytes, 2) == E_STATE
        nb = enc.encode_resident_end()
        assert keep[1][:nb].cpu().numpy().tobytes() == c["stream"]
        check_buffer(R, buf, c, "i420", "after the refused setter")
        # it survives m2v_reset
        buf.fill_(R.FILL)
        enc.reset()
        assert resident(enc, c["frames"], 4, 4, c["pf"]) == c["stream"]
        check_buffer(R, buf, c, "i420", "after reset")
        # cleared: the parent's behaviour - the stream is equal, the buffer untouched, the port works
        buf.fill_(R.FILL)
        enc.set_recon_out(None, 0)
        assert resident(enc, c["frames"], 4, 4, c["pf"]) == c["stream"]
        enc.push_frames(4, 4, c["pf"], x)
        enc.sequence_stop()
        assert enc.pull_all() == c["stream"]
        torch.cuda.synchronize()
        assert untouched()
    finally:
        enc.close()


def test_tb_recon(env, tmp_path):
    """m2v_tb -scenecut T -recon: the file holds the frames the library wrote; without the resident mode it says why not"""
    import os
    import subprocess
    M, R = env
    c = R.case("unref")
    tb = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fpga-mpeg2-encoder_amd", "m2v_tb")
    assert os.path.exists(tb), "m2v_tb is built by __graft_entry__.build()"
    fin, fout, frec = tmp_path / "in.yuv", tmp_path / "out.m2v", tmp_path / "rec.yuv"
    fin.write_bytes(c["frames"].tobytes())
    base = [tb, "-XL", "6", "-YL", "6", "-p", str(c["pf"])]
    r = subprocess.run(base + ["-scenecut", "65280", "-recon", str(frec), "-reconfmt", "nv12", str(fin), "64", "64", str(fout)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert fout.read_bytes() == c["stream"]
    assert frec.read_bytes() == R.write_layout(c["recon"], 64, 64, "nv12").tobytes()
    r = subprocess.run(base + ["-recon", str(frec), str(fin), "64", "64", str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "resident" in r.stderr
