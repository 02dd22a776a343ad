"""The cases of tests/recon_cases.py are sound (no GPU): the layout writers and planes_of_recon agree, the cropped expectation is the
top-left region of the oracle's dump, the conformant dump is what a standard decoder shows and the module's is not, and no expected
buffer could be produced by copying the input or one reconstruction slot."""
import numpy as np
import pytest

import recon_cases as R

M = R.M


def test_entry_point_is_declared():
    L = M.lib()
    assert hasattr(L, "m2v_set_recon_out") and "m2v_set_recon_out" in M.EXPORTS
    assert hasattr(M.Mpeg2Encoder, "set_recon_out") and callable(M.planes_of_recon)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("size", [(80, 112, None), (112, 80, (100, 70)), (64, 64, (49, 49))])
def test_writers_round_trip(layout, size):
    """write_layout and planes_of_recon are each other's inverse, for whole and cropped (odd) sizes; the frame is frame_bytes long"""
    W, H, region = size
    w, h = region or (W, H)
    rng = np.random.default_rng(W + h)
    dump = rng.integers(0, 256, (3, W * H * 3 // 2), dtype=np.uint8)
    buf = R.write_layout(dump, W, H, layout, region)
    assert buf.shape == (3, M.frame_bytes(w, h, layout))
    y, u, v = M.planes_of_recon(buf, w, h, layout)
    Y, U, V = (np.stack(p) for p in zip(*(R.S.planes420(d, W, H) for d in dump)))
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert np.array_equal(y, Y[:, :h, :w]) and np.array_equal(u, U[:, :ch, :cw]) and np.array_equal(v, V[:, :ch, :cw])
    assert np.array_equal(M.planes_of_recon(buf.reshape(-1), w, h, M.LAYOUTS_420[layout])[2], v)       # flat buffer, layout by code
    # the four layouts hold the same samples, and differ as bytes
    if layout != "i420":
        assert buf.tobytes() != R.write_layout(dump, W, H, "i420", region).tobytes()


def test_planes_of_recon_rejects_unknown_layout():
    with pytest.raises((ValueError, KeyError)):
        M.planes_of_recon(np.zeros(96, np.uint8), 8, 8, "rgb24")


def test_cropped_expectation_is_the_top_left_region():
    c = R.fit_case(100, 70, "444")
    W, H = c["W"], c["H"]
    assert (W, H) == (112, 80)
    buf = R.write_layout(c["recon"], W, H, "i420", c["region"])
    for f in range(c["n"]):
        Y, U, V = R.S.planes420(c["recon"][f], W, H)
        assert buf[f, :7000].tobytes() == Y[:70, :100].tobytes()
        assert buf[f, 7000:7000 + 1750].tobytes() == U[:35, :50].tobytes() and buf[f, 8750:].tobytes() == V[:35, :50].tobytes()
    assert buf.shape[1] == 7000 + 2 * 1750


def test_conformant_dump_is_what_a_decoder_shows():
    c = R.case("conformant")
    d = M.decoder.decode(c["stream"], quirks=False)
    assert len(d.frames) == c["n"]
    for f in range(c["n"]):
        for a, b in zip(R.S.planes420(c["recon"][f], c["W"], c["H"]), d.frames[f]):
            assert np.array_equal(a, b), f


def test_module_dump_is_not_what_a_decoder_shows():
    """without "conformant" a P picture of the module's loop differs from a standard decoder's: the two expectations are not
    interchangeable.  The decoder with the module's deviations switched on reproduces the dump."""
    differs = 0
    for name in ("unref", "chunks", "g80"):
        c = R.case(name)
        d, q = M.decoder.decode(c["stream"], quirks=False), M.decoder.decode(c["stream"], quirks=True)
        for f in range(c["n"]):
            want = R.S.planes420(c["recon"][f], c["W"], c["H"])
            assert all(np.array_equal(a, b) for a, b in zip(want, q.frames[f])), (name, f)
            if f % (c["pf"] + 1):
                differs += not all(np.array_equal(a, b) for a, b in zip(want, d.frames[f]))
    assert differs > 0


def test_expectations_tell_frames_and_source_apart():
    """in every GPU case at least two frames of the expected buffer differ, and every frame differs from the source as coded: a kernel
    that copies the input, or one slot for every frame, fails"""
    for name, c in R.gpu_cases().items():
        W, H, n = c["W"], c["H"], c["n"]
        assert c["recon"].shape == (n, W * H * 3 // 2) and c["source"].shape == c["recon"].shape, name
        want = R.write_layout(c["recon"], W, H, "i420", c["region"])
        src = R.write_layout(c["source"], W, H, "i420", c["region"])
        assert len({want[f].tobytes() for f in range(n)}) >= 2, name
        assert all(want[f].tobytes() != src[f].tobytes() for f in range(n)), name
        assert want.any() and len(c["stream"]) > 0, name


def test_cap_case_redoes_some_gops_and_leaves_one():
    c = R.cap_case()
    assert c["levels"] == [3, 2, 1] and c["params"][3] == 1
    lv = R.levels_case()
    assert R.G.per_gop(lv["levels"], 3) == [1, 4, 3]
    # a GOP's pictures at two levels differ: the final level's frames are distinguishable from the first try's
    first = R.by_levels(c["frames"], c["W"], c["H"], c["pf"], [1, 1, 1])
    assert first[:3].tobytes() != c["recon"][:3].tobytes() and first[6:].tobytes() == c["recon"][6:].tobytes()
