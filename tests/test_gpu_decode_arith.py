"""-m gpu: the arithmetic of the main-syntax decoder through every copy of the device's reconstruction kernel, against the plain
reference of tests/arith_ref.py - frames computed from a log by formulas written from the standard's text, which
tests/test_arith_cases.py shows to be the definition's (decoder.decode(..., syntax="main")) byte for byte on every stream here, and
which that file shows to change when any one of the rules is bent.  No tolerance anywhere except the statistics of Annex A.

m2v_decode_device picks its kernels by the options: none k_dm_recon, "decode_b_pictures" k_db_recon, "decode_interlaced" k_di_recon,
"decode_extended" k_dx_recon; m2v_decode_streams_main_device runs k_dsm_recon.  Every decode is a probe for the size, then a decode
into exactly that much, inside a buffer of FILL with guards, from a source and to a destination that are not aligned, the four layouts
going round."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MAIN = 1
GAP = b"\x00\x00\x01"


@pytest.fixture(scope="module")
def env():
    import arith_cases as A
    import decstreams_main_cases as S
    return A.M, A.D, A, S


@pytest.fixture(scope="module")
def enc(env):
    M, D, A, S = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    e.set_option("decode_syntax", MAIN)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(a), np.uint8).copy()).to("cuda:0")


def decode(env, enc, stream, b, i, x, layout="i420", es_off=0, dst_off=0):
    """one m2v_decode_device through the C-ABI -> the frames [pictures, frame bytes]; asserts OK, the probe's sizes and the guards"""
    import torch
    M, D, A, S = env
    enc.set_option("decode_b_pictures", int(bool(b)))
    enc.set_option("decode_interlaced", int(bool(i)))
    enc.set_option("decode_extended", int(bool(x)))
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(stream)])
    assert enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), None, 0, M.LAYOUTS_420[layout], D.MODES["iso"], None) == 0
    r0 = enc.decode_report()
    assert r0["status"] == D.OK, r0
    room = int(r0["pictures"]) * int(r0["frame_bytes"])
    buf = torch.full((2 * D.GUARD + dst_off + room + 16,), D.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc = enc._L.m2v_decode_device(enc._h, es.data_ptr() + es_off, len(stream), buf.data_ptr() + D.GUARD + dst_off, room, M.LAYOUTS_420[layout], D.MODES["iso"], None)
    assert rc == 0, enc._L.m2v_last_error(enc._h)
    r = enc.decode_report()
    got = buf.cpu().numpy()
    lo, hi = D.GUARD + dst_off, D.GUARD + dst_off + room
    assert r["status"] == D.OK and int(r["out_bytes"]) == room, r
    assert (got[:lo] == D.FILL).all() and (got[hi:] == D.FILL).all(), "bytes outside the frames were written"
    return got[lo:hi].reshape(int(r["pictures"]), int(r["frame_bytes"]))


def decode_streams(env, enc, batch, flags, layout="i420", es_off=0, dst_off=0):
    """one m2v_decode_streams_main_device on the batch -> the frames of every stream; asserts OK for each, and the guards"""
    import torch
    M, D, A, S = env
    data, seg = S.place(batch, GAP, lead=1)
    es = torch.cat([torch.zeros(es_off, dtype=torch.uint8, device="cuda:0"), dev(data)])
    off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
    nb = (ctypes.c_uint64 * len(seg))(*[n for _, n in seg])
    call = lambda dst, cap: enc._L.m2v_decode_streams_main_device(enc._h, es.data_ptr() + es_off, off, nb, len(seg), dst, cap, M.LAYOUTS_420[layout], flags, None)
    assert call(None, 0) == 0, enc._L.m2v_last_error(enc._h)
    r0 = S.records_of(enc.decode_streams_report())
    assert all(r["status"] == D.OK for r in r0), r0
    total = max(r["out_offset"] + r["out_bytes"] for r in r0)
    buf = torch.full((2 * S.GUARD + dst_off + total + 16,), S.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert call(buf.data_ptr() + S.GUARD + dst_off, total) == 0, enc._L.m2v_last_error(enc._h)
    recs = S.records_of(enc.decode_streams_report())
    got = buf.cpu().numpy()
    lo = S.GUARD + dst_off
    assert (got[:lo] == S.FILL).all() and (got[lo + total:] == S.FILL).all(), "bytes outside the rooms were written"
    out = []
    for r in recs:
        assert r["status"] == D.OK, r
        out.append(got[lo + r["out_offset"]:lo + r["out_offset"] + r["out_bytes"]].reshape(r["pictures"], r["frame_bytes"]))
    return out


def names():
    import arith_cases
    return arith_cases.NAMES


@pytest.mark.parametrize("name", names())
def test_every_case_through_every_kernel_copy(env, enc, name):
    """a case under every setting of "decode_b_pictures" x "decode_interlaced" x "decode_extended" that accepts its stream - eight for a
    stream of progressive I and P pictures: k_dm_recon, k_db_recon, k_di_recon and k_dx_recon all meet it - gives the plain
    reference's bytes"""
    M, D, A, S = env
    c = A.CASES[name]()
    settings = A.settings(c)
    assert len(settings) == 8 >> (c["b"] + c["i"] + c["x"])
    for k, (b, i, x) in enumerate(settings):
        at = names().index(name) + k
        layout = D.LAYOUTS[at & 3]
        got = decode(env, enc, c["stream"], b, i, x, layout, es_off=at % 5, dst_off=(3 * at + 1) % 7)
        want = A.expected_in(name, layout)
        assert got.shape == want.shape and np.array_equal(got, want), (name, b, i, x, np.nonzero(got.reshape(-1) != want.reshape(-1))[0][:8])


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_every_case_in_one_batch(env, enc, flags):
    """every case whose stream the flags accept (quant_matrix_extension has no flag there) in one call of
    m2v_decode_streams_main_device: k_dsm_recon on all of them side by side"""
    M, D, A, S = env
    batch = [n for n in names() if not A.CASES[n]()["x"] and A.CASES[n]()["b"] <= (flags & 1) and A.CASES[n]()["i"] <= (flags >> 1 & 1)]
    assert len(batch) == 13 + (flags & 1) + (flags >> 1 & 1)
    layout = D.LAYOUTS[flags]
    got = decode_streams(env, enc, [A.CASES[n]()["stream"] for n in batch], flags, layout, es_off=flags + 1, dst_off=2 * flags + 1)
    for n, g in zip(batch, got):
        want = A.expected_in(n, layout)
        assert g.shape == want.shape and np.array_equal(g, want), (n, flags)


def test_decode_batch(env, enc):
    """"decode_batch" 1 and 3 on b_mean (chunks that end between a B picture and its anchors) and, under "decode_extended", on
    weights_1_255 with its matrices from a quant_matrix_extension"""
    M, D, A, S = env
    try:
        for batch in (1, 3):
            enc.set_option("decode_batch", batch)
            for name, (b, i, x) in (("b_mean", (True, False, False)), ("b_mean", (True, True, True)), ("weights_1_255_qme", (False, False, True)),
                                    ("weights_1_255_qme", (True, False, True))):
                got = decode(env, enc, A.CASES[name]()["stream"], b, i, x, dst_off=batch)
                assert np.array_equal(got, A.expected_in(name)), (name, batch, b, i, x)
    finally:
        enc.set_option("decode_batch", 0)


def test_annex_a(env, enc):
    """the accuracy stream (tests/test_arith_cases.py::test_annex_a has the figures and the counts) through k_dm_recon and through
    k_dsm_recon: the criteria of Annex A on the device's samples, all-zero in all-zero out, and the bytes of the plain reference,
    which that test shows to be the definition's"""
    M, D, A, S = env
    a = A.accuracy()
    want = A.R.flat(A.R.frames(a["log"]))
    assert tuple(int(v) for v in A.accuracy_excluded().sum(axis=(1, 2, 3))) == (637, 635, 0, 0, 10007, 10007)
    for name, got in (("k_dm_recon", decode(env, enc, a["stream"], False, False, False, dst_off=3)),
                      ("k_dsm_recon", decode_streams(env, enc, [a["stream"]], 0, dst_off=5)[0])):
        fig = A.accuracy_figures(A.accuracy_residuals(got))
        print(name, {k: np.round(v, 5).tolist() for k, v in fig.items()})
        assert A.accuracy_within(fig), (name, fig)
        assert A.accuracy_uncoded_ok(got), name
        assert np.array_equal(got, want), name
