"""-m gpu: m2v_decode_device on the streams of tests/dec_writer.py - what the oracle encoder never writes - byte for byte against
decoder.decode (the two streams decoder.py needs minutes for: against the host build, which tests/test_dec_cases.py holds to
decoder.py on them), and on every altered stream of tests/dec_cases.py against the host build's verdict.  Every decode goes through
test_gpu_decode.decode: 0xA5 guards around the frames, the capacity exactly the frames' bytes.  tests/test_dec_cases.py asserts from
the writer's log that each stream holds what its name says.  Which device-only path a test is for is in its docstring."""
import pytest

from test_gpu_decode import decode, same

pytestmark = pytest.mark.gpu
BOTH = ("module", "iso")


@pytest.fixture(scope="module")
def env():
    import dec_cases
    import dec_writer
    return dec_cases.M, dec_cases, dec_writer


@pytest.fixture(scope="module")
def enc(env):
    M, D, W = env
    e = M.Mpeg2Encoder(XL=6, YL=6)
    yield e
    e.close()


def small_again(M, D, W, enc, what):
    s = D.small()
    got, r = decode(M, D, enc, s, "i420", "module")
    same(got, W.expected(s, "module"), ("the valid decode behind", what))


@pytest.mark.parametrize("name", ("qcodes", "dc_range", "escapes", "saturate", "pmv_chain"))
def test_directed(env, enc, name):
    """quantiser codes 0 .. 31 with saturation either way; DC sizes 0 .. 11 and a predictor far outside 10 bits (MODULE does not
    saturate it, ISO clips F[0]); every run as an escape, index 63, an escape first in a non-intra block; blocks of 64 coefficients of
    +-2047 at codes 1, 16, 31 (the 32-bit wrap of Chen-Wang, the 18-bit row store); vector prediction carried, reset and wrapped both
    ways - both modes, all four layouts"""
    M, D, W = env
    s, _ = getattr(W, name)()
    for mode in BOTH:
        for layout in D.LAYOUTS:
            got, r = decode(M, D, enc, s, layout, mode)
            same(got, W.expected(s, mode, layout), (name, mode, layout))


def sizes():
    import dec_writer
    return dec_writer.SIZES


@pytest.mark.parametrize("w,h", sizes(), ids=lambda v: str(v))
def test_sizes(env, enc, w, h):
    """header sizes from 1 x 1 (13 frames of 3 bytes: five whole frames in one 16-byte store of k_dec_out) to 2048 x 16 and 16 x 2048,
    all four layouts, both modes; the small ones also 1, 7 and 15 bytes behind a 16-byte boundary"""
    M, D, W = env
    s, _ = W.sized(w, h)
    for mode in BOTH:
        for layout in D.LAYOUTS:
            want = W.expected(s, mode, layout)
            for dst_off in ((0, 1, 7, 15) if (w, h) in W.SMALL_SIZES else (0,)):
                got, r = decode(M, D, enc, s, layout, mode, dst_off=dst_off)
                same(got, want, (w, h, mode, layout, dst_off))
                assert (r["width"], r["height"], r["frame_bytes"]) == (w, h, M.frame_bytes(w, h, layout))


def test_sizes_refused(env, enc):
    """0 and 2049 in either dimension: M2V_DEC_SYNTAX at the first start code, nothing written"""
    M, D, W = env
    for w, h in ((0, 32), (32, 0), (2049, 32), (32, 2049)):
        x = W.bad_size(w, h)
        host = D.host_decode(x, "i420", "module")[1]
        got, r = decode(M, D, enc, x, "i420", "module", cap=1 << 14)
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, 0) == (host["status"], host["err_offset"])
    small_again(M, D, W, enc, "the sizes")


def test_many_pictures(env):
    """400 pictures of 32 x 16 in 11 104 bytes, 1 218 start codes: more than the event list's first guess, so k_dec_scan, k_dec_tiles
    and k_dec_plan run a second time; k_dec_plan judges five events a lane on every lane; the default "decode_batch" cuts it into
    chunks of 256 and 144 with I pictures at 255, 256 and 257; "decode_batch" 7 into 58 chunks"""
    M, D, W = env
    s, L = W.many_pictures()
    e = M.Mpeg2Encoder()
    try:
        for batch, mode, layout in ((0, "module", "i420"), (7, "module", "nv21"), (0, "iso", "nv12"), (7, "iso", "yv12")):
            e.set_option("decode_batch", batch)
            got, r = decode(M, D, e, s, layout, mode)
            same(got, W.expected(s, mode, layout), (batch, mode, layout))
            assert (r["pictures"], r["chains"], r["gops"], r["repeated_headers"]) == (400, len(W.MANY_I), len(W.MANY_I), 2)
        e.set_option("decode_batch", 0)
        small_again(M, D, W, e, "the second run of the scan")
    finally:
        e.close()


def test_big_chunk(env):
    """320 x 304, 256 pictures: one default chunk of 37 355 520 bytes, so k_dec_out's grid of 8192 blocks walks its loop twice.  The
    expectation is the host build's (decoder.py needs 200 s a mode: tests/test_dec_cases.py says what it checks instead)"""
    M, D, W = env
    s, L = W.big_chunk()
    e = M.Mpeg2Encoder()
    try:
        for layout, mode in (("i420", "module"), ("nv12", "iso")):
            want, host = D.host_decode(s, layout, mode)
            assert host["status"] == D.OK and want.size > 8192 * 256 * 16
            got, r = decode(M, D, e, s, layout, mode)
            same(got, want, (layout, mode))
            assert r["pictures"] == 256 and r["chains"] == 1
    finally:
        e.close()


def test_stuffed(env, enc):
    """zero stuffing puts a unit of every kind - sequence header, its two extensions, GOP header, picture header, its extension, a
    slice, the end code - at T - 3 .. T from a multiple of the scan's tile and at -3 .. 0 from a multiple of 16 inside one"""
    M, D, W = env
    for j, (s, _) in enumerate(W.stuffed(M.decode_scan_tile())):
        for mode, layout in (("module", "i420"), ("iso", "nv12")):
            got, r = decode(M, D, enc, s, layout, mode)
            same(got, W.expected(s, mode, layout), (j, mode))
            assert (r["pictures"], r["repeated_headers"], r["gops"]) == (3, 1, 2)


def test_stuffed_2mib(env, enc):
    """515 tiles: every block of k_dec_scan walks its loop over tiles twice or more, k_dec_tiles sums three tiles a lane; start codes
    in tiles 0, 511, 512, 513 and 514, the repeated sequence header in 514.  The expectation is the host build's (the CPU file holds it
    to decoder.py on this stream)"""
    M, D, W = env
    s, _ = W.stuffed_2mib(M.decode_scan_tile())
    for mode in BOTH:
        want, host = D.host_decode(s, "i420", mode)
        got, r = decode(M, D, enc, s, "i420", mode)
        same(got, want, mode)
        assert (r["pictures"], r["repeated_headers"], r["gops"], r["es_bytes"]) == (3, 1, 2, len(s)) and host["repeated_headers"] == 1


def verdicts(M, D, W, enc, cases):
    """every (name, stream, mode): status and err_offset are the host build's, the frames too where it accepts (decode() asserts that
    nothing is written otherwise); a valid decode of small() behind every hundredth and the last.  -> (refused, accepted)"""
    cap = 1 << 14
    refused = accepted = 0
    for k, (name, x, mode) in enumerate(cases):
        want, host = D.host_decode(x, "i420", mode, cap=cap)
        got, r = decode(M, D, enc, x, "i420", mode, cap=cap)
        assert (r["status"], r["err_offset"], r["out_bytes"]) == (host["status"], host["err_offset"], host["out_bytes"]), (name, mode, r, host)
        if host["status"] == D.OK:
            same(got, want, (name, mode))
            accepted += 1
        else:
            assert got is None
            refused += 1
        if k % 100 == 99 or k + 1 == len(cases):
            small_again(M, D, W, enc, name)
    return refused, accepted


@pytest.mark.parametrize("group", ("slice_module", "slice_iso", "header_flips"))
def test_altered_streams(env, enc, group):
    """all 500 of dec_cases.altered() in MODULE mode, every other one in ISO mode, every bit flip of small()'s headers in MODULE mode -
    1 222 verdicts of one handle against the host build's (k_dec_plan judges in parallel ranges and takes a minimum; the host build
    walks the events in order)"""
    M, D, W = env
    s = D.small()
    if group == "header_flips":
        cases = [("bit%d" % b, D.flip(s, b), "module") for b in range(8 * D.first_slice(s))]
    else:
        cases = [(name, x, group[6:]) for name, x in D.altered()[::1 if group == "slice_module" else 2]]
    refused, accepted = verdicts(M, D, W, enc, cases)
    assert refused and accepted and refused + accepted == len(cases) >= 250


def test_written_refusals(env, enc):
    """index 64, escape levels 0 and -2048, end of block first, macroblock type '01', an address increment of 2, a vector half a sample
    outside at each edge, slice code mbh + 1, nonzero slice stuffing - and a P picture without a reference, the rule that lives in
    k_dec_plan alone: behind a repeated sequence header at the very start, and 150 of them, every lane reporting its own"""
    M, D, W = env
    cases = [(name, x, mode) for name, x in W.refusals().items() for mode in BOTH]
    refused, accepted = verdicts(M, D, W, enc, cases)
    assert accepted == 0 and refused == len(cases)
