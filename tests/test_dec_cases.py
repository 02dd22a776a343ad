"""The device decoder on the CPU: csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_host.hpp, compiled with g++, against
decoder.py - valid streams frame for frame and count for count, every VLC function, both inverse transforms, the dequantisers and the
vector wrap unit by unit, refusals on altered streams exactly where the definition refuses, the scan's tile boundaries, and the whole
host build once more under AddressSanitizer and UBSan as a stand-alone program.  tests/test_gpu_decode.py runs the same streams on the
device.  The streams of tests/dec_writer.py - what the oracle encoder never writes - are asserted here from the writer's log to hold
what their names say, go through the same checks, and catch ten one-line changes of the header each by a named case;
tests/test_gpu_decode_streams.py runs them on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dec_cases as D
import dec_writer as W
import transform_clips as T

M = D.M
BOTH = (("module", True), ("iso", False))


def check_valid(stream, modes=BOTH, layout="i420"):
    for mode, quirks in modes:
        d = M.decoder.decode(stream, quirks=quirks)
        f, r = D.host_decode(stream, layout, mode)
        assert r["status"] == D.OK, (mode, r)
        assert np.array_equal(f, D.frames_of(d, layout)), mode
        want = dict(pictures=len(d.pictures), gops=len(d.gops), width=d.width, height=d.height, repeated_headers=d.repeated_headers,
                    chains=sum(p["type"] == 1 for p in d.pictures), es_bytes=len(stream), frame_bytes=M.frame_bytes(d.width, d.height, "i420"))
        assert {k: r[k] for k in want} == want
        assert r["out_bytes"] == r["pictures"] * r["frame_bytes"]


def test_record_is_the_headers():
    assert ctypes.sizeof(D.Stat) == 72 == M.DECODE_STAT_DTYPE.itemsize
    assert [n for n, _ in D.Stat._fields_] == list(M.DECODE_STAT_DTYPE.names)
    hdr = open(os.path.join(D.ROOT, "include", "m2v_mi355x.h")).read()
    for word in ("m2v_decode_device", "m2v_decode_report", "m2v_decode_scan_tile", "M2V_DEC_ISO = 0", "M2V_DEC_MODULE = 1", "M2V_DEC_SYNTAX = -2",
                 "M2V_DEC_OVERFLOW = -3"):
        assert word in hdr
    assert D.host_lib().dec_host_scan_tile() == 4096


@pytest.mark.parametrize("name", D.recon_names())
def test_recon_streams(name):
    """every stream of recon_cases.gpu_cases(), the fit cases also with the true size in the header: decoder.py in both modes, and the
    oracle's dump in the stream's own mode, every layout"""
    assert D.recon_names() == sorted(D.recon_streams())
    c = D.recon_streams()[name]
    check_valid(c["stream"])
    mode = "iso" if c["conformant"] else "module"
    for layout in D.LAYOUTS:
        f, r = D.host_decode(c["stream"], layout, mode)
        assert r["status"] == D.OK and np.array_equal(f, D.expected_from_dump(c, layout)), layout


def test_described_stream_with_repeated_headers():
    s = D.described()
    assert M.decoder.decode(s).repeated_headers >= 1
    check_valid(s)


@pytest.mark.parametrize("name", D.twin_names())
def test_twin_streams(name):
    """the recon, fit and described streams in their other encoding (dec_cases.twin_streams says which, and why not the spliced ones)"""
    assert D.twin_names() == sorted(D.twin_streams())
    check_valid(D.twin_streams()[name])


@pytest.mark.parametrize("conformant", (False, True), ids=("plain", "conformant"))
@pytest.mark.parametrize("fc", D.clip_cases(), ids=D.clip_id)
def test_clip_streams(fc, conformant):
    check_valid(D.clip_stream(fc[0], fc[1], conformant))


# ---- unit by unit ----
def _reference_vlc(entries, w, bits):
    """what decoder._vlc_decoder reads at the front of the `bits`-bit window w: (length, symbol) or None"""
    for code, length, sym in entries:
        if length <= bits and (w >> (bits - length)) == code:
            return length, sym
    return None


@pytest.mark.parametrize("which,name,bits", ((0, "motion", 12), (1, "cbp", 12), (2, "dcy", 12), (3, "dcc", 12), (4, "ac", 17)))
def test_vlc_functions(which, name, bits):
    """every entry of decoder.iso_tables(), and every window of `bits` bits (longer than the longest code): the same length and symbol,
    or no code"""
    t = M.decoder.iso_tables()
    entries = list(t[name])
    if name == "ac":
        entries += [(0b10, 2, "EOB"), (0b000001, 6, "ESC")]
    L = D.host_lib()

    def unpack(v):
        if not v:
            return None
        if name != "ac":
            return v & 255, v >> 8
        run, lvl = (v >> 8) & 255, v >> 16
        return v & 255, ("EOB" if run == 0 else "ESC") if lvl == 0 else (run, lvl)
    for code, length, sym in entries:
        for tail in (0, (1 << (32 - length)) - 1, 0x55555555 >> length):
            assert unpack(L.dec_host_vlc(which, (code << (32 - length)) | tail)) == (length, sym)
    by_len = {}
    for e in entries:
        by_len.setdefault(e[1], {})[e[0]] = e[2]
    step = 1 if bits <= 12 else 3                                  # (every third 17-bit window: 43 691 of them)
    for w in range(0, 1 << bits, step):
        want = None
        for length, codes in by_len.items():
            sym = codes.get(w >> (bits - length))
            if sym is not None:
                want = (length, sym)
                break
        assert unpack(L.dec_host_vlc(which, w << (32 - bits))) == want, bin(w)
    assert [L.dec_host_table(0, k) for k in range(64)] == [int(v) for v in M.decoder.tables()["zz"]]
    assert [L.dec_host_table(1, k) for k in range(64)] == t["intra_w"]


def _over_blocks():
    x = np.array(T.OVER_BLOCKS, np.int64).reshape(-1, 64) - 128
    q = T.o_quant(T.o_fdct(x), False, T.OVER_Q)
    return [T.o_dequant(q, False, T.OVER_Q, conformant=c) for c in (False, True)]


def test_idct_both_variants():
    L = D.host_lib()
    rng = np.random.RandomState(3)
    blocks = np.concatenate(_over_blocks() + [rng.randint(-2048, 2048, size=(1000, 64))])
    sparse = rng.randint(-2048, 2048, size=(200, 64)) * (rng.randint(0, 8, size=(200, 64)) == 0)
    for mode, quirks in BOTH:
        for blk in np.concatenate([blocks, sparse]):
            f = np.ascontiguousarray(blk, np.int32)
            L.dec_host_idct(f.ctypes.data, D.MODES[mode])
            assert np.array_equal(f, M.decoder.idct(blk, quirks)), (mode, blk)


@pytest.mark.parametrize("qcode", (2, 4, 8, 16))
def test_dequant(qcode):
    """every level -2047 .. 2047 at every one of the 64 positions, intra and non-intra, both modes, against _dequant block by block: the
    4095 levels in 64 blocks of 64 different ones (the last holds 63 and the first again), each block rotated through all 64 positions
    - 4096 blocks for each of mode x intra, mismatch control included"""
    L = D.host_lib()
    W = np.array(M.decoder.iso_tables()["intra_w"], np.int64)
    levels = np.arange(-2047, 2048)
    seen = np.zeros((4095, 64), bool)
    for mode, quirks in BOTH:
        for intra in (True, False):
            for k in range(0, len(levels), 64):
                base = np.resize(levels[k:k + 64], 64)
                q = np.ascontiguousarray(np.stack([np.roll(base, shift) for shift in range(64)]), np.int32)
                f = np.zeros_like(q)
                L.dec_host_dequant_many(q.ctypes.data, 64, int(intra), qcode, D.MODES[mode], f.ctypes.data)
                for shift in range(64):
                    assert np.array_equal(f[shift], M.decoder._dequant(q[shift].astype(np.int64), intra, 2 * qcode, W, quirks)), (mode, intra, k, shift)
                seen[q + 2047, np.arange(64)[None, :]] = True
    assert seen.all()


def test_vector_wrap():
    """7.6.3.1 as decoder.decode states it, for every prediction and every delta"""
    L = D.host_lib()
    for pmv in range(-16, 16):
        for delta in range(-16, 17):
            v = pmv + delta
            v = v + 32 if v < -16 else v - 32 if v > 15 else v
            assert L.dec_host_wrap(pmv, delta) == v


# ---- refusals ----
def _judge(cases):
    """-> (refused, accepted, decided by the prefix rule); asserts the host build's answer on every case, in both modes"""
    refused = accepted = prefix = 0
    for name, x in cases:
        for mode, quirks in BOTH:
            d, why = D.spec(x, quirks)
            f, r = D.host_decode(x, "i420", mode)
            if d is None:
                assert r["status"] == D.SYNTAX and r["out_bytes"] == 0, (name, mode, why, r)
                refused += 1
                prefix += why == "prefix"
            else:
                assert r["status"] == D.OK and np.array_equal(f, D.frames_of(d)), (name, mode, r)
                accepted += 1
    return refused, accepted, prefix


def test_header_bit_flips():
    s = D.small()
    refused, accepted, prefix = _judge([("bit%d" % b, D.flip(s, b)) for b in range(8 * D.first_slice(s))])
    print("header flips: %d refused, %d accepted, %d by the prefix rule" % (refused, accepted, prefix))
    assert refused and accepted and prefix <= 0.01 * (refused + accepted)


def test_slice_alterations():
    cases = D.altered()
    flips = [c for c in cases if c[0].startswith("flip")]
    assert len(flips) == 400 and len(cases) == 500
    refused, accepted, prefix = _judge(flips)
    print("slice flips: %d refused, %d accepted, %d by the prefix rule" % (refused, accepted, prefix))
    assert refused >= 0.3 * (refused + accepted) and accepted >= 0.1 * (refused + accepted)
    r2, a2, p2 = _judge(cases[400:])
    print("truncations and insertions: %d refused, %d accepted, %d by the prefix rule" % (r2, a2, p2))
    assert prefix + p2 <= 0.01 * (refused + accepted + r2 + a2)


def test_handmade_refusals():
    cases = list(D.handmade().items()) + list(D.truncations().items())
    assert len(cases) == 9
    refused, accepted, _ = _judge(cases)
    assert accepted == 0 and refused == 2 * len(cases)
    s = D.small()
    f, r = D.host_decode(s, "i420", "module", cap=2 * 1536 - 1)
    assert f is None and r["status"] == D.OVERFLOW and r["out_bytes"] == 0
    assert D.host_decode(s, "i420", "module", cap=2 * 1536)[1]["status"] == D.OK


def test_zero_runs():
    """runs of zeros (and one byte that is not) in front of the first start code and behind every unit, at lengths around the
    eight-byte steps in which the stuffing is checked - whatever the definition says of each"""
    s = D.small()
    cases = []
    for k in (1, 7, 8, 9, 15, 16, 17, 32, 64):
        cases += [("lead%d" % k, bytes(k) + s + bytes(-k % 32)), ("lead%d_80" % k, b"\x80" + bytes(k - 1) + s + bytes(-k % 32))]
        for j, (at, code) in enumerate(D._units(s)[1:]):
            if j % 3 == k % 3:
                cases += [("z%d_%d" % (k, at), s[:at] + bytes(k) + s[at:] + bytes(-k % 32)), ("n%d_%d" % (k, at), s[:at] + b"\x40" + bytes(k - 1) + s[at:] + bytes(-k % 32))]
    refused, accepted, _ = _judge(cases)
    assert refused and accepted


# ---- the scan's tile ----
def test_scan_tile_streams():
    streams = D.tile_streams()
    assert D.tile_census(streams, D.host_lib().dec_host_scan_tile()) == {"T-3", "T-2", "T-1", "T", "slice", "picture", "sequence"}
    for s in streams:
        check_valid(s, modes=BOTH[:1])
    for s in D.tile_streams(conformant=True):
        check_valid(s, modes=BOTH[1:])


def test_two_bad_slices():
    """two refused slices 141 slices apart: the offset is the earlier one's (the device walks them in different blocks, and
    tests/test_gpu_decode.py holds it to this answer)"""
    x, at = D.two_bad_slices()
    check_valid(D.ionly_stream(), modes=BOTH[:1])
    for mode, quirks in BOTH:
        assert D.spec(x, quirks) == (None, "raise")
        f, r = D.host_decode(x, "i420", mode)
        assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, at, 0)


# ---- the written streams (tests/dec_writer.py): what the oracle encoder never writes ----
BAD_SIZES = ((0, 32), (32, 0), (2049, 32), (32, 2049))


def check_layouts(stream):
    """decoder.py against the host build in both modes and all four layouts"""
    check_valid(stream)
    for mode, quirks in BOTH:
        d = M.decoder.decode(stream, quirks=quirks)
        for layout in D.LAYOUTS[1:]:
            f, r = D.host_decode(stream, layout, mode)
            assert r["status"] == D.OK and np.array_equal(f, D.frames_of(d, layout)), (mode, layout)


def _dequantised(intra, k, lvl, code):
    """7.4.2 in front of the saturation, for the coefficient at scan position k"""
    t = W._tabs()
    if intra:
        return 2 * lvl * t["intra_w"][t["raster"][k]] * 2 * code / 32
    return (2 * lvl + (1 if lvl > 0 else -1)) * 16 * 2 * code / 32


def test_written_qcodes():
    s, L = W.qcodes()
    assert L["pictures"] == [1, 2] and L["qcodes"] == [list(range(32))] * 2 and [k for k, _ in L["units"]].count("slice") == 64
    assert len(L["blocks"]) == 64 * 6
    for n, (intra, comp, levels) in enumerate(L["blocks"]):
        code = (n // 6) % 32
        assert intra == (n < 32 * 6)
        f = [_dequantised(intra, k, lvl, code) for k, lvl in levels]
        if code >= 17:
            assert max(f) > 2047 and min(f) < -2048 and sum(v > 2047 for v in f) >= 2 and sum(v < -2048 for v in f) >= 2
        if 1 <= code <= 16:
            assert abs(f[0]) <= 2047 and abs(f[1]) <= 2047 and f[0] == -f[1]      # the pair of +-61 / +-60 does not saturate up to code 16
    check_layouts(s)
    d = M.decoder.decode(s, quirks=True)
    assert d.slice_qcodes == [list(range(32))] * 2


def test_written_dc_range():
    s, L = W.dc_range()
    got = {(comp != 0, size, sign) for comp, size, sign, _, _, _ in L["dc"]}
    assert got == {(c, size, sign) for c in (False, True) for size in range(1, 12) for sign in (-1, 1)} | {(False, 0, 0), (True, 0, 0)}
    for comps in ((0,), (1, 2)):
        behind = [p for comp, _, _, p, _, _ in L["dc"] if comp in comps]
        assert max(behind) > 4096 and min(behind) < -4096
    # the resets: behind a non-intra macroblock between two intra ones, and at a slice start
    mbs = L["mbs"]
    first = {m: [e for e in L["dc"] if e[5] == m][0] for m in range(len(mbs)) if mbs[m]["kind"] == "intra"}
    last = {m: [e for e in L["dc"] if e[5] == m and e[0] == 0][-1] for m in first}
    between = [m for m in first if m >= 2 and mbs[m]["col"] >= 2 and mbs[m - 1]["kind"] == "coded" and mbs[m - 2]["kind"] == "intra" and mbs[m]["pic"] == 1]
    assert between and all(last[m - 2][3] != 0 and first[m][4] == 0 for m in between)
    starts = [m for m in first if mbs[m]["col"] == 0 and mbs[m]["row"] == 1 and mbs[m - 1]["kind"] == "intra"]
    assert len(starts) == 3 and all(last[m - 1][3] != 0 and first[m][4] == 0 for m in starts)
    check_layouts(s)


def test_written_escapes():
    s, L = W.escapes()
    esc = L["esc"]
    assert {(run, lvl) for run, lvl, _, _, _, _ in esc} >= {(run, lvl) for run in range(64) for lvl in (1, -1, 2047, -2047)}
    assert sum(coded for _, _, _, _, _, coded in esc) >= 64                       # escapes of pairs that have a table code
    assert any(intra and k == 63 for _, _, intra, _, k, _ in esc) and any(not intra and k == 63 for _, _, intra, _, k, _ in esc)
    assert sum(first and not intra for _, _, intra, first, _, _ in esc) >= 160 and sum(intra for _, _, intra, _, _, _ in esc) == 96
    assert any(run == 63 and first for run, _, _, first, _, _ in esc)
    check_layouts(s)


def test_written_saturate():
    s, L = W.saturate()
    assert L["qcodes"] == [[1, 16, 31]] * 2 and len(L["blocks"]) == 36
    raster = W._tabs()["raster"]
    dcs = iter(L["dc"])
    for n, (intra, comp, levels) in enumerate(L["blocks"]):
        assert intra == (n < 18)
        sign = list(W.SIGNS.values())[n % 6]
        want = {k: 2047 * sign(raster[k] & 7, raster[k] >> 3) for k in range(64)}
        have = dict(levels)
        if intra:
            e = next(dcs)
            have[0] = e[2] * 2047
            assert e[1] == 11
        assert have == want
    assert len({tuple(lvl for k, lvl in levels if k >= 4) for _, _, levels in L["blocks"]}) == 6
    check_layouts(s)


def test_written_pmv_chain():
    s, L = W.pmv_chain()
    mbs = L["mbs"]
    assert L["pictures"] == [1, 2, 2] and len(mbs) == 27
    assert {(c, m["wrap"][c]) for m in mbs for c in (0, 1) if m["wrap"][c]} == {(0, 1), (0, -1), (1, 1), (1, -1)}
    assert any(m["wrap"][c] == 1 and m["pmv"][c] == 15 and m["delta"][c] > 0 for m in mbs for c in (0, 1))
    assert any(m["wrap"][c] == -1 and m["pmv"][c] == -16 and m["delta"][c] < 0 for m in mbs for c in (0, 1))
    moved = lambda m: m["kind"] != "intra" and m["mv"] != (0, 0)
    carried = [k for k in range(1, 27) if mbs[k]["col"] and mbs[k]["kind"] == mbs[k - 1]["kind"] == "not_coded" and moved(mbs[k - 1]) and mbs[k]["pmv"] == mbs[k - 1]["mv"]]
    assert len(carried) >= 3 and any(mbs[k]["delta"] == (0, 0) for k in carried)
    behind_intra = [k for k in range(11, 27) if mbs[k]["col"] == 2 and mbs[k - 1]["kind"] == "intra" and moved(mbs[k - 2])]
    assert behind_intra and all(mbs[k]["pmv"] == (0, 0) and moved(mbs[k]) for k in behind_intra)
    starts = [k for k in range(10, 27) if mbs[k]["col"] == 0 and mbs[k]["row"] and moved(mbs[k - 1])]
    assert len(starts) >= 3 and all(mbs[k]["pmv"] == (0, 0) and moved(mbs[k]) for k in starts)
    check_layouts(s)
    for quirks in (True, False):
        assert [m["mv"] for m in sum(M.decoder.decode(s, quirks=quirks).mbs, [])] == [m["mv"] for m in mbs]


@pytest.mark.parametrize("w,h", W.SIZES, ids=lambda v: str(v))
def test_written_sizes(w, h):
    s, L = W.sized(w, h)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    assert [k for k, _ in L["units"]].count("slice") == mbh * len(L["pictures"]) and len(L["mbs"]) == mbw * mbh * len(L["pictures"])
    assert M.decoder.sequence_headers(s)[:2] == (w, h)
    if (w, h) == (1, 1):
        assert len(L["pictures"]) >= 12 and M.frame_bytes(1, 1, "i420") == 3 and {1, 2} == set(L["pictures"])
    check_layouts(s)


def test_sizes_outside_the_device():
    """0 and 2049 in either dimension: the device decodes 1 .. 2048 (include/m2v_mi355x.h), the host build says where"""
    for w, h in BAD_SIZES:
        x = W.bad_size(w, h)
        for mode in ("module", "iso"):
            f, r = D.host_decode(x, "i420", mode)
            assert f is None and (r["status"], r["err_offset"], r["out_bytes"]) == (D.SYNTAX, 0, 0), (w, h, r)


def test_written_many_pictures():
    s, L = W.many_pictures()
    assert len(L["pictures"]) == 400 > 256 and [k for k, t in enumerate(L["pictures"]) if t == 1] == list(W.MANY_I) and {255, 256, 257} <= set(W.MANY_I)
    # more start codes than the event list decode_impl (csrc/m2v_decode.hip) guesses first: max(1024, n / 16 + 64) - the scan runs twice
    assert len(L["units"]) == D.prefixes(s) > max(1024, len(s) // 16 + 64)
    p = [m for m in L["mbs"] if L["pictures"][m["pic"]] == 2]
    assert len(p) == 2 * (400 - len(W.MANY_I)) and all(m["kind"] == "not_coded" and m["mv"] != (0, 0) and abs(m["mv"][0]) <= 4 for m in p)
    check_valid(s)
    assert M.decoder.decode(s).repeated_headers == 2


def _source(name):
    return open(os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc", name)).read()


def test_written_big_chunk():
    """One default chunk of more than 8192 x 256 x 16 bytes.  decoder.py would need 200 s a mode for the 97 280 macroblocks, so: the
    host build against decoder.py on the stream's first two pictures (the I picture and the first P picture, closed with an end code),
    both modes; then the host build's frames 2, 3, 128 and 255 of the whole stream against decoder._predict applied to the frame in
    front with the writer's vectors.  The GPU test takes the host build's frames"""
    import re
    s, L = W.big_chunk()
    src = _source("m2v_decode.hip")
    level_bytes = re.search(r"kDecLevelBytes = (\d+)u << (\d+);", src)
    batch_max = int(re.search(r"kDecBatchMax = (\d+);", src).group(1))
    level_bytes = int(level_bytes.group(1)) << int(level_bytes.group(2))
    w, h, n = W.BIG["w"], W.BIG["h"], W.BIG["n"]
    mbw, mbh = w // 16, h // 16
    assert "std::min(kDecBatchMax, kDecLevelBytes / (mbs * 768))" in src
    assert min(batch_max, level_bytes // (mbw * mbh * 768)) == 256 == n == len(L["pictures"])
    assert n * M.frame_bytes(w, h, "i420") > 8192 * 256 * 16 and L["pictures"] == [1] + [2] * 255
    assert len({tuple(m["mv"] for m in L["mbs"][k * mbw * mbh:(k + 1) * mbw * mbh]) for k in range(1, n)}) >= 5
    s2, L2 = W.big_chunk(2)
    assert s2[:len(s2) - 64] == s[:len(s2) - 64]
    check_valid(s2)
    for mode, quirks in BOTH:
        f, r = D.host_decode(s, "i420", mode)
        assert r["status"] == D.OK and f.shape == (n, M.frame_bytes(w, h, "i420"))
        assert np.array_equal(f[:2], D.host_decode(s2, "i420", mode)[0])
        for k in (2, 3, 128, 255):
            y, u, v = (a.astype(np.int64) for a in M.planes_of_recon(f[k - 1:k], w, h, "i420"))
            y, u, v = y[0], u[0], v[0]
            Y, U, V = np.zeros_like(y), np.zeros_like(u), np.zeros_like(v)
            for m in L["mbs"][k * mbw * mbh:(k + 1) * mbw * mbh]:
                assert m["pic"] == k and m["kind"] == "not_coded"
                col, row, mv = m["col"], m["row"], m["mv"]
                cmv = (mv[0] >> 1, mv[1] >> 1) if quirks else (int(mv[0] / 2), int(mv[1] / 2))
                Y[16 * row:16 * row + 16, 16 * col:16 * col + 16] = M.decoder._predict(y, 16 * col, 16 * row, mv[0], mv[1], 16, quirks)
                U[8 * row:8 * row + 8, 8 * col:8 * col + 8] = M.decoder._predict(u, 8 * col, 8 * row, cmv[0], cmv[1], 8, quirks)
                V[8 * row:8 * row + 8, 8 * col:8 * col + 8] = M.decoder._predict(v, 8 * col, 8 * row, cmv[0], cmv[1], 8, quirks)
            assert np.array_equal(f[k], np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint8)), (mode, k)


def test_written_stuffed():
    T = D.host_lib().dec_host_scan_tile()
    streams = W.stuffed(T)
    where = ("T-3", "T-2", "T-1", "T", "16-3", "16-2", "16-1", "16")
    assert D.tile_census([s for s, _ in streams], T, by_kind=True) >= {(kind, at) for kind in D.UNIT_KINDS for at in where}
    for j, (s, L) in enumerate(streams):
        assert [a for _, a in L["units"]] == [a for a, _ in D._units(s)] and [k for k, _ in L["units"]] == [k for _, k in D.unit_kinds(s)]
        for kind in D.UNIT_KINDS:                                # from the writer's log: the last unit of the kind is where stream j puts it
            at = [a for k, a in L["units"] if k == kind][-1]
            assert (at - (j % 4 - 3)) % (T if j < 4 else 16) == 0 and (j < 4) == ((at + 3) % T < 4)
        check_valid(s)
    # the existing census, on the new streams too
    assert D.tile_census([s for s, _ in streams], T) >= {"T-3", "T-2", "T-1", "T"}


def test_written_stuffed_2mib():
    """The full stream through decoder.py in MODULE mode only (20 s of zeros); in ISO mode the host build on the full stream against
    decoder.py on the same units written without stuffing"""
    T = D.host_lib().dec_host_scan_tile()
    s, L = W.stuffed_2mib(T)
    assert len(s) > 2 << 20 and len(s) > 512 * T
    tiles = {a // T for _, a in L["units"]}
    assert min(tiles) == 0 and 511 in tiles and {512, 513, 514} <= tiles
    assert [a // T for k, a in L["units"] if k == "sequence"] == [0, 514]
    census = D.tile_census([s], T, by_kind=True)
    assert ("picture", "T-3") in census and {("tile", 0), ("tile", 511), ("tile", 512), ("tile", 514)} <= census
    check_valid(s, modes=BOTH[:1])
    plain, _ = W.stuffed_2mib(T, stuffing=False)
    assert len(plain) < 1024
    check_valid(plain)
    f, r = D.host_decode(s, "i420", "iso")
    assert r["status"] == D.OK and r["repeated_headers"] == 1 and np.array_equal(f, D.frames_of(M.decoder.decode(plain, quirks=False)))


def test_written_refusals():
    """refused by the definition in both modes, and the host build names the unit the writer put the fault into"""
    cases = list(W.refusals().items())
    assert len(cases) == 17 and set(W.REFUSED_IN) | {"slice_code_mbh_plus_1", "p_behind_repeated_header", "p_pictures_only"} == set(W.refusals())
    refused, accepted, _ = _judge(cases)
    assert accepted == 0 and refused == 2 * len(cases)
    for name, x in cases:
        u = D._units(x)
        if name.startswith("p_"):                                # no reference: the first picture header
            want = [a for a, c in u if c == 0x00][0]
            assert len(u) == (455 if name == "p_pictures_only" else 11)
        elif name == "slice_code_mbh_plus_1":
            want = [a for a, c in u if c == 3][0]
        else:                                                    # the slice of (picture, row)
            picture, row = W.REFUSED_IN[name]
            want = [a for a, c in u if 1 <= c <= 0xAF][2 * picture + row]
        for mode in ("module", "iso"):
            r = D.host_decode(x, "i420", mode)[1]
            assert (r["status"], r["err_offset"]) == (D.SYNTAX, want), (name, r)


# ---- one textual change at a time in a copy of csrc/m2v_decode_kernels.hpp: each is caught by a named written case ----
MUTANTS = (
    ("index_63", "if (k >= 64 || b.err) return false;", "if (k >= 63 || b.err) return false;", "escapes"),
    ("level_-2048", "if (lvl == 0 || lvl == -2048) return false;", "if (lvl == 0) return false;", "refusal:escape_level_-2048"),
    ("iso_dc_clamp", "    return v < -2048 ? -2048 : v > 2047 ? 2047 : v;\n}", "    return v;\n}", "dc_range"),
    ("wrap_14", "else if (v > 15) v -= 32;", "else if (v > 14) v -= 32;", "pmv_chain"),
    ("chroma_width", "const uint32_t cw = (w + 1u) / 2u, ch = (h + 1u) / 2u, ysz = w * h;", "const uint32_t cw = w / 2u, ch = (h + 1u) / 2u, ysz = w * h;", "sizes:15x17"),
    ("row_store_19", "v = (int32_t)((U)v << 14) >> 14;", "v = (int32_t)((U)v << 13) >> 13;", "saturate"),
    ("module_floor", "const int32_t lo = mode == kModule ? -2047 : -2048;\n    return v < lo", "const int32_t lo = -2048;\n    return v < lo", "qcodes"),
    ("dc_not_reset", "if (!intra) s.dc_pred[0] = s.dc_pred[1] = s.dc_pred[2] = 0;", "", "dc_range"),
    ("first_escape", "if (first && (w >> 31)) {", "if (first && (w >> 31) && false) {", "escapes"),
    ("qcode_0_as_1", "const uint32_t qcode = get(b, 5);", "uint32_t qcode = get(b, 5); if (!qcode) qcode = 1;", "qcodes"),
)


def _written(name):
    if name.startswith("refusal:"):
        return W.refusals()[name[8:]]
    if name.startswith("sizes:"):
        return W.sized(*[int(v) for v in name[6:].split("x")])[0]
    return getattr(W, name)()[0]


def _agrees(lib, stream):
    """the library gives the definition's answer on a stream, both modes, I420 and NV21"""
    for mode, quirks in BOTH:
        d, _ = D.spec(stream, quirks)
        for layout in ("i420", "nv21"):
            f, r = D.host_decode(stream, layout, mode, lib=lib)
            if (d is None) != (r["status"] == D.SYNTAX) or (d is not None and not np.array_equal(f, D.frames_of(d, layout))):
                return False
    return True


@pytest.mark.parametrize("name,old,new,case", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_written_cases_catch_mutants(tmp_path, name, old, new, case):
    text = _source("m2v_decode_kernels.hpp")
    assert text.count(old) == 1, "the line this mutant changes is not there (once)"
    (tmp_path / "m2v_decode_kernels.hpp").write_text(text.replace(old, new))
    lib = D.build_host(str(tmp_path))
    assert _agrees(D.host_lib(), _written(case))
    assert not _agrees(lib, _written(case)), "mutant %s slipped past %s" % (name, case)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    s = D.small()
    items = [(s, "module"), (s, "iso")]
    items += [(x, ("module", "iso")[k & 1]) for k, (_, x) in enumerate(D.altered())]
    items += [(D.flip(s, b), "module") for b in range(8 * D.first_slice(s))]
    items += [(x, m) for x in list(D.handmade().values()) + list(D.truncations().values()) for m in ("module", "iso")]
    items += [(b"", "iso"), (b"\x00\x00\x01", "iso"), (b"\x00\x00\x01\xb3", "module"), (bytes(64), "iso")]
    items += [(c["stream"], "iso" if c["conformant"] else "module") for c in D.recon_streams().values()]
    items += [(x, m) for x in (D.described(), D.ionly_stream(), D.two_bad_slices()[0]) + D.tile_streams() + D.tile_streams(conformant=True)
              for m in ("module", "iso")]
    items += [(x, m) for x in D.twin_streams().values() for m in ("module", "iso")]
    # the written streams (tests/dec_writer.py); the large ones through one mode
    written = [W.qcodes()[0], W.dc_range()[0], W.escapes()[0], W.saturate()[0], W.pmv_chain()[0]] + [W.sized(w, h)[0] for w, h in W.SIZES]
    written += [x for x, _ in W.stuffed()] + list(W.refusals().values()) + [W.bad_size(w, h) for w, h in BAD_SIZES]
    items += [(x, m) for x in written for m in ("module", "iso")]
    items += [(W.many_pictures()[0], "iso"), (W.big_chunk()[0], "module"), (W.stuffed_2mib()[0], "iso")]
    first_clip = len(items)
    # every table code, escape, DC size and vector delta: each clip in both encodings, each through both modes
    items += [(D.clip_stream(fc[0], fc[1], conformant), m) for fc in D.clip_cases() for conformant in (False, True) for m in ("module", "iso")]
    assert len(items) - first_clip == 4 * len(D.clip_cases()) and len(D.clip_cases()) >= 22 + 42
    path = tmp_path / "streams.bin"
    path.write_bytes(D.pack_streams(items))
    exe = str(tmp_path / "dec_host_check")
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    # the sanitizers' runtimes linked in: the program starts with whatever environment the test has
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", inc, "-o", exe, os.path.join(D.ROOT, "tools", "dec_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    # the program's verdicts are the library's
    for k in (0, 1, 2, 200, 401, first_clip - 3, first_clip - 1, first_clip, first_clip + 171, len(items) - 1):
        stream, mode = items[k]
        want = D.host_decode(stream, D.LAYOUTS[k & 3], mode)[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
