"""The device decoder on the CPU: csrc/m2v_decode_kernels.hpp and the serial harness tools/dec_host.hpp, compiled with g++, against
decoder.py - valid streams frame for frame and count for count, every VLC function, both inverse transforms, the dequantisers and the
vector wrap unit by unit, refusals on altered streams exactly where the definition refuses, the scan's tile boundaries, and the whole
host build once more under AddressSanitizer and UBSan as a stand-alone program.  tests/test_gpu_decode.py runs the same streams on the
device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dec_cases as D
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
    for k in (0, 1, 2, 200, 401, first_clip - 1, first_clip, first_clip + 171, len(items) - 1):
        stream, mode = items[k]
        want = D.host_decode(stream, D.LAYOUTS[k & 3], mode)[1]
        assert [int(v) for v in lines[k].split()[:4]] == [k, want["status"], want["err_offset"], want["pictures"]]
