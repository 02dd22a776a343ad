"""The device muxer (m2v_set_mux_out, m2v_mux_device): the elementary streams it is tried on and what it must produce for them - shared by
tests/test_mux_cases.py (CPU) and tests/test_gpu_mux.py.  The definition is the expectation: the container of a stream is what the CPU
muxers of libm2v_container.so (m2vc_mux_ts / m2vc_mux_ps) return for it, byte for byte.  Two kinds of input: the oracle's streams of
tests/test_container.py's three clips, and synthetic elementary streams - real start codes and headers, filler bytes >= 2 in the slices,
picture sizes chosen so that the containers reach every stuffing shape, pack length, rate and scan boundary (tests/test_mux_cases.py
counts them in the CPU muxers' output).  Nothing here looks at what the device computes.

host(): the arithmetic of the device muxer (csrc/m2v_mux_kernels.hpp) compiled for the CPU with g++, every 16-byte unit generated in a
loop - the same functions the kernels are thin loops over."""
import ctypes
import functools
import importlib
import os
import subprocess
import tempfile

import numpy as np

import m2v_load

M = m2v_load.load()
C = importlib.import_module(M.__name__ + ".container")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ts", "ps")
OK, SYNTAX, OVERFLOW = 0, -2, -3
SENTINEL = 0xEE


def cpu_mux(kind, es):
    """the specification: -> the container's bytes, or the negative M2VC_E_* code"""
    fn = C.lib().m2vc_mux_ts if kind == "ts" else C.lib().m2vc_mux_ps
    es = bytes(es)
    n = ctypes.c_size_t()
    r = fn(es, len(es), None, 0, ctypes.byref(n))
    if r < 0:
        return r
    out = ctypes.create_string_buffer(max(n.value, 1))
    r = fn(es, len(es), out, n.value, ctypes.byref(n))
    assert r == 0
    return out.raw[:n.value]


# ---- the oracle's streams (tests/test_container.py's clips) ----
@functools.lru_cache(maxsize=None)
def oracle_clip(key):
    """-> (frames [n, 3, H, W], the oracle's stream, W, H, pframes_count, Q_LEVEL)"""
    from oracle import m2v_oracle_ctypes as orc
    orc.build()
    if key == "ip":
        f = M.synth.clip(96, 64, 11, clip_index=40)
        return f, orc.encode(f, 6, 4, 3, XL=6, YL=6), 96, 64, 3, 2
    if key == "i":
        f = M.synth.clip(64, 64, 3, clip_index=41)
        return f, orc.encode(f, 4, 4, 0, XL=6, YL=6), 64, 64, 0, 2
    assert key == "big"
    f = M.synth.clip(320, 240, 6, clip_index=42)
    return f, orc.encode(f, 20, 15, 255, XL=6, YL=6, Q=1), 320, 240, 255, 1


ORACLE_CLIPS = ("ip", "i", "big")


# ---- synthetic elementary streams ----
def _filler(rng, n):
    return rng.randint(2, 256, size=n).astype(np.uint8).tobytes()


def seq_headers(rng, rate_code):
    """34 bytes: sequence_header (96 x 64, the frame_rate_code in the low half of byte 7), two extension start codes with filler"""
    return (b"\x00\x00\x01\xb3\x06\x00\x40" + bytes([0x10 | rate_code]) + _filler(rng, 4) +
            b"\x00\x00\x01\xb5" + _filler(rng, 6) + b"\x00\x00\x01\xb5" + _filler(rng, 8))


MIN_AU = {"P": 26, "I": 34, "IS": 68}


def access_unit(rng, kind, size, tref, coding_type=None):
    """`size` bytes: [repeated sequence headers (IS)] [GOP header (I, IS)] picture header, extension, one slice of filler"""
    assert size >= MIN_AU[kind], (kind, size)
    b = b""
    if kind == "IS":
        b += seq_headers(rng, 2)
    if kind != "P":
        b += b"\x00\x00\x01\xb8" + _filler(rng, 4)
    ct = coding_type if coding_type is not None else (2 if kind == "P" else 1)
    b += b"\x00\x00\x01\x00" + bytes([(tref >> 2) & 0xFF, ((tref & 3) << 6) | (ct << 3) | 7]) + _filler(rng, 2)
    b += b"\x00\x00\x01\xb5" + _filler(rng, 5)
    b += b"\x00\x00\x01\x01"
    return b + _filler(rng, size - len(b))


def synth(aus, rate_code=2, seed=1, pad=True, coding_types=None):
    """sequence headers, the access units (kind, bytes) - the first one an "I" -, sequence_end_code and the module's zero padding to the
    end of the 32-byte word behind it"""
    rng = np.random.RandomState(seed)
    assert aus[0][0] == "I"
    b = seq_headers(rng, rate_code)
    tref = 0
    for k, (kind, size) in enumerate(aus):
        tref = 0 if kind != "P" else tref + 1
        b += access_unit(rng, kind, size, tref, None if coding_types is None else coding_types.get(k))
    b += b"\x00\x00\x01\xb7"
    if pad:
        b += bytes(((len(b) - 4 + 4) // 32 + 1) * 32 - len(b))
    return b


def au_starts(aus):
    at, out = 34, []
    for _, size in aus:
        out.append(at)
        at += size
    return out, at           # the access units' offsets, and the end code's


@functools.lru_cache(maxsize=None)
def scan_tile():
    return M.mux_scan_tile()


def boundary_aus(k):
    """a stream of about 5 T in which a picture_start_code, a GOP header, a repeated sequence header and the end code begin at
    m T - k, m = 1, 2, 3, 5 (T = the scan's tile)"""
    T = scan_tile()
    at = 34
    aus = []
    for kind, target in (("I", T - k), ("P", 2 * T - k), ("I", 3 * T - k), ("IS", 5 * T - k)):
        aus.append((kind, target - at))                     # this one ends, and the next one (or the end code) begins, at the target
        at = target
    # the access units BEGIN with: (34: I), T - k: a picture_start_code, 2 T - k: a GOP header, 3 T - k: a sequence header; end code at 5 T - k
    return aus


def _cases():
    c = {}
    # TS stuffing: a PES packet is 14 + b bytes, 176 in its first packet.  b = 162: exactly the first packet; 100: stuffing behind the PCR;
    # 346 / 345 / 344 / 163: 184, 183 (adaptation_field_length 0), 182 and 1 byte(s) left for the last packet
    c["ts_stuffing"] = synth([("I", 300), ("P", 162), ("P", 100), ("P", 346), ("P", 345), ("P", 344), ("P", 163), ("I", 530), ("P", 40)], seed=2)
    # PS packs: 2020 bytes fill a later picture's first pack exactly (2005 the first picture's, with the system header: 34 + 1971), one
    # more byte starts a pack of 24 bytes, and small pictures end their pack early
    c["ps_packs"] = synth([("I", 1971), ("P", 2020), ("P", 2021), ("P", 300), ("I", 2020 + 2025), ("P", 2020 + 2025 + 1), ("P", 5000)], seed=3)
    for code in range(1, 9):
        c["rate%d" % code] = synth([("I", 700), ("P", 300), ("P", 200), ("IS", 700), ("P", 250)], rate_code=code, seed=10 + code)
    # above the floor of 125 000 bytes/s (60 pictures a second of 4000 bytes), and 2.1 s of stream time: more than 16 PAT / PMT pairs
    c["fast"] = synth([("I", 6000)] + [("P", 4000)] * 9, rate_code=8, seed=20)
    c["long"] = synth([("IS" if i and i % 10 == 0 else "I" if i % 10 == 0 else "P", 4600 + 37 * (i % 7)) for i in range(60)], seed=21)
    # small pictures: more headers than m2v_mux_device guesses for a stream of this size (it runs a second time)
    c["small"] = synth([("I" if i % 4 == 0 else "P", 34 + i % 5) for i in range(300)], seed=22)
    c["one"] = synth([("I", 500)], seed=23)
    c["no_end_padding"] = synth([("I", 400), ("P", 90)], seed=24, pad=False)
    for k in range(4):
        c["boundary%d" % k] = synth(boundary_aus(k), seed=30 + k)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> elementary stream; every one a valid stream"""
    return _cases()


@functools.lru_cache(maxsize=None)
def error_cases():
    """name -> (elementary stream, expected status)"""
    good = synth([("I", 400), ("P", 90), ("P", 120)], seed=40)
    e = {}
    e["not_b3"] = (b"\x00\x00\x01\xb4" + good[4:], SYNTAX)
    e["type3"] = (synth([("I", 400), ("P", 90), ("P", 120)], seed=40, coding_types={1: 3}), SYNTAX)
    e["after_end"] = (good[:-1] + b"\x01", SYNTAX)
    e["rate0"] = (synth([("I", 400), ("P", 90)], rate_code=0, seed=41), SYNTAX)
    e["rate9"] = (synth([("I", 400), ("P", 90)], rate_code=9, seed=42), SYNTAX)
    e["no_picture"] = (seq_headers(np.random.RandomState(43), 2) + b"\x00\x00\x01\xb7" + bytes(28), SYNTAX)
    e["short"] = (b"\x00\x00\x01\xb3\x06\x00\x40\x12", SYNTAX)
    return e


BATCH = ("rate4", "one", "ts_stuffing", "small", "ps_packs")          # five streams of different sizes, one of them a single picture


def place(streams, lead=0, gap=7):
    """the streams one behind the other in one buffer, `lead` bytes in front of the first and `gap` sentinel bytes between them:
    -> (buffer, [(offset, bytes)])"""
    buf, seg = bytearray([SENTINEL] * lead), []
    for s in streams:
        seg.append((len(buf), len(s)))
        buf += s + bytes([SENTINEL] * gap)
    return bytes(buf), seg


def layout(sizes_or_status, cap):
    """the records' out_offset / out_bytes / status for containers of these sizes (a negative entry: that status, nothing written) in a
    buffer of cap bytes: each starts at the next multiple of 32 behind the one before"""
    out, end = [], 0
    for v in sizes_or_status:
        o = (end + 31) // 32 * 32
        if v >= 0 and o + v > cap:
            v = OVERFLOW
        out.append((o, max(v, 0), min(v, 0)))
        if v > 0:
            end = o + v
    return out


# ---- the device muxer's arithmetic on the CPU ----
_HARNESS = r"""
#include "m2v_mux_kernels.hpp"
#include <algorithm>
#include <vector>
using namespace m2v::mux;
// the whole muxer as the kernels run it, serially: scan every 16 positions, sort the events, plan, generate every 16-byte unit of a
// container that starts `lead` bytes past a 16-byte boundary.  Returns the container's bytes or the status; *pictures as the record's.
extern "C" long long mux_host(int kind, const uint8_t *es, uint64_t es_bytes, uint8_t *out, uint64_t cap, int lead, uint32_t *pictures)
{
    Stream S{};
    S.es_bytes = es_bytes; S.kind = (uint32_t)kind;
    std::vector<uint64_t> ev;
    ScanAcc a;
    // (back to front: the order of the list is the atomics', the plan must not rely on it)
    for (uint64_t p0 = (es_bytes + 15) / 16 * 16; p0 >= 16; p0 -= 16) {
        uint64_t w0, w1, w2;
        load24(es, p0 - 16, es_bytes, w0, w1, w2);
        scan16(p0 - 16, es_bytes, w0, w1, w2, a, [&](uint64_t v) { ev.push_back(v); });
    }
    S.inv_first_end = a.inv_first_end; S.inv_first_bad = a.inv_first_bad; S.inv_first_slice = a.inv_first_slice; S.last_nz = a.last_nz;
    std::sort(ev.begin(), ev.end());
    std::vector<Pic> pics(ev.size() + 2);
    uint64_t maxpic = 0;
    *pictures = 0;
    int st = plan_pictures(es, es_bytes, ev.data(), (uint32_t)ev.size(), (uint32_t)ev.size() + 1, S, pics.data(), S.npics, S.n, maxpic);
    if (st != kOk) return st;
    S.out_bytes = plan_layout(S, pics.data(), es, maxpic);
    *pictures = S.npics;
    if (S.out_bytes > cap) return kOverflow;
    const uint64_t units = (S.out_bytes + lead + 15) / 16;
    for (uint64_t u = 0; u < units; ++u) {
        const long long q0 = (long long)(16 * u) - lead;
        const Win w = gen16(S, pics.data(), es, q0);
        for (int k = 0; k < 16; ++k) {
            const long long q = q0 + k;
            if (q >= 0 && (uint64_t)q < S.out_bytes) out[q] = (uint8_t)((k < 8 ? w.lo : w.hi) >> (8 * (k & 7)));
        }
    }
    return (long long)S.out_bytes;
}
extern "C" unsigned long long mux_host_bound(int kind, unsigned long long es_bytes, unsigned long long pictures) { return bound(kind, es_bytes, pictures); }
"""

_host = None


def host_lib():
    """the harness above and csrc/m2v_mux_kernels.hpp, compiled with g++ (no HIP), contraction off as on the device"""
    global _host
    if _host is None:
        d = tempfile.mkdtemp(prefix="m2v_mux_host_")
        src, so = os.path.join(d, "mux_host.cpp"), os.path.join(d, "libmux_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-I", inc, "-o", so, src])
        L = ctypes.CDLL(so)
        L.mux_host.restype = ctypes.c_longlong
        L.mux_host.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                               ctypes.POINTER(ctypes.c_uint32)]
        L.mux_host_bound.restype = ctypes.c_ulonglong
        L.mux_host_bound.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong]
        _host = L
    return _host


def host_mux(kind, es, lead=0, cap=None):
    """-> (the container's bytes or the negative status, pictures)"""
    es = bytes(es)
    room = M.mux_bound(kind, len(es), max(1, len(es) // 8)) + 64 if cap is None else cap
    out = ctypes.create_string_buffer(max(room, 1))
    n = ctypes.c_uint32()
    r = host_lib().mux_host(M.MUX_KINDS[kind], es, len(es), out, room, lead, ctypes.byref(n))
    return (out.raw[:r] if r >= 0 else int(r)), n.value
