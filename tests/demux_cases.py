"""The demultiplexers (m2vc_demux_ts / m2vc_demux_ps, m2v_demux_device): the containers they are tried on and what they must answer -
shared by tests/test_demux_cases.py (CPU) and tests/test_gpu_demux.py.  Every container is written by tests/demux_writer.py, whose log is
the expectation; nothing here looks at what a demultiplexer computes.  A case is dict(kind, data, arg, expect, log): arg = the `stream`
argument (None: find it), expect = the writer's dict(status, err_offset, es, stamps, record).

cpu(): the specification through ctypes.  host(): the device demultiplexer's arithmetic (csrc/m2v_demux_kernels.hpp) compiled for the CPU
with g++ behind the serial harness of tools/demux_host.hpp - the same functions the kernels are thin loops over."""
import ctypes
import functools
import importlib
import os
import struct
import subprocess
import tempfile

import numpy as np

import demux_writer as W
import m2v_load

M = m2v_load.load()
C = importlib.import_module(M.__name__ + ".container")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"ts": 1, "ps": 2}
OK, SYNTAX, OVERFLOW, NOSTREAM = W.OK, W.SYNTAX, W.OVERFLOW, W.NOSTREAM
SENTINEL = 0xEE
RECORD_FIELDS = ("out_bytes", "pes_packets", "packets", "discontinuities", "skipped", "stream")


@functools.lru_cache(maxsize=None)
def scan_tile():
    return M.demux_scan_tile()


def _case(kind, w):
    return dict(kind=kind, data=w.bytes(), arg=w.arg, expect=w.expect(), log=w.log)


# ---- transport streams ----
PAT = [(0, 0x10), (5, 0x1000), (6, 0x1001)]                   # a network PID, then two programs: the first one's PMT counts


def _psi(w, video_pid=0x1E1):
    """PAT with several programs, the other program's PMT, then ours: four streams, the video entry third, descriptors in both loops, a
    pointer_field of 3 and an adaptation field in front of the section"""
    w.psi(0, W.pat_section(PAT))
    w.psi(0x1001, W.pmt_section(6, 0x300, [(0x02, 0x300, b""), (0x03, 0x301, b"")]))
    w.psi(0x1000, W.pmt_section(5, video_pid, [(0x03, 0x1E0, b""), (0x06, 0x1E2, b"\x0a\x04eng\x00"), (0x02, video_pid, b"\x02\x03abc"),
                                               (0x1B, 0x1E3, b"")], program_info=b"\x05\x04HDMV"), pointer=3, short=True)


def ts_count(n, seed):
    """exactly n packets, all of the video PID, which the caller names: no PAT in the container"""
    w = W.TsWriter(seed, video_pid=0x44, arg=0x44)
    per = max(1, n // 10)
    left = n
    k = 0
    while left:
        take = min(per, left)
        w.pes_packet(184 * take - 14 - (k % 5), pts=1000 + 3600 * k)
        left -= take
        k += 1
    assert len(w.out) == 188 * n
    return w


def ts_shapes(seed=7):
    w = W.TsWriter(seed, video_pid=0x1E1)
    w.continuation(184)                                         # the stream is joined in mid-packet: three packets in front of the first start,
    w.other(0x1E0, 184, pusi=1)                                 # (an audio packet whose payload starts like a video PES packet)
    w.continuation(77)
    w.video(b"")                                                # ... one of them without a payload
    _psi(w)
    w.null()
    w.tei()
    w.pes_packet(900, pts=900000, dts=896250, sizes=(19, 0, 1, 183, 184))       # header ends with its packet; payloads of 0, 1, 183, 184 bytes
    w.other(0x300, 184)
    w.pes_packet(300)                                           # hl 0: no stamps
    w.pes_packet(10, pts=903750)                                # hl 5, one packet
    w.null()
    w.pes_packet(500, pts=907500, stuffing=7)                   # stuffing behind the stamp
    w.psi(0, W.pat_section(PAT))                                # repeated PSI, now in the middle
    w.tei(pid=0x300)
    w.pes_packet(700, pts=911250, dts=911000, stuffing=3, gap=3)                # packets lost: a discontinuity
    w.pes_packet(400, pts=915000, sizes=(100,), gap=2, di=1)                    # ... and one the multiplexer announces
    w.video(b"", di=1)                                          # adaptation field only, length 183
    w.pes_packet(184 * 20, pts=918750)                          # the counter wraps
    w.pes_packet(40, pts=922500, gap=-1)                        # the counter repeated: not removed, counted
    return w


def ts_big(seed=8, pes_packets=40, nbytes=60000):
    """a few MB, 13 tiles, other PIDs woven in (tests/test_gpu_demux.py shrinks the grids around it, and says what that reaches)"""
    w = W.TsWriter(seed, video_pid=0x1E1)
    _psi(w)
    for k in range(pes_packets):
        w.pes_packet(nbytes + 13 * k, pts=90000 + 3750 * k, dts=None if k % 3 else 86250 + 3750 * k)
        for _ in range(k % 4):
            w.other(0x1E0, 184)
        if k % 8 == 0:
            _psi(w)
            w.null()
    return w


def _ts_ref(seed, arg=None):
    """a small valid start: PSI (or none with the PID given) and one PES packet"""
    w = W.TsWriter(seed, video_pid=0x1E1, arg=arg)
    if arg is None:
        _psi(w)
    w.pes_packet(300, pts=5000)
    return w


def _ts_refusals():
    R = {}
    pes = lambda **bad: W.pes_header(0xE0, 0, pts=7000, dts=bad.pop("dts", None), **bad)

    def broken_video(name, data, head, full=True):
        """a packet that starts a PES packet with this header (and elementary bytes to the packet's end)"""
        w = _ts_ref(100 + len(R))
        w.video(data + (W.payload(w.rng, 184 - len(data)) if full else b""), pusi=1, head=head, broken=True)
        w.pes_packet(200, pts=9000)
        R[name] = w

    w = _ts_ref(90); w.out = w.out[:-100]; R["length"] = w
    w = W.TsWriter(91, arg=0x1E1); R["empty"] = w
    w = _ts_ref(92); w.errors.append(len(w.out)); w.raw(W.ts_packet(0x300, 0, W.payload(w.rng, 184), sync=0x48)); w.pes_packet(100, pts=1); R["sync"] = w
    # PAT / PMT
    for name, sec in (("pat_table_id", W.psi_section(1, 1, W.Bits().put(5, 16).put(7, 3).put(0x1000, 13).bytes())),
                      ("pat_syntax_indicator", W.pat_section(PAT, syntax=0)), ("pat_crc", W.pat_section(PAT, bad_crc=True)),
                      ("pat_crosses", W.pat_section([(k + 1, 0x1000 + k) for k in range(60)]))):
        w = W.TsWriter(110 + len(R), video_pid=0x1E1); w.psi(0, sec, broken=True); _psi(w); w.pes_packet(100, pts=1); R[name] = w
    w = W.TsWriter(93, video_pid=0x1E1); w.psi(0, W.pat_section(PAT), short=True, afl=183, broken=True); R["pat_adaptation_183"] = w
    w = W.TsWriter(94, video_pid=0x1E1); w.psi(0, W.pat_section([(0, 0x10)])); w.pes_packet(100, pts=1); w.nostream = True; R["pat_no_program"] = w
    w = W.TsWriter(95, video_pid=0x1E1); w.pes_packet(100, pts=1); w.nostream = True; R["no_pat"] = w
    w = W.TsWriter(96, video_pid=0x1E1); w.psi(0, W.pat_section(PAT)); w.pes_packet(100, pts=1); w.nostream = True; R["no_pmt"] = w
    streams = [(0x03, 0x1E0, b""), (0x02, 0x1E1, b"")]
    for name, sec, bad in (("pmt_crc", W.pmt_section(5, 0x1E1, streams, bad_crc=True), True), ("pmt_program", W.pmt_section(6, 0x1E1, streams), True),
                           ("pmt_table_id", W.psi_section(3, 5, b"\xe1\xe1\xf0\x00"), True),
                           ("pmt_info_length", W.psi_section(2, 5, W.Bits().put(7, 3).put(0x1E1, 13).put(15, 4).put(200, 12).bytes()), True),
                           ("pmt_no_video", W.pmt_section(5, 0x1E0, [(0x03, 0x1E0, b""), (0x1B, 0x1E1, b"")]), False)):
        w = W.TsWriter(120 + len(R), video_pid=0x1E1); w.psi(0, W.pat_section(PAT)); w.psi(0x1000, sec, broken=bad); w.pes_packet(100, pts=1)
        w.nostream = not bad
        R[name] = w
    # the video packets' own header
    for name, kw in (("scrambling_control", dict(tsc=2)), ("adaptation_control_0", dict(afc=0)), ):
        w = _ts_ref(130 + len(R)); w.video(W.payload(w.rng, 184), broken=True, **kw); w.pes_packet(100, pts=1); R[name] = w
    w = _ts_ref(97); w.video(b"", afc=2, afl=182, broken=True); R["adaptation_only_182"] = w
    w = _ts_ref(98); w.video(b"", afc=3, afl=183, broken=True); R["adaptation_3_length_183"] = w
    # the PES header
    broken_video("pes_prefix", pes(prefix=2), 14)
    broken_video("pes_stream_id", W.pes_header(0xC0, 0, pts=7000), 14)
    broken_video("pes_marker_10", pes(marker=1), 14)
    broken_video("pes_scrambling", pes(scrambling=1), 14)
    broken_video("pes_flags_1", pes(flags=1), 14)
    broken_video("pes_pts_short", W.pes_header(0xE0, 0, flags=2, hl=4) + b"\x21\x00\x01\x00", 13)
    broken_video("pes_pts_prefix", pes(pts_prefix=3), 14)
    broken_video("pes_pts_marker", pes(pts_markers=(1, 0, 1)), 14)
    broken_video("pes_dts_short", W.pes_header(0xE0, 0, pts=7000, flags=3), 14)
    broken_video("pes_dts_prefix", pes(dts=6000, dts_prefix=3), 19)
    broken_video("pes_dts_marker", pes(dts=6000, dts_markers=(1, 1, 0)), 19)
    broken_video("pes_crosses_packet", W.pes_header(0xE0, 0, pts=7000, stuffing=200)[:184], 184)
    broken_video("pes_under_9", W.pes_header(0xE0, 0)[:8], 8, full=False)
    broken_video("pes_start_without_payload", b"", 0, full=False)
    w = W.TsWriter(99, video_pid=0x1E1); _psi(w); w.continuation(184); w.continuation(50); R["no_start"] = w
    # two errors: the earlier counts, whichever kind it is
    w = _ts_ref(140); w.video(W.payload(w.rng, 184), broken=True, tsc=1); w.errors.append(len(w.out)); w.raw(W.ts_packet(0x300, 0, b"\xff" * 184, sync=0))
    R["two_video_first"] = w
    w = _ts_ref(141); w.errors.append(len(w.out)); w.raw(W.ts_packet(0x300, 0, b"\xff" * 184, sync=0)); w.video(W.payload(w.rng, 184), broken=True, tsc=1)
    w.out = w.out[:-3]
    R["two_sync_first"] = w
    return R


# ---- program streams ----
def ps_shapes(seed=20, arg=None, end=True):
    w = W.PsWriter(seed, arg=arg)
    w.pack(stuffing=0, scr=0)
    w.system_header((0xE0, 0xE1))
    w.fake(0xBC)                                                # a program stream map
    w.pes_packet(0xE0, 500, pts=90000, dts=86250)
    for k in range(1, 8):
        w.pack(stuffing=k, scr=27000 * k)
        if k == 2:
            w.fake(0xBE)                                        # padding
        if k == 3:
            w.fake(0xBD); w.fake(0xBF)                          # private streams
        if k == 4:
            w.fake(0xC0)                                        # audio
        w.pes_packet(0xE0 + (k & 1), 100 * k + (k == 5), pts=None if k == 6 else 90000 + 3750 * k, dts=86000 + 3750 * k if k == 7 else None,
                     stuffing=4 if k == 2 else 0)
    w.pes_packet(0xE1, 0, pts=777)                              # an empty packet: a stamp and no byte
    w.pes_packet(0xE0, 0)
    if end:
        w.end(zeros=37)
    return w


def ps_tile(k, multiples=2):
    """a unit starts k bytes in front of every multiple of the transport tile (k = 1 .. 3: its start code straddles the boundary; 0: at
    it; 4: just in front), a video packet each time"""
    T = scan_tile()
    w = W.PsWriter(30 + k)
    w.pack()
    for m in range(1, multiples + 1):
        target = m * T - k
        while target - len(w.out) > 60000:
            w.pes_packet(0xE0, 30000 - len(w.out) % 7, pts=len(w.out))
            w.filler(20000)
        left = target - len(w.out)
        w.pes_packet(0xE0, left - 14 - 30, pts=5)
        w.filler(30)
        assert len(w.out) == target
        w.pes_packet(0xE0, 100, pts=6, dts=5)
    w.end()
    return w


def ps_many_units(seed=40, n=5000):
    """thousands of units of a few bytes: video packets of 0 .. 12 bytes between packs and padding"""
    w = W.PsWriter(seed)
    for k in range(n):
        if k % 3 == 0:
            w.pack(stuffing=k % 8)
        if k % 5 == 0:
            w.filler(6 + k % 11)
        w.pes_packet(0xE0, k % 13, pts=k if k % 2 else None)
    w.end()
    return w


def ps_big(seed=41, packs=1500):
    """a few MB: 2 KB packs as a multiplexer writes them, audio between"""
    w = W.PsWriter(seed)
    for k in range(packs):
        w.pack(scr=27000 * k)
        if k == 0:
            w.system_header()
        if k % 16 == 0:
            w.pes_packet(0xE0, 2011, pts=90000 + 3750 * k)
        elif k % 7 == 3:
            w.unit(0xC0, W.payload(w.rng, 2028))
        else:
            w.pes_packet(0xE0, 2025)
    w.end()
    return w


def _ps_ref(seed, arg=None):
    w = W.PsWriter(seed, arg=arg)
    w.pack(); w.system_header(); w.pes_packet(0xE0, 200, pts=5000)
    return w


def _ps_refusals():
    R = {}

    def after(name, fn, seed=200):
        w = _ps_ref(seed + len(R)); fn(w); w.pack(); w.pes_packet(0xE0, 50, pts=1); w.end(); R[name] = w

    after("prefix", lambda w: w.garbage(b"\x00\x00\x02\xba" + bytes(20)))
    after("code_b3", lambda w: w.garbage(b"\x00\x00\x01\xb3" + bytes(20)))
    after("code_b8", lambda w: w.garbage(b"\x00\x00\x01\xb8\x00\x08" + bytes(8)))
    after("mpeg1_pack", lambda w: w.pack_mpeg1())
    for f in ("two", "m0", "m1", "m2", "m3", "mm"):
        after("pack_" + f, lambda w, f=f: w.pack(broken=True, **{f: 0}))
    after("pes_length_0", lambda w: w.pes_packet(0xE0, 0, broken=True, length=0))
    after("pes_length_2", lambda w: w.pes_packet(0xE0, 0, broken=True, length=2))
    after("pes_hl_past_length", lambda w: w.pes_packet(0xE0, 10, pts=5, broken=True, hl=16))
    after("pes_flags_1", lambda w: w.pes_packet(0xE0, 10, broken=True, flags=1))
    after("pes_marker_10", lambda w: w.pes_packet(0xE0, 10, broken=True, marker=3))
    after("pes_scrambling", lambda w: w.pes_packet(0xE0, 10, broken=True, scrambling=2))
    after("pes_pts_prefix", lambda w: w.pes_packet(0xE0, 10, pts=5, broken=True, pts_prefix=1))
    after("pes_pts_marker", lambda w: w.pes_packet(0xE0, 10, pts=5, broken=True, pts_markers=(0, 1, 1)))
    after("pes_dts_prefix", lambda w: w.pes_packet(0xE0, 10, pts=5, dts=4, broken=True, dts_prefix=2))
    after("pes_dts_short", lambda w: w.pes_packet(0xE0, 10, pts=5, broken=True, flags=3))
    # what ends in the middle of a unit
    w = _ps_ref(230); w.pack(stuffing=5, broken=True); w.out = w.out[:-2]; R["pack_stuffing_cut"] = w
    w = _ps_ref(231); w.pack(broken=True); w.out = w.out[:-3]; R["pack_cut"] = w
    w = _ps_ref(232); w.unit(0xBE, bytes(40), broken=True, length=41); R["unit_past_end"] = w
    w = _ps_ref(233); w.garbage(b"\x00\x00\x01\xe0\x00"); R["unit_cut"] = w
    w = _ps_ref(234); w.garbage(b"\x00\x00\x01"); R["code_cut"] = w
    w = _ps_ref(235); w.end(zeros=5, tail=b"\x00\x00\x07\x00"); R["after_end"] = w
    # no stream
    w = _ps_ref(236, arg=0xE5); w.end(); R["id_absent"] = w
    w = W.PsWriter(237); w.pack(); w.system_header(); w.unit(0xC0, bytes(100)); w.end(); R["no_video"] = w
    w = W.PsWriter(238); R["empty"] = w
    # two errors: the chain meets the first
    w = _ps_ref(239); w.pes_packet(0xE0, 10, broken=True, flags=1); w.pack(broken=True, two=0); R["two"] = w
    return R


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case; every one valid (status OK)"""
    c = {}
    for n in (1, 63, 64, 65, 256, 257, 1030):
        c["ts_n%d" % n] = _case("ts", ts_count(n, 50 + n % 7))
    c["ts_shapes"] = _case("ts", ts_shapes())
    c["ps_shapes"] = _case("ps", ps_shapes())
    c["ps_second_id"] = _case("ps", ps_shapes(21, arg=0xE1))
    c["ps_no_end"] = _case("ps", ps_shapes(22, end=False))
    for k in range(5):
        c["ps_tile%d" % k] = _case("ps", ps_tile(k))
    c["ps_many_units"] = _case("ps", ps_many_units())
    assert all(v["expect"]["status"] == OK for v in c.values())
    return c


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> case; the status is SYNTAX or NOSTREAM, as the writer's log says"""
    r = {"ts:" + k: _case("ts", w) for k, w in _ts_refusals().items()}
    r.update({"ps:" + k: _case("ps", w) for k, w in _ps_refusals().items()})
    assert all(v["expect"]["status"] in (SYNTAX, NOSTREAM) for v in r.values())
    return r


@functools.lru_cache(maxsize=None)
def big(kind):
    return _case(kind, ts_big() if kind == "ts" else ps_big())


# ---- altered containers ----
ALTER_BASE = {"ts": "ts_alter", "ps": "ps_alter"}
ALTER_SEED = {"ts": 1, "ps": 2}


@functools.lru_cache(maxsize=None)
def alter_base(kind):
    """-> (case, the bytes whose every bit is flipped).  TS: a PAT with two dozen programs, then the first video packet (the PMT comes
    later: the PID found there holds for the packets in front of it too), so a flip in the first two packets breaks a section or a
    header about as often as it changes bytes of the stream; PS: a first pack of two small packets"""
    if kind == "ts":
        w = W.TsWriter(60, video_pid=0x1E1)
        w.psi(0, W.pat_section(PAT + [(10 + k, 0x1100 + k) for k in range(21)]))
        w.pes_packet(330, pts=1000, dts=900)
        _psi(w)
        for k in range(6):
            w.pes_packet(150 + 90 * k, pts=2000 + k)
            w.other(0x1E0, 100 + k)
        return _case("ts", w), 376
    w = W.PsWriter(61)
    w.pack(stuffing=2); w.system_header(); w.pes_packet(0xE0, 60, pts=1000, dts=900); w.filler(16); w.pes_packet(0xE0, 40)
    first = len(w.out)
    for k in range(6):
        w.pack(stuffing=k)
        w.pes_packet(0xE0, 200 + 50 * k, pts=2000 + k)
        w.fake(0xBD)
    w.end(zeros=3)
    return _case("ps", w), first


@functools.lru_cache(maxsize=None)
def altered(kind):
    """[bytes]: every bit of the first two packets / the first pack flipped, then 500 seeded flips, cuts and insertions over the whole"""
    case, first = alter_base(kind)
    base = case["data"]
    out = []
    for bit in range(8 * first):
        b = bytearray(base)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append(bytes(b))
    rng = np.random.RandomState(ALTER_SEED[kind])
    unit = 188 if kind == "ts" else 1
    for k in range(500):
        b = bytearray(base)
        what = k % 4
        if what < 2:                                            # a bit anywhere
            at = int(rng.randint(0, len(b)))
            b[at] ^= 1 << int(rng.randint(0, 8))
        elif what == 2:                                         # a cut: the tail, or a span from the middle (TS: whole packets every other time)
            u = unit if k % 8 == 2 else 1
            at = int(rng.randint(0, len(b) // u)) * u
            n = int(rng.randint(1, 4)) * u if u > 1 else int(rng.randint(1, 300))
            if k % 16 == 6:
                del b[at:]
            else:
                del b[at:at + n]
        else:                                                   # an insertion of seeded bytes, or of a copy of what stands there
            u = unit if k % 8 == 3 else 1
            at = int(rng.randint(0, len(b) // u + 1)) * u
            n = u if u > 1 else int(rng.randint(1, 300))
            ins = bytes(b[at:at + n]) if k % 16 == 7 and at + n <= len(b) else W.payload(rng, n)
            b[at:at] = ins
        out.append(bytes(b))
    return out


def alter_arg(kind):
    return alter_base(kind)[0]["arg"]


# ---- the specification ----
def cpu(kind, data, arg=None, cap=None, stamp_cap=None):
    """-> dict(status, err_offset, es, stamps [(es_offset, pts, dts, src_offset)], record {field: value})"""
    r, info, es, stamps = C.demux_raw(kind, data, arg, cap, stamp_cap)
    assert r == info.status
    return dict(status=r, err_offset=info.err_offset, es=es, stamps=[(s.es_offset, s.pts, s.dts, s.src_offset) for s in stamps],
                record={f: getattr(info, f) for f in RECORD_FIELDS})


# ---- the device demultiplexer's arithmetic on the CPU ----
class HostRecord(ctypes.Structure):
    _fields_ = [("src_offset", ctypes.c_uint64), ("src_bytes", ctypes.c_uint64), ("out_offset", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64),
                ("err_offset", ctypes.c_uint64), ("pes_packets", ctypes.c_uint32), ("packets", ctypes.c_uint32), ("discontinuities", ctypes.c_uint32),
                ("skipped", ctypes.c_uint32), ("stream", ctypes.c_uint32), ("status", ctypes.c_int32)]


_HARNESS = r"""
#include "demux_host.hpp"
extern "C" void demux_host_run(int kind, const uint8_t *src, uint64_t n, int stream, uint8_t *out, uint64_t cap, int lead, void *stamps, uint64_t stamp_cap,
                               demux_host::Record *rec)
{
    *rec = demux_host::run(kind, src, n, stream, out, cap, lead, (demux_host::Stamp *)stamps, stamp_cap);
}
"""


def build_host(include_dir=None):
    """the harness over csrc/m2v_demux_kernels.hpp (include_dir: a directory with another copy of that header, looked in first)"""
    d = tempfile.mkdtemp(prefix="m2v_demux_host_")
    src, so = os.path.join(d, "demux_host.cpp"), os.path.join(d, "libdemux_host.so")
    with open(src, "w") as f:
        f.write(_HARNESS)
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    first = ["-I", include_dir] if include_dir else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror"] + first + ["-I", inc, "-I", os.path.join(ROOT, "tools"), "-o", so, src])
    L = ctypes.CDLL(so)
    L.demux_host_run.restype = None
    L.demux_host_run.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HostRecord)]
    return L


@functools.lru_cache(maxsize=None)
def host_lib():
    return build_host()


def host(kind, data, arg=None, lead=0, lib=None, cap=None, stamp_cap=None):
    """the same dict as cpu(), from the host build; the stream is written `lead` bytes past a 16-byte boundary between sentinels"""
    lib = lib or host_lib()
    data = bytes(data)
    room = len(data) + 64 if cap is None else cap
    nst = len(data) // 9 + 2 if stamp_cap is None else stamp_cap
    buf = ctypes.create_string_buffer(bytes([SENTINEL]) * (room + 64), room + 64)
    stamps = np.full((nst + 1, 4), SENTINEL, np.uint64)
    rec = HostRecord()
    base = ctypes.addressof(buf)
    at = (-base) % 16 + 16 + lead
    lib.demux_host_run(KINDS[kind], data, len(data), -1 if arg is None else arg, base + at, room, lead, stamps.ctypes.data, nst, ctypes.byref(rec))
    raw = buf.raw
    n = rec.out_bytes
    assert n <= room and set(raw[:at]) <= {SENTINEL} and set(raw[at + n:]) <= {SENTINEL}, "the host build wrote outside its stream"
    k = min(rec.pes_packets, nst)
    assert (stamps[k:] == SENTINEL).all(), "the host build wrote outside its stamps"
    return dict(status=rec.status, err_offset=rec.err_offset, es=raw[at:at + n], stamps=[tuple(int(v) for v in row) for row in stamps[:k]],
                record={f: getattr(rec, f) for f in RECORD_FIELDS})


def pack_containers(items):
    """[(kind, arg, bytes)] -> the file tools/demux_host_check.cpp reads"""
    out = [struct.pack("<I", len(items))]
    for kind, arg, data in items:
        out.append(struct.pack("<IiQ", KINDS[kind], -1 if arg is None else arg, len(data)))
        out.append(bytes(data))
    return b"".join(out)
