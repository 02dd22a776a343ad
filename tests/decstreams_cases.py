"""Several streams per call (m2v_decode_streams_device): the batches it is tried on and what it must answer - shared by
tests/test_decstreams_cases.py (CPU, the host build tools/dec_host.hpp: decode_streams) and tests/test_gpu_decode_streams_batch.py.
The model composes, stream by stream, what the definition says of that stream ALONE - decoder.decode through dec_cases.spec - into the
records and the packed output; nothing here looks at what the code under test computes.  Two things decoder.py does not say come from
today's single-stream host build (dec_cases.host_decode): whether a refusal is probe-stage (the single-stream probe, a call without
room, refuses it) and a refused stream's err_offset."""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

import dec_cases as D
import dec_writer as W
import demux_writer  # noqa: F401  (the container batches of the GPU test take their packets from it)

M = D.M
GUARD, FILL = D.GUARD, D.FILL
BOTH = (("module", True), ("iso", False))
ALWAYS = ("es_bytes", "out_bytes", "err_offset", "status")                       # compared for every stream
SIZED = ("pictures", "width", "height", "frame_bytes")                          # ... for every stream the probe stage accepts
COUNTS = ("gops", "repeated_headers", "chains")                                 # ... for every stream that is OK


class StreamStat(ctypes.Structure):
    """m2v_decode_stream_stat (include/m2v_mi355x.h), 88 bytes"""
    _fields_ = [("es_offset", ctypes.c_uint64), ("out_offset", ctypes.c_uint64), ("rec", D.Stat)]


# ---- the batches ----
@functools.lru_cache(maxsize=None)
def written(w, h, types, seed):
    """a written stream (tests/dec_writer.py) of w x h with pictures of these types, seeded content"""
    rng = np.random.RandomState(seed)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    s, _ = W.stream(w, h, [W.random_picture(rng, t, mbw, mbh, gop=(k == 0)) for k, t in enumerate(types)])
    return W.valid(s)


@functools.lru_cache(maxsize=None)
def oracle64():
    """a 64 x 64 stream of the oracle encoder"""
    s = D.recon_streams()["unref"]["stream"]
    assert M.decoder.sequence_headers(s)[:2] == (64, 64)
    return s


@functools.lru_cache(maxsize=None)
def slice_refusal():
    """(name, stream): the first flip of dec_cases.altered() that the definition refuses and the single-stream probe accepts - refused in
    the slice walk"""
    for name, x in D.altered():
        if name.startswith("flip") and D.spec(x, False)[0] is None and D.spec(x, True)[0] is None and D.host_decode(x, cap=0)[1]["status"] == D.OVERFLOW:
            return name, x
    raise AssertionError("no flip of dec_cases.altered() is refused in a slice")


@functools.lru_cache(maxsize=None)
def batches():
    """name -> the streams of the batch, in order"""
    small, small8 = D.small(7), D.small(8)
    mixed = [W.sized(1, 1)[0], small, W.sized(17, 33)[0], oracle64(), D.recon_streams()["g80"]["stream"]]
    return {
        "one": [small],
        "smallest": [small, small8],
        "mixed": mixed,
        "mixed_reversed": mixed[::-1],
        "verdicts": [small, D.handmade()["picture_type_3"], small8, slice_refusal()[1], W.sized(17, 33)[0], D.truncations()["cut_in_header"], b"", small],
        "two_bad": [small, D.two_bad_slices()[0], small8],
        "three": [small, W.sized(17, 33)[0], small8],
        "chunks": [written(32, 32, (1, 2, 2), 11), written(64, 64, (1, 2), 12), D.ionly_stream(), small],
        "events": [small, W.many_pictures()[0], small8],
        "many": [written(16, 16, (1,), 13)] * 4096,
    }


def place(streams, gap=b"", lead=0):
    """-> (bytes, [(offset, bytes)]): the streams one behind the other, `gap` between them (and in front, behind `lead` zeros)"""
    out, seg = bytes(lead) + gap, []
    for s in streams:
        seg.append((len(out), len(s)))
        out += bytes(s) + gap
    return out, seg


# ---- the model ----
@functools.lru_cache(maxsize=None)
def _alone(stream, mode):
    """what the definition says of one stream alone: (Decoded or None, the single-stream probe's record, the single-stream record)"""
    d, _ = D.spec(stream, mode == "module")
    probe = D.host_decode(stream, "i420", mode, cap=0)[1]
    whole = D.host_decode(stream, "i420", mode)[1] if d is None and probe["status"] != D.SYNTAX else probe
    return d, probe, whole


def expected(batch, layout="i420", mode="iso", cap=None, probe=False):
    """-> dict(records = [dict per stream: the fields of StreamStat.rec that are defined for it, out_offset, stage], out = the packed
    output (FILL where nothing may be written), written = bool per byte, total = the bytes of all rooms).  stage: None (OK),
    "probe", "slice" or "cap".  cap None: everything fits.  probe: what a call without a destination reports"""
    recs, at, parts = [], 0, []
    for s in batch:
        s = bytes(s)
        d, p, whole = _alone(s, mode)
        r = dict(es_bytes=len(s), out_offset=at, out_bytes=0, err_offset=0, status=D.OK, stage=None)
        if p["status"] == D.SYNTAX:
            assert d is None, "the single-stream probe refuses a stream the definition reads"
            r.update(status=D.SYNTAX, err_offset=p["err_offset"], stage="probe")
            recs.append(r)
            continue
        if d is not None:
            r.update(pictures=len(d.pictures), width=d.width, height=d.height, frame_bytes=M.frame_bytes(d.width, d.height, "i420"))
            r.update(gops=len(d.gops), repeated_headers=d.repeated_headers, chains=sum(q["type"] == 1 for q in d.pictures))
        else:                                    # decoder.py raises inside a slice and says nothing: the sizes are the probe's
            r.update({k: p[k] for k in SIZED})
        room = r["pictures"] * r["frame_bytes"]
        if probe:
            r["out_bytes"] = room
        elif cap is not None and at + room > cap:
            r.update(status=D.OVERFLOW, stage="cap")
        elif d is None:
            r.update(status=D.SYNTAX, err_offset=whole["err_offset"], stage="slice")
        else:
            r["out_bytes"] = room
            parts.append((at, D.frames_of(d, layout).reshape(-1)))
        at += room
        recs.append(r)
    out, mask = np.full(at, FILL, np.uint8), np.zeros(at, bool)
    for a, f in parts if not probe else []:
        out[a:a + f.size] = f
        mask[a:a + f.size] = True
    return dict(records=recs, out=out, written=mask, total=at)


def records_of(arr):
    """StreamStat array / numpy structured array -> [dict]"""
    out = []
    for q in arr:
        rec = q.rec if isinstance(q, StreamStat) else q["rec"]
        get = (lambda k: getattr(rec, k)) if isinstance(q, StreamStat) else (lambda k: rec[k])
        r = {k: int(get(k)) for k in D.STAT_FIELDS}
        r["es_offset"] = int(q.es_offset if isinstance(q, StreamStat) else q["es_offset"])
        r["out_offset"] = int(q.out_offset if isinstance(q, StreamStat) else q["out_offset"])
        out.append(r)
    return out


def check(got_records, got_buf, want, base=0, segments=None):
    """got_records: [dict] (records_of); got_buf: the destination as the call left it, filled with FILL beforehand, output byte 0 at
    index `base` (GUARD bytes in front and behind belong to it); want: expected().  Every record field that is defined, every
    output byte, and every byte that must stay FILL - around the output and INSIDE every room that must stay untouched.  Raises
    AssertionError naming the stream and what is wrong with it"""
    recs = want["records"]
    assert len(got_records) == len(recs), "%d records for %d streams" % (len(got_records), len(recs))
    for b, (g, w) in enumerate(zip(got_records, recs)):
        if segments is not None:
            assert g["es_offset"] == segments[b][0], "stream %d: es_offset %d, not %d" % (b, g["es_offset"], segments[b][0])
        assert g["out_offset"] == w["out_offset"], "stream %d: out_offset %d, not %d" % (b, g["out_offset"], w["out_offset"])
        fields = ALWAYS + (SIZED if w["stage"] != "probe" else ()) + (COUNTS if w["stage"] is None else ())
        for k in fields:
            assert g[k] == w[k], "stream %d (%s): %s %d, not %d" % (b, w["stage"] or "ok", k, g[k], w[k])
    got_buf = np.asarray(got_buf)
    out = got_buf[base:base + want["total"]]
    assert out.size == want["total"], "the destination is shorter than the rooms"
    for b, w in enumerate(recs):
        if w["stage"] in ("slice", "cap"):
            a, e = w["out_offset"], w["out_offset"] + w["pictures"] * w["frame_bytes"]
            bad = np.nonzero(out[a:min(e, out.size)] != FILL)[0]
            assert bad.size == 0, "stream %d (%s): byte %d of its room was written" % (b, w["stage"], bad[0])
    bad = np.nonzero(out != want["out"])[0]
    if bad.size:
        o = int(bad[0])
        b = max(k for k, w in enumerate(recs) if w["out_offset"] <= o)
        raise AssertionError("stream %d: output byte %d (its byte %d) is %d, not %d; %d bytes differ" % (b, o, o - recs[b]["out_offset"], out[o], want["out"][o], bad.size))
    assert (got_buf[:base] == FILL).all(), "bytes in front of the output were written"
    assert (got_buf[base + want["total"]:] == FILL).all(), "bytes behind the rooms were written"


# ---- the host build ----
_HARNESS = r"""
#include "dec_host.hpp"
using namespace dec_host;
extern "C" int ds_host_decode(const uint8_t *es, const uint64_t *off, const uint64_t *nb, uint64_t n, int layout, int mode, uint8_t *out, uint64_t cap,
                              uint64_t decode_batch, uint64_t level_bytes, StreamRecord *recs)
{
    std::vector<Segment> seg(n);
    for (uint64_t b = 0; b < n; ++b) seg[b] = Segment{es + off[b], nb[b]};
    const std::vector<StreamRecord> r = decode_streams(seg.data(), n, layout, mode, out, cap, decode_batch, level_bytes ? level_bytes : m2v::dec::kStreamsLevelBytes);
    for (uint64_t b = 0; b < n; ++b) { recs[b] = r[b]; recs[b].es_offset = off[b]; }
    return 0;
}
// the chunks of a decode of everything: (first stream, its picture, pictures) per chunk -> their number
extern "C" int ds_host_chunks(const uint8_t *es, const uint64_t *off, const uint64_t *nb, uint64_t n, uint64_t decode_batch, uint64_t level_bytes, uint32_t *out, int max)
{
    std::vector<Probed> Q(n);
    std::vector<std::vector<uint8_t>> types(n);
    std::vector<m2v::dec::StreamInfo> info(n);
    for (uint64_t b = 0; b < n; ++b) {
        if (nb[b] < 4) Q[b].R.status = m2v::dec::kSyntax; else Q[b] = probe(es + off[b], nb[b]);
        for (const Pic &p : Q[b].pics) types[b].push_back((uint8_t)p.type);
        info[b] = m2v::dec::StreamInfo{Q[b].R.status, Q[b].R.pictures, Q[b].R.width, Q[b].R.height, types[b].data()};
    }
    const m2v::dec::StreamsPlan P = m2v::dec::plan_streams(info.data(), n, ~0ull, false, decode_batch, level_bytes ? level_bytes : m2v::dec::kStreamsLevelBytes);
    int k = 0;
    for (const m2v::dec::StreamsChunk &C : P.chunks) {
        if (k < max) { out[3 * k] = P.pics[C.first].stream; out[3 * k + 1] = P.pics[C.first].pic; out[3 * k + 2] = (uint32_t)C.count; }
        ++k;
    }
    return k;
}
"""
_host = None


def build_host(kernels_dir=None):
    """the harness above over tools/dec_host.hpp, compiled with g++ (no HIP) -> the library.  kernels_dir: a directory searched for
    m2v_decode_kernels.hpp in front of csrc (an altered copy of the header)"""
    d = tempfile.mkdtemp(prefix="m2v_ds_host_")
    src, so = os.path.join(d, "ds_host.cpp"), os.path.join(d, "libds_host.so")
    with open(src, "w") as f:
        f.write(_HARNESS)
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    first = ["-I", kernels_dir] if kernels_dir else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror"] + first + ["-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
    L = ctypes.CDLL(so)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.ds_host_decode.argtypes = [ctypes.c_char_p, u64p, u64p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                 ctypes.c_uint64, ctypes.POINTER(StreamStat)]
    L.ds_host_chunks.argtypes = [ctypes.c_char_p, u64p, u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    return L


def host_lib():
    global _host
    if _host is None:
        _host = build_host()
    return _host


def _segs(seg):
    n = len(seg)
    return (ctypes.c_uint64 * n)(*[a for a, _ in seg]), (ctypes.c_uint64 * n)(*[b for _, b in seg])


def host_decode_streams(data, seg, layout="i420", mode="iso", cap=None, probe=False, decode_batch=0, level_bytes=0, lib=None):
    """-> ([dict per stream], the destination: GUARD + the rooms (cap, if that is more) + GUARD bytes, output byte 0 at index GUARD; None
    for a probe).  cap None: exactly the rooms, asked of a probe first"""
    L = lib or host_lib()
    off, nb = _segs(seg)
    recs = (StreamStat * len(seg))()
    L.ds_host_decode(bytes(data), off, nb, len(seg), M.LAYOUTS_420[layout], D.MODES[mode], None, 0, decode_batch, level_bytes, recs)
    if probe:
        return records_of(recs), None
    total = max(r["out_offset"] + r["out_bytes"] for r in records_of(recs))
    cap = total if cap is None else cap
    room = max(cap, total)                       # (a smaller cap: the rooms behind it are there to be seen untouched)
    buf = np.full(2 * GUARD + room, FILL, np.uint8)
    L.ds_host_decode(bytes(data), off, nb, len(seg), M.LAYOUTS_420[layout], D.MODES[mode], buf.ctypes.data + GUARD, cap, decode_batch, level_bytes, recs)
    return records_of(recs), buf


def host_chunks(data, seg, decode_batch=0, level_bytes=0):
    """[(first stream, its picture, pictures)] per chunk of a decode of the whole batch"""
    off, nb = _segs(seg)
    out = (ctypes.c_uint32 * (3 * 4096))()
    n = host_lib().ds_host_chunks(bytes(data), off, nb, len(seg), decode_batch, level_bytes, out, 4096)
    return [tuple(out[3 * k:3 * k + 3]) for k in range(min(n, 4096))]


def pack_batches(items):
    """[(streams, layout, mode, cap or None, decode_batch)] -> the file tools/dec_host_streams_check reads (its header says the format)"""
    out = [struct.pack("<I", len(items))]
    for streams, layout, mode, cap, decode_batch in items:
        out.append(struct.pack("<IIQII", D.MODES[mode], M.LAYOUTS_420[layout], 0xFFFFFFFFFFFFFFFF if cap is None else cap, decode_batch, len(streams)))
        for s in streams:
            out += [struct.pack("<Q", len(s)), bytes(s)]
    return b"".join(out)
