"""ctypes binding of libm2v_container.so (include/m2v_container.h): elementary-stream scan and MPEG-2 PS / TS
multiplexers.  CPU-only conveniences around the encoder's output; nothing here touches the GPU
path or the encoded bits."""
import ctypes
import importlib
import os

_build = importlib.import_module(__package__ + ".build")     # the package also exports a function called build

_L = None


class StreamInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("frame_rate_code", ctypes.c_uint32),
                ("aspect_ratio_code", ctypes.c_uint32), ("bit_rate_400", ctypes.c_uint32),
                ("pictures", ctypes.c_uint32), ("i_pictures", ctypes.c_uint32), ("p_pictures", ctypes.c_uint32),
                ("gops", ctypes.c_uint32), ("slices", ctypes.c_uint32), ("bytes", ctypes.c_uint64),
                ("padding_bytes", ctypes.c_uint64), ("has_sequence_end", ctypes.c_int)]


class Picture(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("coding_type", ctypes.c_uint32),
                ("temporal_reference", ctypes.c_uint32), ("gop_start", ctypes.c_uint32), ("slices", ctypes.c_uint32)]


class Stamp(ctypes.Structure):
    """m2vc_stamp: one PES packet of a demultiplexed stream; pts / dts = ABSENT when the header carries none"""
    _fields_ = [("es_offset", ctypes.c_uint64), ("pts", ctypes.c_uint64), ("dts", ctypes.c_uint64), ("src_offset", ctypes.c_uint64)]


class DemuxInfo(ctypes.Structure):
    _fields_ = [("out_bytes", ctypes.c_uint64), ("err_offset", ctypes.c_uint64), ("pes_packets", ctypes.c_uint32),
                ("packets", ctypes.c_uint32), ("discontinuities", ctypes.c_uint32), ("skipped", ctypes.c_uint32),
                ("stream", ctypes.c_uint32), ("status", ctypes.c_int32)]


ABSENT = 0xFFFFFFFFFFFFFFFF
E_PARAM, E_SYNTAX, E_OVERFLOW, E_NOSTREAM = -1, -2, -3, -4


class ContainerError(RuntimeError):
    pass


def lib():
    global _L
    if _L is None:
        path = _build.CONTAINER_LIB
        if not os.path.exists(path):
            _build.build_container()
        L = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.m2vc_frame_rate.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.m2vc_scan.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(StreamInfo), vp, sz, ctypes.POINTER(sz)]
        for f in (L.m2vc_mux_ps, L.m2vc_mux_ts):
            f.argtypes = [ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz)]
        for f in (L.m2vc_demux_ps, L.m2vc_demux_ts):
            f.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, vp, sz, vp, sz, ctypes.POINTER(DemuxInfo)]
        _L = L
    return _L


def _chk(r, what):
    if r < 0:
        raise ContainerError("%s failed: %s" % (what, {-1: "bad parameter", -2: "not an elementary stream of this encoder",
                                                      -3: "buffer too small", -4: "no video stream in the container"}.get(r, r)))


def frame_rate(code):
    num, den = ctypes.c_uint32(), ctypes.c_uint32()
    _chk(lib().m2vc_frame_rate(code, ctypes.byref(num), ctypes.byref(den)), "m2vc_frame_rate")
    return num.value, den.value


def scan(es):
    """-> (StreamInfo, [Picture])"""
    es = bytes(es)
    info, n = StreamInfo(), ctypes.c_size_t()
    _chk(lib().m2vc_scan(es, len(es), ctypes.byref(info), None, 0, ctypes.byref(n)), "m2vc_scan")
    pics = (Picture * max(n.value, 1))()
    _chk(lib().m2vc_scan(es, len(es), ctypes.byref(info), pics, n.value, ctypes.byref(n)), "m2vc_scan")
    return info, list(pics[:n.value])


def _mux(fn, what, es):
    es = bytes(es)
    n = ctypes.c_size_t()
    _chk(fn(es, len(es), None, 0, ctypes.byref(n)), what)
    out = ctypes.create_string_buffer(n.value)
    _chk(fn(es, len(es), out, n.value, ctypes.byref(n)), what)
    return out.raw[:n.value]


def mux_ps(es):
    """MPEG-2 Program Stream around the elementary stream `es`."""
    return _mux(lib().m2vc_mux_ps, "m2vc_mux_ps", es)


def mux_ts(es):
    """MPEG-2 Transport Stream around the elementary stream `es`."""
    return _mux(lib().m2vc_mux_ts, "m2vc_mux_ts", es)


def demux_raw(kind, src, stream=None, cap=None, stamp_cap=None):
    """m2vc_demux_ts ("ts") / m2vc_demux_ps ("ps") as they answer: -> (status, DemuxInfo, elementary bytes, [Stamp]).  stream: the PID /
    stream_id, None: found in the container.  cap / stamp_cap: the capacities handed over (None: what the container needs)."""
    fn = {"ts": lib().m2vc_demux_ts, "ps": lib().m2vc_demux_ps}[kind]
    src = bytes(src)
    sid = -1 if stream is None else int(stream)
    info = DemuxInfo()
    r = fn(src, len(src), sid, None, 0, None, 0, ctypes.byref(info))
    if r != 0:
        return r, info, b"", []
    need, pes = info.out_bytes, info.pes_packets
    cap = need if cap is None else int(cap)
    stamp_cap = pes if stamp_cap is None else int(stamp_cap)
    out = ctypes.create_string_buffer(max(cap, 1))
    stamps = (Stamp * max(stamp_cap, 1))()
    r = fn(src, len(src), sid, out, cap, stamps, stamp_cap, ctypes.byref(info))
    if r != 0:
        return r, info, b"", []
    return r, info, out.raw[:info.out_bytes], list(stamps[:min(pes, stamp_cap)])


def _demux(kind, src, stream):
    r, info, es, stamps = demux_raw(kind, src, stream)
    if r == E_SYNTAX:
        raise ContainerError("m2vc_demux_%s failed: the container breaks a rule at offset %d" % (kind, info.err_offset))
    _chk(r, "m2vc_demux_%s" % kind)
    return es, stamps, info


def demux_ts(ts, pid=None):
    """The video elementary stream of a transport stream -> (bytes, [Stamp] one per PES packet, DemuxInfo).  pid None: through PAT / PMT."""
    return _demux("ts", ts, pid)


def demux_ps(ps, stream_id=None):
    """The video elementary stream of a program stream -> (bytes, [Stamp], DemuxInfo).  stream_id None: the first video stream's."""
    return _demux("ps", ps, stream_id)
